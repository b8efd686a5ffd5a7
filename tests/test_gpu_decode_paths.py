"""The LZ4 decoder (csrc/lz4_decode.hip) on hand-built streams, byte for byte
against the CPU oracle's decode of the same bytes.

The streams come from tests/lz4_craft.py -- records no encoder of ours would
emit -- and tests/test_lz4_craft.py asserts on the CPU what each family visits:

  f1  every match path of lz4_exec_block / wave_match x destination x source
      alignment x length edge; far offsets in blocks above the LDS budget
  f2  every literal path x destination x source alignment; short and long
      runs in every order (the in-place decoder's ordered literal loop)
  f3  literal- and match-length extension runs against read_ext's windows
  f4  batching: dependent and independent matches, chunk boundaries, counts
  f5  one long periodic fill per offset (small_mod up to 96 KiB)
  f6  blocks of 16..128 bytes, a partial last block, raw tails
  f7  a last block on either side of the in-place margin test

Each runs through the record-access variants (default in place, 16 global +
touch, 32 global, 64 own LDS buffer), the element sizes' output paths, the
host and device entry points, and blocks above the LDS budget run
k_seq_scan_big + k_lz4_exec_big.  No tolerances: tobytes() equality, and the
consumed length (the API wrappers raise unless it equals the stream length).
"""
import ctypes

import numpy as np
import pytest

from tests import lz4_craft as C
from tests.test_lz4_craft import HostCheck

pytestmark = pytest.mark.gpu

DEC_VARIANTS = [0, 16, 32, 64]
STATIC = 1 << 24      # bshuf_set_variant bit: static block assignment
DTYPES = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}
FAMILIES_8K = ["f1_8192", "f2_8192", "f3_8192", "f4_8192", "f5_8192"]


@pytest.fixture(scope="module")
def bs():
    import bitshuffle_amd
    assert bitshuffle_amd.using_HIP(), "no HIP device: the GPU suite must run on MI355X"
    return bitshuffle_amd


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture
def variant(bs):
    def set_(v):
        assert bs.lib.bshuf_set_variant(v) == 0, v
    yield set_
    assert bs.lib.bshuf_set_variant(0) == 0


def dtype_of(E):
    return np.dtype(DTYPES[E]) if E in DTYPES else np.dtype("V%d" % E)


class Case:
    """A framed stream, what it decodes to (the oracle, computed once) and how
    to call the decoder on it."""

    def __init__(self, oracle, pays, n, E=1, tail_elems=0, last=None, tail=None):
        assert n % (8 * E) == 0
        self.E, self.block = E, n // E
        elems = len(pays) * self.block + tail_elems
        pays = list(pays)
        if last is not None:    # a partial last block of `last[1]` bytes
            assert last[1] % (8 * E) == 0 and last[1] < n
            pays.append(last[0])
            elems += last[1] // E
        if tail is None:
            tail = C.Lits(n + E).take(tail_elems * E)
        self.buf = C.stream(pays, tail)
        self.shape, self.dtype = (elems,), dtype_of(E)
        self.want = oracle.decompress_lz4(self.buf, self.shape, self.dtype, self.block).tobytes()
        assert len(self.want) == elems * E

    def host(self, bs):
        got = bs.decompress_lz4(self.buf, self.shape, self.dtype, self.block)
        assert got.tobytes() == self.want

    def dev(self, bs, torch, **kw):
        t = torch.from_numpy(self.buf.copy()).cuda()
        y = bs.decompress_lz4_dev(t, self.shape, torch.uint8, self.block, elem_size=self.E, **kw)
        assert y.cpu().numpy().tobytes() == self.want


@pytest.fixture(scope="module")
def case(oracle):
    """(name, E) -> Case, built once per module."""
    cache = {}

    def get(name, E=1, **kw):
        key = (name, E, tuple(sorted(kw.items())))
        if key not in cache:
            n, pays = C.cases()[name]
            cache[key] = Case(oracle, pays, n, E, **kw)
        return cache[key]
    return get


# 1. every family at 8 KiB under every record-access path
@pytest.mark.parametrize("v", DEC_VARIANTS)
@pytest.mark.parametrize("name", FAMILIES_8K)
def test_families_under_every_record_path(bs, case, variant, name, v):
    variant(v)
    case(name).host(bs)


# 2. 1 KiB blocks: eight records per in-place buffer's worth of LDS
@pytest.mark.parametrize("v", DEC_VARIANTS)
def test_match_and_dependency_grids_in_1k_blocks(bs, case, variant, v):
    variant(v)
    case("f1_1024").host(bs)
    case("f4_1024").host(bs)


# 3. small and ragged blocks: 16..128 bytes, a partial last block, raw tails
@pytest.mark.parametrize("v", DEC_VARIANTS)
def test_small_blocks_partial_block_and_tails(bs, oracle, case, variant, v):
    variant(v)
    for n in C.F6_SIZES:
        for tail_elems in (0, 1, 7):    # 8 E - 1 = 7 bytes at E = 1
            case("f6_%d" % n, tail_elems=tail_elems).host(bs)
    pays = C.cases()["f6_128"][1]
    for m in (16, 72):
        for tail_elems in (0, 1, 7):
            Case(oracle, pays, 128, last=(C.cases()["f6_%d" % m][1][-1], m), tail_elems=tail_elems).host(bs)
    # 8 KiB blocks, a 1 KiB partial block (64 chained matches) and 7 elements
    chain = dict(C.f4_named(1024))["chain64"]
    for E in (1, 2):
        Case(oracle, C.cases()["f4_8192"][1], 8192, E, last=(chain, 1024), tail_elems=7).host(bs)


# 4. one long periodic fill per offset; 64 KiB: LDS-resident with far offsets;
# 96 KiB: k_seq_scan_big + k_lz4_exec_big
@pytest.mark.parametrize("n", [8192, 65536, C.BIG])
def test_long_periodic_fills(bs, torch, case, variant, n):
    c = case("f5_%d" % n)
    for v in (DEC_VARIANTS if n == 65536 else [0]):
        variant(v)
        c.host(bs)
    variant(0)
    c.dev(bs, torch)


# 5. crafted streams through the global-memory executor (gbl_match, its
# batching and its fences)
@pytest.mark.parametrize("fam", ["f1", "f3", "f4"])
def test_large_blocks_through_the_global_executor(bs, torch, case, fam):
    c = case("%s_%d" % (fam, C.BIG))
    assert c.block * c.E > 81920 and len(c.buf) < 10 * (4 + C.lz4_bound(C.BIG))
    c.host(bs)
    c.dev(bs, torch)


# 6. element sizes: the EK register transposes (1, 2, 4, 8), any element size
# through registers (3, 12: stage_off = -1)
@pytest.mark.parametrize("E", [1, 2, 4, 8, 3, 12])
def test_element_sizes(bs, torch, case, E):
    n = C.E_SIZES.get(E, 8192)
    for fam in ("f1", "f2"):
        c = case("%s_%d" % (fam, n), E)
        c.host(bs)
        c.dev(bs, torch)


def test_e3_with_16k_blocks_stages_in_lds(bs, torch, case):
    n = C.E_SIZES[(3, "16k")]
    assert n > 8192
    for fam in ("f1", "f2"):
        c = case("%s_%d" % (fam, n), 3)
        c.host(bs)
        c.dev(bs, torch)


def test_e3_at_the_largest_lds_blocks(bs, torch, case, variant):
    """81,600-byte blocks of 3-byte elements: the block, its in-place record
    region and an LDS staging block together exceed the CU's 160 KiB, so the
    output goes out with byte stores (a launch asking for all three is
    refused, error -70).  Variant 64 is in the same position from 54 KiB on."""
    c = case("f5_%d" % C.LDS_TOP, 3)
    assert 81552 < c.block * c.E <= 81720
    for v in DEC_VARIANTS:
        variant(v)
        c.host(bs)
    variant(0)
    c.dev(bs, torch)


def test_e3_into_an_odd_output_pointer_stores_bytes(bs, torch, case):
    """An output that is not 8-byte aligned takes the byte-store path
    (stage_off = 0), as in test_device_api_unaligned_pointers."""
    for fam in ("f1", "f2"):
        c = case("%s_%d" % (fam, C.E_SIZES[3]), 3)
        nbytes = len(c.want)
        src = torch.from_numpy(c.buf.copy()).cuda()
        back = torch.zeros(nbytes + 64, dtype=torch.uint8, device="cuda")
        res = torch.zeros(1, dtype=torch.int64, device="cuda")
        rc = bs.lib.bshuf_decompress_lz4_dev(ctypes.c_void_p(src.data_ptr()), src.numel(),
                                             ctypes.c_void_p(back.data_ptr() + 1), c.shape[0], 3,
                                             c.block, None, 0, ctypes.c_void_p(res.data_ptr()), None, None)
        assert rc == 0 and int(res.item()) == src.numel()
        got = back.cpu().numpy()
        assert got[1:1 + nbytes].tobytes() == c.want
        assert got[0] == 0 and not got[1 + nbytes:].any(), "nothing outside the output"


# 7. entry points: the device API without offsets (parallel index rebuild), a
# device-held length with a larger capacity, the batch API
@pytest.mark.parametrize("name", FAMILIES_8K)
def test_device_api_index_rebuild(bs, torch, case, name):
    case(name).dev(bs, torch)


def test_device_length_with_a_larger_capacity(bs, torch, case):
    for name in ("f2_8192", "f4_8192"):
        c = case(name, tail_elems=5)
        cap = torch.full((len(c.buf) + 5000,), 0xF0, dtype=torch.uint8, device="cuda")
        cap[:len(c.buf)] = torch.from_numpy(c.buf.copy()).cuda()
        length = torch.tensor([len(c.buf)], dtype=torch.int64, device="cuda")
        y = bs.decompress_lz4_dev(cap, c.shape, torch.uint8, c.block, length=length)
        assert y.cpu().numpy().tobytes() == c.want


def test_batch_of_two_crafted_streams_and_an_encoded_one(bs, oracle, torch, case):
    a = oracle.gen_g1(9 * 4096 + 1000 + 3)
    enc = oracle.compress_lz4(a, 4096)
    cs = [case("f3_8192", 2), case("f4_8192", 2, tail_elems=3)]
    assert len({len(c.buf) for c in cs}) == 2 and cs[0].shape != cs[1].shape
    bufs = [torch.from_numpy(c.buf.copy()).cuda() for c in cs] + [torch.from_numpy(enc.copy()).cuda()]
    shapes = [c.shape for c in cs] + [a.shape]
    outs = bs.decompress_lz4_batch_dev(bufs, shapes, torch.int16, 4096)
    for o, want in zip(outs, [c.want for c in cs] + [a.tobytes()]):
        assert o.cpu().numpy().tobytes() == want


# 8. the static schedule: every wave decodes blocks w, w + G, ... of the
# dependency grid one after another (9,500 blocks over 4,608 resident waves),
# so a record that lands while the previous block's output is leaving shows
def test_dependency_grid_under_the_static_schedule(bs, oracle, torch, variant):
    n, pays = C.cases()["f4_8192"]
    c = Case(oracle, pays * 380, n)
    for v in (STATIC, 0):
        variant(v)
        c.dev(bs, torch)


# 9. the in-place margin: the last block of a stream with a long raw tail fails
# the test and is read from global memory; the tightest streams on either side
def test_in_place_margin_either_side(bs, oracle, torch, variant):
    host = HostCheck()
    built = [(E,) + C.f7(E) for E in C.F7_ES]
    fit = [b for b in built if host.last_block_fits(*b[1:])]
    no = [b for b in built if not host.last_block_fits(*b[1:])]
    assert len(fit) >= 8 and len(no) >= 8
    picked = sorted(fit, key=lambda b: -b[0])[:3] + sorted(no, key=lambda b: b[0])[:3]
    picked.append((C.F7_LARGE[0],) + C.f7(*C.F7_LARGE))    # 64 KiB blocks, fails the test
    for E, st, pays, n in picked:
        c = Case(oracle, pays, n, E, tail_elems=C.F7_TAIL, tail=st[len(C.frame(pays)):].tobytes())
        assert c.buf.tobytes() == st.tobytes()
        for v in DEC_VARIANTS:
            variant(v)
            c.host(bs)
        variant(0)
        c.dev(bs, torch)
