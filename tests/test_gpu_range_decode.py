"""Random-access decode (bshuf_decompress_lz4_ranges_dev): element ranges of a
framed stream, byte for byte against slices of the CPU oracle's decode of the
same stream.

The streams are the oracle's (the reference encoder's bytes).  Every call
writes into an output that is 64 bytes longer than the ranges need and filled
with 0xA5, and those 64 bytes must come back untouched.  Every case runs with
the block index supplied (compress_lz4_dev's `offsets=` of the same data; once
block_index_dev's) and with the index rebuilt by the call.  No tolerances:
tobytes() equality."""
import numpy as np
import pytest

from tests import lz4_craft as C

pytestmark = pytest.mark.gpu

ES = [1, 2, 4, 8, 3, 12]
GUARD = 64


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


class Stream:
    """A framed stream on the device, its block index and the bytes it decodes to."""

    def __init__(self, bs, torch, oracle, buf, size, E, block, want=None, index=True):
        self.bs, self.torch = bs, torch
        self.size, self.E, self.block = size, E, block
        dt = np.dtype({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}.get(E, "V%d" % E))
        if want is None:
            want = oracle.decompress_lz4(buf, (size,), dt, block)
        self.want = np.frombuffer(want.tobytes(), dtype=np.uint8)
        assert self.want.size == size * E
        self.host = np.ascontiguousarray(buf, dtype=np.uint8)
        self.buf = torch.from_numpy(self.host.copy()).cuda()
        self.nb = int(bs.lib.bshuf_lz4_dev_nblocks(size, E, block))
        self.offs = None
        if index:
            # the encoder's index: compress the decoded bytes again on the device
            raw = torch.from_numpy(self.want.copy()).cuda()
            self.offs = torch.full((max(self.nb, 1),), -1, dtype=torch.int64, device="cuda")
            c = bs.compress_lz4_dev(raw, block, offsets=self.offs, elem_size=E)
            assert c.cpu().numpy().tobytes() == self.host.tobytes(), "encode differs from the oracle"

    def expect(self, ranges):
        E = self.E
        parts = [self.want[s * E:(s + c) * E] for s, c in ranges]
        return np.concatenate(parts).tobytes() if parts else b""

    def out_tensor(self, ranges, shift=0):
        n = sum(c for _, c in ranges) * self.E
        whole = self.torch.full((shift + n + GUARD,), 0xA5, dtype=self.torch.uint8, device="cuda")
        return whole[shift:], n

    def check_out(self, out, n, ranges):
        got = out.cpu().numpy()
        assert got[:n].tobytes() == self.expect(ranges), ranges[:4]
        assert got[n:].tobytes() == b"\xa5" * GUARD, "bytes behind the ranges were written"

    def run(self, ranges, offsets="own", shift=0, buf=None, **kw):
        ranges = list(ranges)
        out, n = self.out_tensor(ranges, shift)
        offs = self.offs if isinstance(offsets, str) else offsets
        views = self.bs.decompress_lz4_ranges_dev(self.buf if buf is None else buf, self.size,
                                                  self.torch.uint8, ranges, self.block, out=out,
                                                  offsets=offs, elem_size=self.E, **kw)
        self.check_out(out, n, ranges)
        assert len(views) == len(ranges)
        for v, (s, c) in zip(views, ranges):
            assert v.numel() == c * self.E
        return views

    def both(self, ranges, **kw):
        """With the index supplied, and rebuilt."""
        self.run(ranges, **kw)
        self.run(ranges, offsets=None, **kw)


def raw_bytes(oracle, nbytes, gen):
    """Compressible bytes: the oracle's G1 (int16 counts) or G2 (float32) data."""
    if gen == 1:
        a = oracle.gen_g1((nbytes + 1) // 2)
    else:
        a = oracle.gen_g2((nbytes + 3) // 4)
    return np.ascontiguousarray(a).view(np.uint8)[:nbytes].copy()


@pytest.fixture(scope="module")
def make(bs, torch, oracle):
    cache = {}

    def get(E, block, size, gen=1):
        key = (E, block, size, gen)
        if key not in cache:
            dt = np.dtype({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}.get(E, "V%d" % E))
            data = raw_bytes(oracle, size * E, gen).view(dt)
            buf = oracle.compress_lz4(data, block)
            cache[key] = Stream(bs, torch, oracle, buf, size, E, block)
            assert cache[key].want.tobytes() == data.tobytes()
        return cache[key]
    return get


def block_of(bs, E, which):
    return 128 if which == "128" else bs.default_block_size(E)


def main_size(b):
    return 5 * b + 24 + 5   # five full blocks, a partial block of 24, a 5-element tail


def single_ranges(b, size):
    """The issue's single ranges for the main shape; for the smaller sizes,
    those of them that fit."""
    r = [
        (0, size),                       # the whole array
        (min(7, size), 0),               # empty
        (b // 2 + 3, 1),                 # one element in the middle of a block
        (b + 5, b - 11),                 # wholly inside one block
        (b - 3, 9),                      # straddling one block boundary
        (b, 2 * b),                      # exactly on block boundaries
        (4 * b + 7, b - 7 + 11),         # ending inside the partial block
        (5 * b, 24 + 5),                 # the partial block plus the tail
        (5 * b + 24 + 2, 3),             # starting inside the tail
    ]
    if size:
        r.append((size - 1, 1))          # the last element
    return [x for x in r if x[0] + x[1] <= size]


@pytest.mark.parametrize("which", ["128", "default"])
@pytest.mark.parametrize("E", ES)
def test_single_ranges(bs, make, E, which):
    b = block_of(bs, E, which)
    for size in (main_size(b), 2 * b, 5, 0):
        st = make(E, b, size, gen=1 if E != 4 else 2)
        rs = single_ranges(b, size)
        assert len(rs) == (10 if size == main_size(b) else {2 * b: 6, 5: 3, 0: 2}[size])
        for r in rs:
            st.both([r])


@pytest.mark.parametrize("which", ["128", "default"])
@pytest.mark.parametrize("E", ES)
def test_range_lists(bs, make, E, which):
    b = block_of(bs, E, which)
    size = main_size(b)
    st = make(E, b, size, gen=1 if E != 4 else 2)
    st.both([(b - 5, b + 9), (b + 1, 2 * b)])                       # an overlapping pair
    st.both([(2 * b + 3, b), (2 * b + 3, b)])                       # a repeated range
    st.both([(5 * b + 20, 9), (3 * b, b), (b + 1, 7), (0, 3)])      # descending order
    rng = np.random.default_rng(0)
    many = []
    for _ in range(300):                                            # more pieces than one workgroup
        start = int(rng.integers(0, size + 1))
        many.append((start, int(rng.integers(0, min(3 * b, size - start) + 1))))
    st.both(many)


@pytest.mark.parametrize("E", [1, 3])
def test_unaligned_output(bs, make, E):
    """`out` starts 3 bytes into a tensor: no destination is 16-byte aligned."""
    b = 128
    st = make(E, b, main_size(b))
    for rs in ([(0, st.size)], [(b, 2 * b)], [(b - 3, 9), (5 * b, 29), (2 * b + 1, 3 * b)]):
        st.run(rs, shift=3)
        st.run(rs, shift=3, offsets=None)


def test_index_from_block_index_dev(bs, make):
    st = make(2, 128, main_size(128))
    offs = bs.api.block_index_dev(st.buf, st.size, 2, 128)
    assert offs.cpu().tolist() == st.offs.cpu().tolist()
    st.run([(100, 300), (5 * 128 + 20, 9)], offsets=offs)


def test_caller_workspace(bs, torch, make):
    st = make(2, 128, main_size(128))
    rs = [(3, 200), (4 * 128 + 7, 128 + 20)]
    ws = bs.decompress_lz4_ranges_workspace(st.buf.numel(), st.size, 2, rs, 128)
    n = int(bs.lib.bshuf_decompress_lz4_ranges_dev_workspace(
        st.buf.numel(), st.size, 2, 128, *_size_arrays(rs), len(rs)))
    assert ws.numel() == n and ws.data_ptr() % 256 == 0
    st.run(rs, workspace=ws)
    st.run(rs, workspace=ws, offsets=None)
    for offsets in ("own", None):
        with pytest.raises(bs.BshufError) as e:
            st.run(rs, workspace=ws[:n - 1], offsets=offsets)
        assert e.value.args[1] == -71


def _size_arrays(rs):
    import ctypes
    a = (ctypes.c_size_t * len(rs))(*[s for s, _ in rs])
    b = (ctypes.c_size_t * len(rs))(*[c for _, c in rs])
    return a, b


def test_host_errors(bs, make):
    st = make(2, 128, main_size(128))
    for r in ((st.size, 1), (st.size - 3, 4), (0, st.size + 1), (2 ** 64 - 1, 2)):
        with pytest.raises(bs.BshufError) as e:
            bs.decompress_lz4_range_dev(st.buf, st.size, st.torch.int16, *r, block_size=128)
        assert e.value.args[1] == -71, r
    with pytest.raises(bs.BshufError) as e:
        bs.decompress_lz4_range_dev(st.buf, st.size, st.torch.int16, 0, 8, block_size=12)
    assert e.value.args[1] == -81


def test_typed_output_and_one_range(bs, torch, make):
    """Without elem_size the output has the dtype asked for; no ranges give 0 bytes."""
    st = make(2, 128, main_size(128))
    for offsets in (st.offs, None):
        y = bs.decompress_lz4_range_dev(st.buf, st.size, torch.int16, 130, 300, block_size=128,
                                        offsets=offsets)
        assert y.dtype == torch.int16 and y.numel() == 300
        assert y.cpu().numpy().tobytes() == st.expect([(130, 300)])
        out, res = bs.decompress_lz4_ranges_dev(st.buf, st.size, torch.int16, [], 128, offsets=offsets,
                                                sync=False)
        torch.cuda.synchronize()
        assert int(res.item()) == 0 and out.numel() == 0
    with pytest.raises(ValueError):
        bs.decompress_lz4_range_dev(st.buf.cpu(), st.size, torch.int16, 0, 8, block_size=128)
    with pytest.raises(ValueError):
        bs.decompress_lz4_range_dev(st.buf[::2], st.size, torch.int16, 0, 8, block_size=128)


def crafted(bs, torch, oracle, pays, n, **kw):
    from tests.test_gpu_decode_paths import Case
    c = Case(oracle, pays, n, 1, **kw)
    want = np.frombuffer(c.want, dtype=np.uint8)
    return Stream(bs, torch, oracle, c.buf, c.shape[0], 1, c.block, want=want, index=False)


def test_crafted_small_blocks(bs, torch, oracle):
    """lz4_craft's f6 family: tiny blocks, a partial last block, raw tails."""
    for n in C.F6_SIZES:
        pays = C.cases()["f6_%d" % n][1]
        for kw in (dict(tail_elems=0), dict(tail_elems=7)):
            st = crafted(bs, torch, oracle, pays, n, **kw)
            offs = bs.api.block_index_dev(st.buf, st.size, 1, n)
            rs = [(n + 3, n - 5), (n - 2, n + 4), (st.size - n - 3, n + 3)]
            for r in rs:
                st.run([r], offsets=offs)
                st.run([r], offsets=None)
    pays = C.cases()["f6_128"][1]
    for m in (16, 72):
        st = crafted(bs, torch, oracle, pays, 128, last=(C.cases()["f6_%d" % m][1][-1], m), tail_elems=7)
        offs = bs.api.block_index_dev(st.buf, st.size, 1, 128)
        full = len(pays) * 128
        for r in ((full - 9, 9 + m // 2), (full, m + 7), (full + m - 1, 5)):
            st.run([r], offsets=offs)
            st.run([r], offsets=None)


def test_crafted_8k_blocks(bs, torch, oracle):
    n, pays = C.cases()["f1_8192"]
    st = crafted(bs, torch, oracle, pays, n, tail_elems=5)
    offs = bs.api.block_index_dev(st.buf, st.size, 1, n)
    for r in ((100, 50), (n - 10, 30), (2 * n + 17, st.size - 2 * n - 17)):
        st.run([r], offsets=offs)
        st.run([r], offsets=None)


def test_large_blocks(bs, make):
    """96 KiB blocks: above the LDS decoder's size, one piece at a time through
    k_seq_scan_big + k_lz4_exec_big."""
    b = 49152
    st = make(2, b, 2 * b + 16 + 3)
    assert st.nb == 3
    rs = [(b + 100, 1000), (b - 50, 100), (2 * b + 5, 14)]
    for r in rs:
        st.both([r])
    st.both(rs)


def test_corrupt_block_with_offsets(bs, torch, make):
    b = 128
    st = make(2, b, main_size(b))
    bad = st.buf.clone()
    o2 = int(st.offs[2].item())
    bad[o2:o2 + 4] = torch.tensor([0x7F, 0xFF, 0xFF, 0xFF], dtype=torch.uint8, device="cuda")
    # ranges that do not touch block 2 decode to the clean data's slices
    st.run([(10, 200)], buf=bad)
    st.run([(3 * b + 5, b + 20)], buf=bad)
    st.run([(10, 200), (3 * b + 5, b + 20), (5 * b + 3, 26)], buf=bad)
    # one that does fails as the whole decode of that stream does
    with pytest.raises(bs.BshufError) as whole:
        bs.decompress_lz4_dev(bad, (st.size,), torch.int16, b, offsets=st.offs)
    assert whole.value.args[1] < 0
    for rs in ([(2 * b + 1, 5)], [(b + 100, 60)], [(0, 5), (2 * b, b), (4 * b, 5)]):
        with pytest.raises(bs.BshufError) as e:
            st.run(rs, buf=bad)
        assert e.value.args[1] == whole.value.args[1], rs


def test_asynchronous_use(bs, torch, make):
    st = make(4, 128, main_size(128), gen=2)
    rs = [(7, 300), (5 * 128 + 1, 28), (128, 128)]
    for offsets in (st.offs, None):
        out, n = st.out_tensor(rs)
        o, res = bs.decompress_lz4_ranges_dev(st.buf, st.size, torch.uint8, rs, 128, out=out,
                                              offsets=offsets, elem_size=4, sync=False)
        torch.cuda.synchronize()
        assert o is out and int(res.item()) == n
        st.check_out(out, n, rs)
    # on a stream of its own
    side = torch.cuda.Stream()
    out, n = st.out_tensor(rs)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        o, res = bs.decompress_lz4_ranges_dev(st.buf, st.size, torch.uint8, rs, 128, out=out,
                                              offsets=st.offs, elem_size=4, sync=False)
        o2, res2 = bs.decompress_lz4_ranges_dev(st.buf, st.size, torch.uint8, rs, 128,
                                                elem_size=4, sync=False, stream=side)
    side.synchronize()
    assert int(res.item()) == n and int(res2.item()) == n
    st.check_out(out, n, rs)
    assert o2.cpu().numpy().tobytes() == st.expect(rs)
