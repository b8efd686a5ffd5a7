"""The parallel block-index rebuild (csrc/lz4_decode.hip: k_idx_exits,
k_idx_exits_join, chunk_entry, k_idx_walk, k_idx_check) on streams whose
literals carry decoy header chains, against the serial walk and the oracle's
decode of the same bytes.  Byte-exact, no tolerances.

tests/index_model.py builds the streams and tests/test_index_model.py asserts
on the CPU what each one visits: ambiguous chunks and runs of them (D1, D2,
the random streams), candidate lists above kIdxCandCap (D3), split windows
joined by k_idx_exits_join (D4).  Every device call that finds its headers
without `offsets=` goes through the rebuild: the index itself, the whole
decode, the device-held length, the batch, ranges, windows and stream sets.
"""
import numpy as np
import pytest

from tests import index_model as M
from tests.test_index_model import EVERYTHING

pytestmark = pytest.mark.gpu

GUARD = 64
WINDOW_CASES = [e for e in EVERYTHING if e[1] in ("d1", "d2")]


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


def np_dtype(E):
    return np.dtype(np.uint8) if E == 1 else np.dtype("V%d" % E)


@pytest.fixture(scope="module")
def streams(oracle):
    """(builder, args) -> the stream with its oracle decode (want) and its
    serial index (index); built once per module."""
    cache = {}

    def get(name, *args):
        key = (name,) + args
        if key not in cache:
            c = getattr(M, name)(*args)
            c.want = oracle.decompress_lz4(c.buf, (c.size,), np_dtype(c.E), c.block).tobytes()
            c.index = M.serial_index(c.buf, c.Cb, c.nb)
            cache[key] = c
        return cache[key]
    return get


def to_dev(torch, buf):
    return torch.from_numpy(np.ascontiguousarray(buf).copy()).cuda()


def guarded(torch, nbytes):
    """(whole, out): out is `nbytes` between two 64-byte guards of 0xA5."""
    whole = torch.full((GUARD + nbytes + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    return whole, whole[GUARD:GUARD + nbytes]


def guards_untouched(whole):
    h = whole.cpu().numpy()
    return bool((h[:GUARD] == 0xA5).all() and (h[-GUARD:] == 0xA5).all())


def decode(bs, torch, c, t, **kw):
    """decompress_lz4_dev of stream tensor t into a guarded output."""
    whole, out = guarded(torch, c.size * c.E)
    bs.decompress_lz4_dev(t, (c.size,), torch.uint8, c.block, out=out, elem_size=c.E, **kw)
    torch.cuda.synchronize()
    assert guards_untouched(whole)
    return out.cpu().numpy().tobytes()


# 1. the index, the whole decode and the device-held length, every stream
@pytest.mark.parametrize("name,args", [e[1:] for e in EVERYTHING], ids=[e[0] for e in EVERYTHING])
def test_index_decode_and_device_held_length(bs, torch, streams, name, args):
    c = streams(name, *args)
    t = to_dev(torch, c.buf)
    got = bs.api.block_index_dev(t, c.size, c.E, c.block)
    assert got.cpu().numpy().tolist() == c.index.tolist()
    assert decode(bs, torch, c, t) == c.want
    # the same stream in a buffer of twice its size and more, whose slack holds
    # nothing but plausible headers: chunks past the end, and the last chunk's
    # candidates behind Cb
    cap = 2 * len(c.buf) + 4096 + 3
    big = np.frombuffer(M.words16(cap), dtype=np.uint8).copy()
    big[:len(c.buf)] = c.buf
    length = torch.tensor([len(c.buf)], dtype=torch.int64, device="cuda")
    assert decode(bs, torch, c, to_dev(torch, big), length=length) == c.want


# 2. the batch: decoys on both sides of a stream boundary
def test_batch_with_decoys_on_both_sides_of_an_encoded_stream(bs, torch, oracle, streams):
    a = oracle.gen_g1((20 * 8192 + 1000 + 3) // 2).view(np.uint8)      # full blocks, a partial one, a tail
    enc = oracle.compress_lz4(a, 8192)
    cs = [streams("d1_8k"), None, streams("d2", "a", "e1")]
    bufs = [cs[0].buf, enc, cs[2].buf]
    want = [cs[0].want, a.tobytes(), cs[2].want]
    outs = [guarded(torch, len(w)) for w in want]
    ts = [to_dev(torch, b) for b in bufs]
    bs.decompress_lz4_batch_dev(ts, [(len(w),) for w in want], torch.uint8, 8192, outs=[o for _, o in outs],
                                elem_size=1)
    torch.cuda.synchronize()
    for (whole, out), w in zip(outs, want):
        assert guards_untouched(whole)
        assert out.cpu().numpy().tobytes() == w


# 3. ranges, windows and stream sets: three pieces per stream
def pieces(c):
    """[(start, count)] in elements: inside the ambiguous chunk 1, across its
    exit, and the last block with the tail."""
    w = c.block + 40
    k_in = int(np.searchsorted(c.starts, c.g.CH + c.g.CH // 2))
    k_exit = int(np.searchsorted(c.starts, 2 * c.g.CH))       # the block whose header is chunk 1's exit
    assert c.size - w <= (c.nb - 1) * c.block
    return [(k_in * c.block + 5, w), (k_exit * c.block - w // 2, w), (c.size - w, w)]


@pytest.mark.parametrize("name,args", [e[1:] for e in WINDOW_CASES], ids=[e[0] for e in WINDOW_CASES])
def test_ranges_windows_and_sets(bs, torch, streams, name, args):
    c = streams(name, *args)
    t = to_dev(torch, c.buf)
    pcs = pieces(c)
    w = pcs[0][1]
    want = [c.want[s * c.E:(s + n) * c.E] for s, n in pcs]
    got = bs.decompress_lz4_ranges_dev(t, c.size, torch.uint8, pcs, c.block, elem_size=c.E)
    assert [g.cpu().numpy().tobytes() for g in got] == want
    starts = torch.tensor([s for s, _ in pcs], dtype=torch.int64, device="cuda")
    got = bs.decompress_lz4_windows_dev(t, c.size, torch.uint8, starts, w, c.block, elem_size=c.E)
    assert [g.tobytes() for g in got.cpu().numpy()] == want
    # a set of the stream and a clean one of its shape, indexes rebuilt by the set
    other = streams("clean", c.E, c.block, 20)
    sset = bs.lz4_stream_set_dev([to_dev(torch, other.buf), t], [other.size, c.size], c.E, c.block)
    assert sset.status.cpu().tolist() == [0, 0]
    ids = torch.tensor([1, 0, 1, 1], dtype=torch.int64, device="cuda")
    st4 = torch.tensor([pcs[0][0], 3, pcs[1][0], pcs[2][0]], dtype=torch.int64, device="cuda")
    got = bs.decompress_lz4_windows_set_dev(sset, torch.uint8, ids, st4, w, elem_size=c.E)
    assert [g.tobytes() for g in got.cpu().numpy()] == [want[0], other.want[3 * c.E:(3 + w) * c.E], want[1], want[2]]


# 4. one caller workspace, dirty, for calls back to back
@pytest.mark.parametrize("fill", [0xFF, 0x00])
def test_dirty_workspace_back_to_back(bs, torch, streams, fill):
    """The split path keeps the slices' extremes in `exits` and `cnt`, which it
    fills itself: nothing may lean on what the workspace held or on what the
    call before left there."""
    seq = [streams("d2", "a", "e1"), streams("clean", 1, 8192, M.D2_BLOCKS), streams("d4", "join_s1"),
           streams("clean", 1, M.D4_BLOCK, 9), streams("d4", "join_s0"), streams("d3", "thousands")]
    need = max(int(bs.lib.bshuf_decompress_lz4_dev_workspace(len(c.buf), c.size, c.E, c.block)) for c in seq)
    ws = torch.full((need + 256,), fill, dtype=torch.uint8, device="cuda")
    for c in seq:
        assert decode(bs, torch, c, to_dev(torch, c.buf), workspace=ws) == c.want, c.note


# 5. broken chains beside a live decoy
def _zero(c, k):
    b = c.buf.copy()
    b[c.starts[k]:c.starts[k] + 4] = 0
    return b


def _plus_one(c, k):
    b = c.buf.copy()
    v = int.from_bytes(b[c.starts[k]:c.starts[k] + 4].tobytes(), "big") + 1
    b[c.starts[k]:c.starts[k] + 4] = np.frombuffer(v.to_bytes(4, "big"), dtype=np.uint8)
    return b


def _cut_at_last_decoy(c, k):
    return c.buf[:c.planted[-1]].copy()     # the decoy chain ends exactly here, the true one runs past it


def _destroy(c, k):
    b = c.buf.copy()
    b[c.starts[k]:c.starts[k] + 4] = 0xFF
    return b


BROKEN = {
    # name: (stream, neighbours in the batch, corruption, block it hits, zero-length header)
    "d1-zero": (("d1", "dies"), (("d1", "exact"), ("d1", "dies")), _zero, 2900, True),
    "d1-plus-one": (("d1", "dies"), (("d1", "exact"), ("d1", "dies")), _plus_one, 2900, False),
    "d1-cut-at-decoy": (("d1", "dies"), (("d1", "exact"), ("d1", "dies")), _cut_at_last_decoy, None, False),
    "d2a-behind-ambiguous": (("d2", "a", "e1"), (("d1_8k",), ("d2", "b", "e1")), _destroy, "exit", False),
}


def _code(exc):
    assert len(exc.value.args) > 1, exc.value
    return int(exc.value.args[1])


@pytest.mark.parametrize("case", list(BROKEN))
def test_broken_chain_beside_a_live_decoy(bs, torch, oracle, streams, case):
    key, nbrs, corrupt, k, zero_len = BROKEN[case]
    c = streams(*key)
    if k == "exit":
        k = int(np.searchsorted(c.starts, 2 * c.g.CH))     # the true header behind the ambiguous chunk
    bad = corrupt(c, k)
    # the serial walk first: what it does is what the device must do
    with pytest.raises(ValueError):
        M.serial_index(bad, len(bad) - c.tail, c.nb)
    pinned = False
    if len(bad) == len(c.buf):
        # (the host entry points take no stream length, as the reference's:
        # a cut stream is not theirs to refuse)
        with pytest.raises(RuntimeError) as host:
            bs.decompress_lz4(bad, (c.size,), np.uint8, c.block)
        assert _code(host) < 0
        with pytest.raises(RuntimeError) as orc:
            oracle.decompress_lz4(bad, (c.size,), np.uint8, c.block)
        pinned = zero_len and _code(orc) == -1001
        if pinned:
            assert _code(host) == -1001
    t = to_dev(torch, bad)
    with pytest.raises(bs.BshufError) as idx:
        bs.api.block_index_dev(t, c.size, c.E, c.block)
    assert _code(idx) < 0
    whole, out = guarded(torch, c.size)
    with pytest.raises(bs.BshufError) as dec:
        bs.decompress_lz4_dev(t, (c.size,), torch.uint8, c.block, out=out, elem_size=1)
    torch.cuda.synchronize()
    assert _code(dec) < 0 and guards_untouched(whole)
    if pinned:
        assert _code(dec) == -1001
    # between two sound streams: they decode exactly, the broken one reports
    ns = [streams(*n) for n in nbrs]
    three = [(ns[0].buf, ns[0].size), (bad, c.size), (ns[1].buf, ns[1].size)]
    outs = [guarded(torch, size) for _, size in three]
    _, res = bs.decompress_lz4_batch_dev([to_dev(torch, b) for b, _ in three], [(size,) for _, size in three],
                                         torch.uint8, c.block, outs=[o for _, o in outs], elem_size=1, sync=False)
    res = res.cpu().tolist()
    assert res[0] == len(ns[0].buf) and res[1] < 0 and res[2] == len(ns[1].buf)
    assert all(guards_untouched(whole) for whole, _ in outs)
    assert outs[0][1].cpu().numpy().tobytes() == ns[0].want
    assert outs[2][1].cpu().numpy().tobytes() == ns[1].want


@pytest.mark.parametrize("fill", [0xFF, 0x00])
def test_broken_first_chunk_in_a_dirty_workspace_spares_the_neighbours(bs, torch, streams, fill):
    """A stream whose first header is broken has no count for chunk 0.  The
    counts are scanned into every later chunk's first block number, so chunk
    0's word must be written all the same: left as the workspace held it
    (all ones), chunk 1's first header went to block -1 of the stream, which
    in a batch is the last block of the stream in front."""
    from bitshuffle_amd.api import _size_array
    c = streams("d2", "a", "e1")
    ns = [streams("d1_8k"), streams("d2", "b", "e1")]
    bad = c.buf.copy()
    bad[:4] = 0
    three = [(ns[0].buf, ns[0].size), (bad, c.size), (ns[1].buf, ns[1].size)]
    pnb, keep1 = _size_array([len(b) for b, _ in three])
    psz, keep2 = _size_array([size for _, size in three])
    need = int(bs.lib.bshuf_decompress_lz4_batch_dev_workspace(pnb, psz, 3, 1, c.block))
    assert need > 0
    ws = torch.full((need + 256,), fill, dtype=torch.uint8, device="cuda")
    outs = [guarded(torch, size) for _, size in three]
    _, res = bs.decompress_lz4_batch_dev([to_dev(torch, b) for b, _ in three], [(size,) for _, size in three],
                                         torch.uint8, c.block, outs=[o for _, o in outs], workspace=ws,
                                         elem_size=1, sync=False)
    res = res.cpu().tolist()
    assert res[0] == len(ns[0].buf) and res[1] < 0 and res[2] == len(ns[1].buf)
    assert all(guards_untouched(whole) for whole, _ in outs)
    assert outs[0][1].cpu().numpy().tobytes() == ns[0].want
    assert outs[2][1].cpu().numpy().tobytes() == ns[1].want
