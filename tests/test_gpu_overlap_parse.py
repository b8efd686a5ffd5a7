"""The pipelined encode with its parse launches on two streams (csrc/launch.h,
encode_pipelined): which stream parses a segment, and how the segments are cut,
must not show in any output.  Every case compares compressed bytes with the
oracle's (or, at 512 MiB, with the unsegmented launch's) and decodes them back,
under the default schedule, with every parse on the caller's stream
(bshuf_set_variant bit 1 << 27), with the other segment schedule (1 << 28), with
the side stream's compaction by the 256-thread kernel (1 << 29) and unsegmented
(1 << 20).

int16 with block_size = 64 elements (128-byte blocks): 65,536 blocks, where the
pipelined path starts, are 8 MiB.
"""
import ctypes

import numpy as np
import pytest

from tests import fast_model

pytestmark = pytest.mark.gpu

BLOCK = 64              # elements per block
NO_PIPE = 1 << 20       # bshuf_set_variant bit: unsegmented encode
NO_OVERLAP = 1 << 27    # every parse launch on the caller's stream
ALT_SEGMENTS = 1 << 28  # the segment schedule that is not the default
WIDE_COMPACT = 1 << 29  # side-stream compaction by the 256-thread k_compact
VARIANTS = [0, NO_OVERLAP, NO_PIPE, ALT_SEGMENTS, ALT_SEGMENTS | NO_OVERLAP, WIDE_COMPACT]
VARIANT_IDS = ["default", "no-overlap", "no-pipe", "alt-segments", "alt-segments-no-overlap",
               "wide-compact"]
# (elements, blocks): 65,536 and 65,541 full blocks; 65,540 full blocks + a
# partial one of 40 elements + 5 raw tail elements
SIZES = {"65536": (65536 * BLOCK, 65536), "65541": (65541 * BLOCK, 65541),
         "partial+tail": (65540 * BLOCK + 40 + 5, 65541)}


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
    """set(v) selects a variant; the default is restored after the test."""
    def set_(v):
        assert bs.lib.bshuf_set_variant(v) == 0, v
    yield set_
    assert bs.lib.bshuf_set_variant(0) == 0


@pytest.fixture(scope="module")
def data(oracle):
    """G1-like int16 with all-zero and random 128-byte blocks mixed in, so that
    block times and record lengths differ.  Read-only."""
    n = 65541 * BLOCK + 64
    a = oracle.gen_g1(n).copy()
    rng = np.random.default_rng(77)
    nb = n // BLOCK
    blocks = a[: nb * BLOCK].reshape(nb, BLOCK)
    kind = rng.integers(0, 16, nb)
    kind[8150:8250] = 0      # runs across the first segment bound (block 8,192)
    kind[57300:57400] = 1    # ... and across the last one of eight equal segments
    blocks[kind == 0] = 0
    blocks[kind == 1] = rng.integers(-32768, 32768, (int((kind == 1).sum()), BLOCK)).astype(np.int16)
    a.setflags(write=False)
    return a


@pytest.fixture(scope="module")
def streams(oracle, data):
    """size name -> (input, the oracle's compressed stream), computed once."""
    cache = {}

    def get(name):
        if name not in cache:
            n, nb = SIZES[name]
            a = data[:n]
            cache[name] = (a, oracle.compress_lz4(a, BLOCK), nb)
        return cache[name]
    return get


@pytest.fixture(scope="module")
def second(oracle, data):
    """A second input of 65,541 full blocks (the first one's halves swapped)."""
    n = SIZES["65541"][0]
    b = data[:n].copy()
    b[: n // 2], b[n - n // 2:] = data[n - n // 2: n], data[: n // 2]
    return b, oracle.compress_lz4(b, BLOCK)


# 1. every schedule gives the oracle's bytes, and they decode back
@pytest.mark.parametrize("size", list(SIZES))
def test_streams_identical_across_schedules(bs, torch, streams, variant, size):
    a, want, nb = streams(size)
    assert int(bs.lib.bshuf_lz4_dev_nblocks(a.size, 2, BLOCK)) == nb
    x = torch.from_numpy(a.copy()).cuda()
    for v, name in zip(VARIANTS, VARIANT_IDS):
        variant(v)
        c = bs.compress_lz4_dev(x, BLOCK)
        assert c.cpu().numpy().tobytes() == want.tobytes(), name
        y = bs.decompress_lz4_dev(c, x.shape, x.dtype, BLOCK)
        assert torch.equal(x, y), name


# 2. two calls back to back on one stream, one dirty workspace, no host
# synchronisation between them: the second call's fill and parses must be
# ordered behind everything of the first on all three streams
@pytest.mark.parametrize("v", [0, ALT_SEGMENTS], ids=["default", "alt-segments"])
def test_back_to_back_calls_share_a_dirty_workspace(bs, torch, streams, second, variant, v):
    a, want_a, _ = streams("65541")
    b, want_b = second
    variant(v)
    xs = [torch.from_numpy(t.copy()).cuda() for t in (a, b)]
    cap = bs.compress_lz4_bound(a.size, 2, BLOCK)
    ws = bs.api.compress_lz4_workspace(a.size, 2, BLOCK)
    ws.fill_(0xFF)
    bufs = [torch.zeros(cap, dtype=torch.uint8, device="cuda") for _ in xs]
    torch.cuda.synchronize()
    res = [bs.compress_lz4_dev(x, BLOCK, out=o, workspace=ws, sync=False)[1] for x, o in zip(xs, bufs)]
    torch.cuda.synchronize()
    for o, r, w in zip(bufs, res, (want_a, want_b)):
        assert int(r.item()) == w.size
        assert o[: w.size].cpu().numpy().tobytes() == w.tobytes()


# 3. a call on a non-default stream, then one on the default stream from the
# same thread: both use the thread's par and side streams
def test_two_caller_streams_share_par_and_side(bs, torch, streams, second, variant):
    a, want_a, _ = streams("65541")
    b, want_b = second
    variant(0)
    xa, xb = (torch.from_numpy(t.copy()).cuda() for t in (a, b))
    torch.cuda.synchronize()
    s1 = torch.cuda.Stream()
    with torch.cuda.stream(s1):
        oa, ra = bs.compress_lz4_dev(xa, BLOCK, sync=False)
    ob, rb = bs.compress_lz4_dev(xb, BLOCK, sync=False)
    torch.cuda.synchronize()
    for o, r, w in ((oa, ra, want_a), (ob, rb, want_b)):
        assert int(r.item()) == w.size
        assert o[: w.size].cpu().numpy().tobytes() == w.tobytes()


# 4. sync=False: the device-held length goes straight into the decoder
def test_device_held_length_into_decode(bs, torch, streams, variant):
    a, want, _ = streams("partial+tail")
    variant(0)
    x = torch.from_numpy(a.copy()).cuda()
    buf = torch.zeros(bs.compress_lz4_bound(a.size, 2, BLOCK), dtype=torch.uint8, device="cuda")
    _, res = bs.compress_lz4_dev(x, BLOCK, out=buf, sync=False)
    y, r = bs.decompress_lz4_dev(buf, x.shape, x.dtype, BLOCK, sync=False, length=res)
    assert int(res.item()) == want.size == int(r.item())
    assert buf[: want.size].cpu().numpy().tobytes() == want.tobytes()
    assert torch.equal(x, y)


# 5. batch: 65,544 blocks in three chunks of full blocks.  Eight equal segments
# (and the first seven of the tapered schedule) are 8,193 blocks each: the first
# chunk ends on the bound 16,386, the second at 26,386 inside segment 3.
@pytest.mark.parametrize("v", [0, NO_OVERLAP, ALT_SEGMENTS, WIDE_COMPACT],
                         ids=["default", "no-overlap", "alt-segments", "wide-compact"])
def test_batch_chunk_bounds_on_and_inside_segments(bs, torch, oracle, data, variant, v):
    chunks = (16386, 10000, 39158)
    assert sum(chunks) == 65544 and 65544 // 8 * 2 == chunks[0]
    arrs, pos = [], 0
    for nb in chunks:
        arrs.append(data[pos: pos + nb * BLOCK])
        pos = (pos + nb * BLOCK) % (20000 * BLOCK)  # overlapping windows of the 65,541-block input
    variant(v)
    xs = [torch.from_numpy(t.copy()).cuda() for t in arrs]
    outs, res = bs.compress_lz4_batch_dev(xs, BLOCK, sync=False)
    dec, dres = bs.decompress_lz4_batch_dev(outs, [t.shape for t in arrs], torch.int16, BLOCK,
                                            sync=False, lengths=res)
    want = [oracle.compress_lz4(t, BLOCK) for t in arrs]
    assert res.cpu().tolist() == [w.size for w in want] == dres.cpu().tolist()
    for t, o, w, d in zip(arrs, outs, want, dec):
        assert o[: w.size].cpu().numpy().tobytes() == w.tobytes()
        assert d.cpu().numpy().tobytes() == t.tobytes()


# 6. mode="fast" at the same size: 65,541 blocks made of 37 distinct ones, so
# that the numpy model can cache payloads
@pytest.mark.parametrize("v", [0, NO_OVERLAP, NO_PIPE], ids=["default", "no-overlap", "no-pipe"])
def test_fast_mode_equals_its_model(bs, torch, oracle, data, variant, v):
    base = data[100 * BLOCK: 137 * BLOCK]
    arr = np.resize(base, 65541 * BLOCK)
    want = fast_model.compress_lz4(oracle, arr, BLOCK, cache={})
    variant(v)
    x = torch.from_numpy(arr).cuda()
    got = bs.compress_lz4_dev(x, BLOCK, mode="fast")
    assert got.cpu().numpy().tobytes() == want.tobytes()
    assert torch.equal(bs.decompress_lz4_dev(got, x.shape, x.dtype, BLOCK), x)


def prof_collect(bs):
    buf = ctypes.create_string_buffer(1 << 16)
    bs.lib.bshuf_prof_collect(buf, len(buf))
    return {ln.split()[0]: int(ln.split()[1]) for ln in buf.value.decode().splitlines() if ln.strip()}


# 7. per-kernel timing on: the serial schedule runs, same bytes, and every
# segment's parse, scan and compaction is listed
def test_profiling_keeps_bytes_and_names(bs, torch, streams, variant):
    a, want, _ = streams("65541")
    variant(0)
    x = torch.from_numpy(a.copy()).cuda()
    try:
        bs.lib.bshuf_prof_enable(1)
        prof_collect(bs)  # reset
        c = bs.compress_lz4_dev(x, BLOCK)
        torch.cuda.synchronize()
        names = prof_collect(bs)
    finally:
        bs.lib.bshuf_prof_enable(0)
    assert c.cpu().numpy().tobytes() == want.tobytes()
    segs = names.get("k_lz4_encode", 0)
    assert segs in (8, 10), names  # the two schedules of pipe_segments.h
    assert names.get("k_compact_side") == segs and names.get("scan_block_offsets_side") == segs, names
    assert "k_compact" not in names and "scan_block_offsets" not in names, names
    # ... and the next plain call is back on two streams with the same bytes
    assert bs.compress_lz4_dev(x, BLOCK).cpu().numpy().tobytes() == want.tobytes()


# 8. default 8 KiB blocks, 65,536 + 3 of them (512 MiB): the oracle would take
# too long, so the segmented streams are compared with the unsegmented one
def test_default_blocks_512_mib(bs, torch, variant):
    n = (65536 + 3) * int(bs.default_block_size(2))
    x = torch.empty(n, dtype=torch.int16, device="cuda")
    bs.synth_fill_dev(x, 1)
    variant(NO_PIPE)
    ref = bs.compress_lz4_dev(x).clone()
    for v in (0, ALT_SEGMENTS, NO_OVERLAP, WIDE_COMPACT):
        variant(v)
        c = bs.compress_lz4_dev(x)
        assert c.numel() == ref.numel() and torch.equal(c, ref), v
    y = bs.decompress_lz4_dev(c, x.shape, x.dtype)
    assert torch.equal(x, y)


# 9. the segment-local offset scan itself (bshuf_seg_scan_dev), against
# numpy.cumsum: u64 values near 2^33, a non-zero seed, lengths around the wave
# (64), the 256-element step and the 1,024-element tile, and 65 tiles
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1023, 1025, 65537])
@pytest.mark.parametrize("seeded", [1, 0], ids=["seeded", "first-segment"])
def test_segment_scan_against_cumsum(bs, torch, n, seeded):
    fn = bs.lib.bshuf_seg_scan_dev
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int64,
                   ctypes.c_int64, ctypes.c_int, ctypes.c_void_p]
    f0 = 5
    rng = np.random.default_rng(n)
    foot = ((1 << 33) - rng.integers(0, 1 << 20, f0 + n + 1)).astype(np.uint64)
    seed = np.uint64((1 << 40) + 12345)
    offs0 = np.full(f0 + n + 2, 0xDEADBEEFDEADBEEF, dtype=np.uint64)
    offs0[f0] = seed
    want = offs0.copy()
    start = seed if seeded else np.uint64(0)
    want[f0: f0 + n + 1] = start + np.concatenate(([0], np.cumsum(foot[f0: f0 + n], dtype=np.uint64)))
    d_foot = torch.from_numpy(foot.view(np.int64)).cuda()
    d_offs = torch.from_numpy(offs0.view(np.int64)).cuda()
    tmp = torch.full((8192,), 0xFF, dtype=torch.uint8, device="cuda")
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert fn(d_foot.data_ptr(), d_offs.data_ptr(), tmp.data_ptr(), tmp.numel(), f0, f0 + n, seeded, st) == 0
    got = d_offs.cpu().numpy().view(np.uint64)
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:8]
    # too little temp storage is refused, not overrun
    assert fn(d_foot.data_ptr(), d_offs.data_ptr(), tmp.data_ptr(), 8191, f0, f0 + n, seeded, st) != 0
