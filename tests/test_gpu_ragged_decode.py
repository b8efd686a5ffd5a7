"""Ragged window decode (bshuf_decompress_lz4_ragged_dev,
bshuf_decompress_lz4_ragged_set_dev): K windows whose starts and counts live in
device tensors, packed back to back (values + offsets) or one per row of a
pitched output, byte for byte against slices of the original array.

Every call writes into an output filled with 0xA5 that has 64 guard bytes in
front and behind; every byte outside the good windows must come back as it
was.  The offsets are numpy's exclusive scan of the good windows' counts.  No
tolerances: tobytes() equality."""
import copy

import numpy as np
import pytest

from tests import hip_graph as H
from tests.test_gpu_range_decode import Stream, raw_bytes

pytestmark = pytest.mark.gpu

GUARD = 64
FILL = 0xA5


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


def dev(torch, a):
    return torch.tensor(np.asarray(a, dtype=np.int64), dtype=torch.int64, device="cuda")


def scan_of(streams, ids, starts, counts, max_window, E):
    """(good, offsets): which windows are good, numpy's exclusive scan of their counts.
    streams: the original bytes per stream; ids None: all windows in streams[0]."""
    K = len(starts)
    eff = np.zeros(K, dtype=np.int64)
    good = np.zeros(K, dtype=bool)
    for i in range(K):
        sid = 0 if ids is None else ids[i]
        if not 0 <= sid < len(streams):
            continue
        size = len(streams[sid]) // E
        if 0 <= counts[i] <= max_window and 0 <= starts[i] <= size - counts[i]:
            eff[i] = counts[i]
            good[i] = True
    return good, np.concatenate([[0], np.cumsum(eff)]).astype(np.int64)


def plan(streams, ids, starts, counts, max_window, E, pitch, capacity, fail):
    """What a call must leave: (offsets, status, result, body bytes of `capacity` elements)."""
    K = len(starts)
    good, offs = scan_of(streams, ids, starts, counts, max_window, E)
    body = np.full(capacity * E, FILL, dtype=np.uint8)
    status = []
    for i in range(K):
        at = i * pitch if pitch else int(offs[i])
        # (an empty window writes nothing, so it needs no room)
        if not good[i] or (not pitch and counts[i] > 0 and at + counts[i] > capacity):
            status.append(-71)
        elif i in fail:
            status.append(fail[i])
        else:
            status.append(int(counts[i]) * E)
            src = streams[0 if ids is None else ids[i]]
            body[at * E:(at + counts[i]) * E] = src[starts[i] * E:(starts[i] + counts[i]) * E]
    bad = [c for c in status if c < 0]
    result = int(offs[K]) * E if not bad else (-71 if -71 in bad else bad[-1])
    return offs, status, result, body


def run(bs, torch, st, starts, counts, max_window, pitch=0, offsets="own", capacity=None, buf=None, fail=(),
        sset=None, ids=None, streams=None, workspace=None, shift=0):
    """One call, sync=False; checks offsets, statuses, result, every byte of the output and the guards."""
    E = st.E if st is not None else sset.elem_size
    streams = [st.want] if streams is None else streams
    starts, counts = list(starts), list(counts)
    K = len(starts)
    total = int(scan_of(streams, ids, starts, counts, max_window, E)[1][-1])
    if capacity is None:
        capacity = K * pitch if pitch else total
    offs, status, result, body = plan(streams, ids, starts, counts, max_window, E, pitch, capacity, dict(fail))
    whole = torch.full((GUARD + shift + capacity * E + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    out = whole[GUARD + shift:GUARD + shift + capacity * E]
    d_off = torch.full((K + 1,), 777, dtype=torch.int64, device="cuda")
    d_status = torch.full((K,), 12345, dtype=torch.int64, device="cuda")
    d_starts, d_counts = dev(torch, starts), dev(torch, counts)
    if sset is None:
        offp = st.offs if isinstance(offsets, str) else offsets
        r = bs.decompress_lz4_ragged_dev(st.buf if buf is None else buf, st.size, torch.uint8, d_starts,
                                         d_counts, max_window, out=out, out_offsets=d_off, pitch=pitch,
                                         block_size=st.block, status=d_status, offsets=offp, elem_size=E,
                                         workspace=workspace, sync=False)
    else:
        r = bs.decompress_lz4_ragged_set_dev(sset, torch.uint8, dev(torch, ids), d_starts, d_counts, max_window,
                                             out=out, out_offsets=d_off, pitch=pitch, status=d_status,
                                             elem_size=E, workspace=workspace, sync=False)
    torch.cuda.synchronize()
    o, oo, stt, res = r
    assert o is out and oo is d_off and stt is d_status
    assert d_off.cpu().numpy().tolist() == offs.tolist(), "offsets differ from numpy's scan"
    got_status = d_status.cpu().tolist()
    if got_status != status:
        rows = [i for i in range(K) if got_status[i] != status[i]][:8]
        raise AssertionError("status of windows %s: got %s, want %s (starts %s, counts %s)"
                             % (rows, [got_status[i] for i in rows], [status[i] for i in rows],
                                [starts[i] for i in rows], [counts[i] for i in rows]))
    assert int(res.item()) == result
    got = whole.cpu().numpy()
    lo = GUARD + shift
    assert got[:lo].tobytes() == bytes([FILL]) * lo, "bytes in front of the output were written"
    assert got[lo + capacity * E:].tobytes() == bytes([FILL]) * GUARD, "bytes behind the output were written"
    if got[lo:lo + capacity * E].tobytes() != body.tobytes():
        d = np.nonzero(got[lo:lo + capacity * E] != body)[0]
        raise AssertionError("%d bytes differ, the first at byte %d (element %d)" % (d.size, d[0], d[0] // E))
    return status


def special_windows(size, b, mw):
    """(start, count) pairs every main shape must hold."""
    last = size % b - size % 8
    covered = size // b * b + last
    tail = size - covered
    assert tail > 0
    w = [(0, 0), (size, 0), (5, 1), (10, mw), (size - mw, mw),
         (b + 3, 10),                                 # inside one block
         (b - 20, 20), (3 * b - 150, 150),            # end exactly on a block edge
         (2 * b, 1), (2 * b - 1, 2),                  # a block's first element; across an edge
         (covered - 5, 5 + tail), (covered - 1, 2),   # reach into the tail
         (covered, tail), (covered + 1, 1),           # wholly in the tail
         (size - 1, 1),
         (size - 1, 2), (3, -1), (0, mw + 1), (-1, 3), (size + 1, 0), (2 ** 62, 1), (7, -2 ** 62)]  # refused
    return w


def windows_for(size, b, mw, K, seed):
    w = special_windows(size, b, mw)
    rng = np.random.default_rng(seed)
    while len(w) < K:
        c = int(rng.integers(0, mw + 1))
        w.append((int(rng.integers(0, size - c + 1)), c))
    order = rng.permutation(len(w))
    return [w[i][0] for i in order], [w[i][1] for i in order]


MAIN = [(2, 64, 37 * 64 + 40 + 3), (2, 4096, 3 * 4096 + 5), (1, 64, 37 * 64 + 40 + 3), (3, 64, 37 * 64 + 40 + 3)]


@pytest.mark.parametrize("E,block,size", MAIN)
def test_main_shapes_packed_and_padded(bs, torch, make, E, block, size):
    st = make(E, block, size)
    if E == 2 and block == 4096:
        assert block == bs.default_block_size(2)
    mw, K = 200, 257
    starts, counts = windows_for(size, block, mw, K, seed=size + E)
    for offsets in ("own", None):
        run(bs, torch, st, starts, counts, mw, offsets=offsets)
        run(bs, torch, st, starts, counts, mw, pitch=mw, offsets=offsets)
    run(bs, torch, st, starts, counts, mw, pitch=mw + 7, shift=1)
    run(bs, torch, st, starts, counts, mw, shift=3)


def test_good_windows_only_give_the_byte_count(bs, torch, make):
    st = make(2, 64, 37 * 64 + 40 + 3)
    starts, counts = windows_for(st.size, 64, 200, 40, seed=1)
    keep = [i for i in range(len(starts)) if 0 <= counts[i] <= 200 and 0 <= starts[i] <= st.size - counts[i]]
    starts, counts = [starts[i] for i in keep], [counts[i] for i in keep]
    for pitch in (0, 200):
        status = run(bs, torch, st, starts, counts, 200, pitch=pitch)
        assert all(s >= 0 for s in status)
    # the Python call with a real dtype and its own buffers
    out, offs, status = bs.decompress_lz4_ragged_dev(st.buf, st.size, torch.int16, dev(torch, starts),
                                                     dev(torch, counts), 200, block_size=64, offsets=st.offs)
    assert out.dtype == torch.int16 and out.numel() == len(starts) * 200
    o = offs.cpu().tolist()
    assert o == np.concatenate([[0], np.cumsum(counts)]).tolist()
    flat = out.cpu().numpy().view(np.uint8)
    for i, (s, c) in enumerate(zip(starts, counts)):
        assert flat[o[i] * 2:(o[i] + c) * 2].tobytes() == st.want[s * 2:(s + c) * 2].tobytes()
    out, _, _ = bs.decompress_lz4_ragged_dev(st.buf, st.size, torch.int16, dev(torch, starts),
                                             dev(torch, counts), 200, pitch=208, block_size=64)
    assert tuple(out.shape) == (len(starts), 208)


@pytest.mark.parametrize("K", [1, 63, 64, 65, 255, 256, 1025, 70001])
def test_scan_sizes(bs, torch, make, K):
    """Below one tile of the placement scan, at its edges, and over many tiles."""
    st = make(2, 64, 37 * 64 + 40 + 3)
    mw = 9
    rng = np.random.default_rng(K)
    counts = rng.integers(0, mw + 1, K)
    starts = rng.integers(0, st.size - mw + 1, K)
    if K > 3:
        counts[rng.integers(0, K, max(K // 50, 1))] = -1          # refused ones: eff 0
    counts[K - 1] = mw
    run(bs, torch, st, starts.tolist(), counts.tolist(), mw)


def test_capacity(bs, torch, make):
    st = make(2, 64, 37 * 64 + 40 + 3)
    mw = 200
    starts, counts = windows_for(st.size, 64, mw, 60, seed=5)
    starts += [100, 7, 9]
    counts += [33, 0, -1]                                         # the last non-empty window, then an empty one
    total = int(scan_of([st.want], None, starts, counts, mw, 2)[1][-1])
    run(bs, torch, st, starts, counts, mw, capacity=total)
    status = run(bs, torch, st, starts, counts, mw, capacity=total - 1)
    refused = [i for i in range(len(starts)) if status[i] == -71 and 0 <= counts[i] <= mw
               and 0 <= starts[i] <= st.size - counts[i]]
    assert refused == [len(starts) - 3], "exactly the last non-empty window is refused"
    status = run(bs, torch, st, starts, counts, mw, capacity=0)
    assert all(s in (0, -71) for s in status) and 0 in status
    # padded: a capacity below K * pitch is the host's -71
    with pytest.raises(bs.BshufError) as e:
        out = torch.empty(len(starts) * mw - 1, dtype=torch.int16, device="cuda")
        bs.decompress_lz4_ragged_dev(st.buf, st.size, torch.int16, dev(torch, starts), dev(torch, counts), mw,
                                     out=out, pitch=mw, block_size=64)
    assert e.value.args[1] == -71


def test_equal_counts_are_the_window_decode(bs, torch, make):
    st = make(2, 64, 37 * 64 + 40 + 3)
    L, K = 131, 100
    rng = np.random.default_rng(3)
    starts = rng.integers(0, st.size - L + 1, K).tolist() + [0, st.size - L]
    K = len(starts)
    d_starts = dev(torch, starts)
    for offsets in (st.offs, None):
        want = bs.decompress_lz4_windows_dev(st.buf, st.size, torch.int16, d_starts, L, 64, offsets=offsets)
        out, offs, status = bs.decompress_lz4_ragged_dev(st.buf, st.size, torch.int16, d_starts,
                                                         dev(torch, [L] * K), L, block_size=64, offsets=offsets)
        assert out.cpu().numpy().tobytes() == want.cpu().numpy().tobytes()
        assert offs.cpu().tolist() == [i * L for i in range(K + 1)]
        assert status.cpu().tolist() == [L * 2] * K


def test_inert_blocks_isolate(bs, torch, make):
    """Block 2's header is destroyed.  A window fails exactly when it holds
    elements of block 2; a window in a neighbouring block succeeds although the
    Mw blocks its staging area stands for include block 2."""
    b = 128
    size = 5 * b + 24 + 5
    st = make(2, b, size)
    bad = st.buf.clone()
    o2 = int(st.offs[2].item())
    bad[o2:o2 + 4] = torch.tensor([0x7F, 0xFF, 0xFF, 0xFF], dtype=torch.uint8, device="cuda")
    with pytest.raises(bs.BshufError) as whole:
        bs.decompress_lz4_dev(bad, (size,), torch.int16, b, offsets=st.offs)
    code = whole.value.args[1]
    assert code < 0
    mw = 200
    assert (mw + b - 2) // b + 1 == 3                      # Mw: a window in block 1 stands for blocks 1, 2, 3
    wins = [(10, 26, False), (2 * b + 1, 26, True), (2 * b - 10, 26, True), (3 * b + 5, 26, False),
            (5 * b + 3, 26, False), (b + 100, 1, False), (b + 100, 28, False), (2 * b - 1, 1, False),
            (2 * b - 1, 2, True), (3 * b, 1, False), (3 * b - 1, 1, True), (b, mw, True), (0, b, False),
            (3 * b, mw, False), (b + 7, 0, False)]
    starts, counts = [w[0] for w in wins], [w[1] for w in wins]
    fail = {i: code for i, w in enumerate(wins) if w[2]}
    for pitch in (0, mw):
        run(bs, torch, st, starts, counts, mw, pitch=pitch, buf=bad, fail=fail)
    ok = [w for w in wins if not w[2]]
    run(bs, torch, st, [w[0] for w in ok], [w[1] for w in ok], mw, buf=bad)


SET_SIZES = [37 * 64 + 40 + 3, 5, 64 + 24, 10 * 64, 3 * 64 + 40 + 5]


@pytest.fixture(scope="module")
def sets(bs, torch, make):
    streams = [make(2, 64, n) for n in SET_SIZES]
    out = {}
    for supplied in (True, False):
        offs = [st.offs for st in streams] if supplied else None
        out[supplied] = bs.lz4_stream_set_dev([st.buf for st in streams], SET_SIZES, 2, 64, offsets=offs)
    return streams, out


def test_set_of_unequal_streams(bs, torch, sets):
    """Five streams; stream 2 has fewer blocks than Mw, stream 1 is all tail."""
    streams, ssets = sets
    mw, b = 200, 64
    Mw = min((mw + b - 2) // b + 1, max(st.nb for st in streams))
    assert streams[2].nb < Mw and streams[1].nb == 0
    wants = [st.want for st in streams]
    rng = np.random.default_rng(11)
    ids, starts, counts = [], [], []
    for sid, st in enumerate(streams):                             # per stream: the edges
        top = min(mw, st.size)
        for s, c in ((0, top), (st.size - top, top), (st.size - 1, 1), (st.size, 0), (st.size - 1, 2), (0, 0)):
            ids.append(sid), starts.append(s), counts.append(c)
    ids += [2, 2, 2, 1, 1]                                         # the short stream, the all-tail one
    starts += [3, 60, 64, 0, 2]
    counts += [70, 10, 24, 5, 3]
    for _ in range(120):
        sid = int(rng.integers(-1, len(streams) + 1))              # -1 and 5: out of range
        size = streams[sid].size if 0 <= sid < len(streams) else 100
        c = int(rng.integers(0, min(mw, size) + 1))
        ids.append(sid), starts.append(int(rng.integers(0, size - c + 1))), counts.append(c)
    order = rng.permutation(len(ids))
    ids, starts, counts = ([a[i] for i in order] for a in (ids, starts, counts))
    for supplied in (True, False):
        for pitch in (0, mw):
            status = run(bs, torch, None, starts, counts, mw, pitch=pitch, sset=ssets[supplied], ids=ids,
                         streams=wants)
    k = [i for i in range(len(ids)) if (ids[i], starts[i], counts[i]) == (2, 3, 70)][0]
    assert status[k] == 140, "a window of the short stream decodes"
    # the same shape through the fixed-length call: the short stream takes no window of 70
    assert (70 + b - 2) // b + 1 > streams[2].nb
    d_status = torch.zeros(1, dtype=torch.int64, device="cuda")
    _, res = bs.decompress_lz4_windows_set_dev(ssets[True], torch.int16, dev(torch, [2]), dev(torch, [3]), 70,
                                               status=d_status, sync=False)
    torch.cuda.synchronize()
    assert d_status.cpu().tolist() == [-71] and int(res.item()) == -71
    run(bs, torch, None, [3], [70], 70, sset=ssets[True], ids=[2], streams=wants)


def test_set_that_does_not_match_the_call(bs, torch, sets):
    """The call names another nb_max than the set's header: every window is refused."""
    streams, ssets = sets
    other = copy.copy(ssets[True])
    other.max_size = ssets[True].max_size + 64
    ids, starts, counts = [0, 3, 2, 1], [5, 0, 3, 0], [100, 7, 70, 5]
    K = len(ids)
    out = torch.full((K * 200 * 2,), FILL, dtype=torch.uint8, device="cuda")
    o, offs, status, res = bs.decompress_lz4_ragged_set_dev(other, torch.uint8, dev(torch, ids), dev(torch, starts),
                                                            dev(torch, counts), 200, out=out, elem_size=2,
                                                            sync=False)
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [-71] * K and int(res.item()) == -71
    assert offs.cpu().tolist() == [0] * (K + 1)
    assert bool((out == FILL).all())


def test_capture_and_replay(bs, torch, make):
    """One captured call with a caller workspace: a linear chain without
    allocations, replayed with other starts AND counts in the same tensors over
    a workspace refilled with 0x00, 0xFF and random bytes."""
    b = 64
    st = make(2, b, 37 * 64 + 40 + 3)
    mw, K = 200, 96
    contents = [windows_for(st.size, b, mw, K, seed=100 + k) for k in range(4)]
    starts, counts = dev(torch, contents[0][0]), dev(torch, contents[0][1])
    cap_elems = K * mw
    whole = torch.full((GUARD + cap_elems * 2 + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    out = whole[GUARD:GUARD + cap_elems * 2]
    offs = torch.zeros(K + 1, dtype=torch.int64, device="cuda")
    status = torch.zeros(K, dtype=torch.int64, device="cuda")
    result = torch.zeros(1, dtype=torch.int64, device="cuda")
    ws = bs.decompress_lz4_ragged_workspace(st.buf.numel(), st.size, 2, K, mw, b)
    gen = torch.Generator(device="cuda").manual_seed(9)
    news = [(dev(torch, s), dev(torch, c)) for s, c in contents]
    torch.cuda.synchronize()
    gs = H.GraphStream()

    def call():
        bs.decompress_lz4_ragged_dev(st.buf, st.size, torch.uint8, starts, counts, mw, out=out, out_offsets=offs,
                                     block_size=b, workspace=ws, result=result, status=status, offsets=st.offs,
                                     stream=gs.handle.value, elem_size=2, sync=False)
        return 0

    def load(k, fill):
        with torch.cuda.stream(gs.torch_stream):
            starts.copy_(news[k][0])
            counts.copy_(news[k][1])
            whole.fill_(FILL)
            offs.fill_(-5), status.fill_(-5), result.fill_(-5)
            if fill == "random":
                ws.copy_(torch.randint(0, 256, (ws.numel(),), dtype=torch.uint8, device="cuda", generator=gen))
            else:
                ws.fill_(fill)

    def check(k):
        s, c = contents[k]
        w_offs, w_status, w_result, body = plan([st.want], None, s, c, mw, 2, 0, cap_elems, {})
        assert offs.cpu().tolist() == w_offs.tolist()
        assert status.cpu().tolist() == w_status and int(result.item()) == w_result
        got = whole.cpu().numpy()
        assert got[GUARD:-GUARD].tobytes() == body.tobytes()
        assert got[:GUARD].tobytes() == got[-GUARD:].tobytes() == bytes([FILL]) * GUARD

    g = None
    try:
        torch.cuda.synchronize()
        load(0, 0xFF)
        call()
        gs.synchronize()
        check(0)
        g = gs.capture(call)
        assert H.MEM_ALLOC not in g.types and H.MEM_FREE not in g.types, g.names()
        assert set(g.types) <= {H.KERNEL, H.MEMCPY, H.MEMSET}, g.names()
        assert g.is_linear_chain(), (g.nodes, g.edges)
        g.instantiate()
        for k, fill in zip((1, 2, 3), (0x00, 0xFF, "random")):
            load(k, fill)
            g.launch()
            gs.synchronize()
            check(k)
    finally:
        gs.synchronize()
        if g is not None:
            g.destroy()
        gs.close()


def test_dirty_workspace_and_workspace_contract(bs, torch, make, sets):
    b = 64
    st = make(2, b, 37 * 64 + 40 + 3)
    mw, K = 200, 64
    starts, counts = windows_for(st.size, b, mw, K, seed=21)
    n = int(bs.lib.bshuf_decompress_lz4_ragged_dev_workspace(st.buf.numel(), st.size, 2, b, K, mw))
    ws = bs.decompress_lz4_ragged_workspace(st.buf.numel(), st.size, 2, K, mw, b)
    assert ws.numel() == n and ws.data_ptr() % 256 == 0
    for fill in (0x00, 0xFF):
        for offsets in ("own", None):
            for pitch in (0, mw):
                ws.fill_(fill)
                run(bs, torch, st, starts, counts, mw, pitch=pitch, offsets=offsets, workspace=ws)
    # no workspace: the library's pool, outside capture (every other test)
    d_s, d_c = dev(torch, starts), dev(torch, counts)
    with pytest.raises(bs.BshufError) as e:
        bs.decompress_lz4_ragged_dev(st.buf, st.size, torch.int16, d_s, d_c, mw, block_size=b,
                                     workspace=ws[:n - 1], sync=False)
    assert e.value.args[1] == -71
    # over a set
    streams, ssets = sets
    wsn = int(bs.lib.bshuf_decompress_lz4_ragged_set_dev_workspace(max(SET_SIZES), 2, 64, 3, mw))
    sws = bs.decompress_lz4_ragged_set_workspace(ssets[True], 3, mw)
    assert sws.numel() == wsn
    sws.fill_(0xFF)
    run(bs, torch, None, [3, 0, 100], [70, 5, 200], mw, sset=ssets[True], ids=[2, 1, 0],
        streams=[s.want for s in streams], workspace=sws)
    with pytest.raises(bs.BshufError) as e:
        bs.decompress_lz4_ragged_set_dev(ssets[True], torch.int16, dev(torch, [2, 1, 0]), dev(torch, [3, 0, 100]),
                                         dev(torch, [70, 5, 200]), mw, workspace=sws[:wsn - 1], sync=False)
    assert e.value.args[1] == -71


def test_host_refusals_and_empty_calls(bs, torch, make):
    b = 64
    st = make(2, b, 37 * 64 + 40 + 3)
    d_s, d_c = dev(torch, [0, 5]), dev(torch, [3, 4])
    for kw in (dict(max_window=st.size + 1), dict(max_window=10, pitch=9)):
        with pytest.raises(bs.BshufError) as e:
            bs.decompress_lz4_ragged_dev(st.buf, st.size, torch.int16, d_s, d_c, block_size=b, **kw)
        assert e.value.args[1] == -71
    # packed needs the offsets: NULL is the host's -71
    z = torch.zeros(4, dtype=torch.int64, device="cuda")
    rc = bs.lib.bshuf_decompress_lz4_ragged_dev(st.buf.data_ptr(), st.buf.numel(), st.size, 2, b, d_s.data_ptr(),
                                                d_c.data_ptr(), 2, 10, z.data_ptr(), 4, 0, None, None, 0,
                                                z.data_ptr(), None, None, None)
    assert rc == -71
    # nothing to decode: result 0, offsets 0
    for K, mw in ((0, 5), (2, 0)):
        offs = torch.full((K + 1,), 9, dtype=torch.int64, device="cuda")
        out, o, status, res = bs.decompress_lz4_ragged_dev(st.buf, st.size, torch.int16, d_s[:K], d_c[:K], mw,
                                                           out_offsets=offs, block_size=b, sync=False)
        torch.cuda.synchronize()
        assert int(res.item()) == 0 and offs.cpu().tolist() == [0] * (K + 1)
    for wrong in (d_c.cpu(), d_c.to(torch.int32), d_c[:1]):
        with pytest.raises(ValueError):
            bs.decompress_lz4_ragged_dev(st.buf, st.size, torch.int16, d_s, wrong, 10, block_size=b)
