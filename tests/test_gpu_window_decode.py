"""Window decode (bshuf_decompress_lz4_windows_dev): K windows of one length
whose starts live in a device tensor, byte for byte against slices of the CPU
oracle's decode of the oracle's stream.

Every call writes into an output filled with 0xA5 that has 64 guard bytes in
front and behind, which must come back untouched -- as must the slice of a
window whose start is out of range.  Every case runs with the block index
supplied and with the index rebuilt by the call.  No tolerances: tobytes()
equality."""
import numpy as np
import pytest

from tests.test_gpu_range_decode import Stream, raw_bytes

pytestmark = pytest.mark.gpu

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


def expected(st, starts, window, status=None):
    """(K, window * E) bytes: the oracle's slices; 0xA5 where the window is not written."""
    wb = window * st.E
    exp = np.full((len(starts), wb), 0xA5, dtype=np.uint8)
    for i, s in enumerate(starts):
        ok = 0 <= s <= st.size - window and (status is None or status[i] == wb)
        if ok:
            exp[i] = st.want[s * st.E:(s + window) * st.E]
    return exp


def run(st, starts, window, offsets="own", shift=0, buf=None, want_status=None, want_result=None):
    """One call, sync=False; checks the output, the guards, the statuses and the result."""
    torch, E = st.torch, st.E
    if not isinstance(starts, torch.Tensor):
        starts = torch.tensor(list(starts), dtype=torch.int64, device="cuda")
    K, wb = starts.numel(), window * E
    whole = torch.full((GUARD + shift + K * wb + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    out = whole[GUARD + shift:GUARD + shift + K * wb]
    status = torch.full((K,), 12345, dtype=torch.int64, device="cuda")
    offs = st.offs if isinstance(offsets, str) else offsets
    o, res = st.bs.decompress_lz4_windows_dev(st.buf if buf is None else buf, st.size, torch.uint8, starts,
                                              window, st.block, out=out, status=status, offsets=offs,
                                              elem_size=E, sync=False)
    torch.cuda.synchronize()
    assert o is out
    host_starts = starts.cpu().tolist()
    if want_status is None:
        want_status = [wb if 0 <= s <= st.size - window else -71 for s in host_starts]
    assert status.cpu().tolist() == want_status
    if want_result is None:
        bad = [c for c in want_status if c < 0]
        want_result = K * wb if not bad else (-71 if -71 in bad else bad[-1])
    assert int(res.item()) == want_result
    got = whole.cpu().numpy()
    lo = GUARD + shift
    assert got[:lo].tobytes() == b"\xa5" * lo, "bytes in front of the windows were written"
    assert got[lo + K * wb:].tobytes() == b"\xa5" * GUARD, "bytes behind the windows were written"
    exp = expected(st, host_starts, window, want_status)
    body = got[lo:lo + K * wb].reshape(K, wb)
    if body.tobytes() != exp.tobytes():
        rows = np.nonzero((body != exp).any(axis=1))[0]
        raise AssertionError("windows %s (starts %s) of %d differ, window %d E %d"
                             % (rows[:8].tolist(), [host_starts[i] for i in rows[:8]], K, window, E))
    return status


def both(st, starts, window, **kw):
    run(st, starts, window, **kw)
    run(st, starts, window, offsets=None, **kw)


@pytest.mark.parametrize("E", [1, 2, 4, 8, 3, 12])
def test_every_start_of_a_small_stream(make, E):
    """Three full blocks of 64, a partial block of 40 and a 5-element tail:
    every valid start of every window length in one call, shuffled."""
    b = 64
    size = 3 * b + 40 + 5
    st = make(E, b, size, gen=1 if E != 4 else 2)
    assert st.nb == 4
    for window in (1, 2, 8, 63, 64, 65, 66, 131, size):
        starts = np.arange(size - window + 1)
        np.random.default_rng(window).shuffle(starts)
        both(st, starts.tolist(), window)


@pytest.mark.parametrize("window", [100, 4098])
def test_default_blocks_device_made_starts(bs, torch, make, window):
    b = 4096
    size = 5 * b + 1000 + 3
    st = make(2, b, size)
    g = torch.Generator(device="cuda").manual_seed(7 + window)
    starts = torch.randint(0, size - window + 1, (257,), generator=g, device="cuda", dtype=torch.int64)
    for shift in (0, 1, 3):
        both(st, starts, window, shift=shift)
    # a real dtype: (K, window) of it
    for offsets in (st.offs, None):
        y = bs.decompress_lz4_windows_dev(st.buf, size, torch.int16, starts, window, b, offsets=offsets)
        assert y.dtype == torch.int16 and tuple(y.shape) == (257, window)
        exp = expected(st, starts.cpu().tolist(), window)
        assert y.cpu().numpy().tobytes() == exp.tobytes()


@pytest.mark.parametrize("size", [5, 64, 128])
def test_streams_without_blocks_or_without_a_tail(make, size):
    st = make(2, 64, size)
    assert st.nb == size // 64
    for window in sorted({1, 3, size // 2 + 1, size}):
        both(st, list(range(size - window + 1))[::-1], window)


def test_few_windows_of_a_long_stream(make):
    """Few windows against the stream's length: every window has a token-position
    area of its own (the other cases' windows cover so much of their short
    streams that they share the whole decode's area)."""
    b = 128
    size = 64 * b + 24 + 5
    st = make(2, b, size)
    maxlen = 2 * b + 2 * b // 255 + 16                     # LZ4_compressBound of one block
    for window, starts in ((26, [70 * b // 2 + 3]),
                           (26, [size - 26, b - 3, 40 * b + 100]),
                           (200, [5 * b + 120, 5 * b + 121, 63 * b, 0])):
        Mw = (window + b - 2) // b + 1
        private = len(starts) * (Mw * (4 + maxlen) // 3 + 80)
        assert private < st.buf.numel() // 3 + 80, "these windows would share the whole decode's area"
        both(st, starts, window)


def test_out_of_range_starts(bs, torch, make):
    b = 64
    size = 3 * b + 40 + 5
    st = make(2, b, size)
    for window in (1, 70, size):
        starts = [-1, 0, size - window, size - window + 1, 2 ** 62]
        wb = window * 2
        for offsets in ("own", None):
            run(st, starts, window, offsets=offsets, want_status=[-71, wb, wb, -71, -71], want_result=-71)
        with pytest.raises(bs.BshufError) as e:
            bs.decompress_lz4_windows_dev(st.buf, size, torch.int16,
                                          torch.tensor(starts, dtype=torch.int64, device="cuda"), window, b,
                                          offsets=st.offs)
        assert e.value.args[1] == -71


def test_corrupt_block_with_offsets(bs, torch, make):
    """Block 2's header is destroyed.  With the index supplied, a window fails
    exactly when it holds elements of block 2 -- also when the blocks decoded
    for it include block 2 and its elements do not."""
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
    window = 26
    wb = window * 2
    #          blk 0  blk 2   1+2       blk 3     4+5+tail   blk 1 (2 decoded beside it)  2+3
    starts = [10, 2 * b + 1, 2 * b - 10, 3 * b + 5, 5 * b + 3, b + 100, 3 * b - 5]
    touches = [False, True, True, False, False, False, True]
    want = [code if t else wb for t in touches]
    run(st, starts, window, buf=bad, want_status=want, want_result=code)
    # no failing window: the byte count
    ok = [s for s, t in zip(starts, touches) if not t]
    run(st, ok, window, buf=bad)
    # a failing window that is not the last one
    run(st, [2 * b + 1, 10], window, buf=bad, want_status=[code, wb], want_result=code)
    with pytest.raises(bs.BshufError) as e:
        bs.decompress_lz4_windows_dev(bad, size, torch.int16,
                                      torch.tensor(starts, dtype=torch.int64, device="cuda"), window, b,
                                      offsets=st.offs)
    assert e.value.args[1] == code


def test_caller_workspace_and_host_errors(bs, torch, make):
    b = 128
    size = 5 * b + 24 + 5
    st = make(2, b, size)
    starts = torch.tensor([3, 4 * b + 7, 5 * b], dtype=torch.int64, device="cuda")
    ws = bs.decompress_lz4_windows_workspace(st.buf.numel(), size, 2, 3, 29, b)
    n = int(bs.lib.bshuf_decompress_lz4_windows_dev_workspace(st.buf.numel(), size, 2, b, 3, 29))
    assert ws.numel() == n and ws.data_ptr() % 256 == 0
    for offsets in (st.offs, None):
        y = bs.decompress_lz4_windows_dev(st.buf, size, torch.int16, starts, 29, b, workspace=ws,
                                          offsets=offsets)
        assert y.cpu().numpy().tobytes() == expected(st, starts.tolist(), 29).tobytes()
        with pytest.raises(bs.BshufError) as e:
            bs.decompress_lz4_windows_dev(st.buf, size, torch.int16, starts, 29, b, workspace=ws[:n - 1],
                                          offsets=offsets)
        assert e.value.args[1] == -71
    with pytest.raises(bs.BshufError) as e:
        bs.decompress_lz4_windows_dev(st.buf, size, torch.int16, starts, size + 1, b)
    assert e.value.args[1] == -71
    # nothing to decode: result 0
    for K, window in ((0, 5), (3, 0)):
        out, res = bs.decompress_lz4_windows_dev(st.buf, size, torch.int16, starts[:K], window, b, sync=False)
        torch.cuda.synchronize()
        assert int(res.item()) == 0 and tuple(out.shape) == (K, window)
    for wrong in (starts.cpu(), starts.to(torch.int32), torch.stack([starts, starts], 1)[:, 0],
                  starts.tolist()):
        with pytest.raises(ValueError):
            bs.decompress_lz4_windows_dev(st.buf, size, torch.int16, wrong, 29, b)


def test_starts_never_reach_the_host(bs, torch, make, monkeypatch):
    b = 4096
    size = 5 * b + 1000 + 3
    st = make(2, b, size)
    starts = torch.tensor([0, b - 1, 5 * b + 900, 17], dtype=torch.int64, device="cuda")
    window = 100
    out = torch.full((4, window), 0x5A5A, dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    seen = []

    def spy(name):
        orig = getattr(torch.Tensor, name)

        def f(self, *a, **kw):
            seen.append((name, self))
            return orig(self, *a, **kw)
        monkeypatch.setattr(torch.Tensor, name, f)
    for name in ("cpu", "item", "tolist"):
        spy(name)
    for offsets in (st.offs, None):
        o, res = bs.decompress_lz4_windows_dev(st.buf, size, torch.int16, starts, window, b, out=out,
                                               offsets=offsets, sync=False)
    calls = list(seen)
    monkeypatch.undo()
    assert not any(t is starts or (t.is_cuda and t.data_ptr() == starts.data_ptr()) for _, t in calls), calls
    assert not calls, "a sync=False call read a tensor on the host: %s" % [n for n, _ in calls]
    torch.cuda.synchronize()
    assert int(res.item()) == 4 * window * 2
    assert out.cpu().numpy().tobytes() == expected(st, starts.tolist(), window).tobytes()


def test_capture_and_replay(bs, torch, make):
    """One captured call, replayed with other starts in the same tensor."""
    b = 4096
    size = 5 * b + 1000 + 3
    st = make(2, b, size)
    K, window = 64, 4098
    wb = window * 2
    covered = 5 * b + 1000
    sets = [
        [(i % 4) * b for i in range(K)],                                   # block-aligned
        [b - 1 + (i % 3) * b for i in range(K)],                           # straddling from bs - 1 on
        [size - window - (i % 3) for i in range(K)],                       # partial block and tail
    ]
    assert all(0 <= s <= size - window for ss in sets for s in ss)
    assert all(s + window > covered for s in sets[2])
    starts = torch.tensor([5 + i for i in range(K)], dtype=torch.int64, device="cuda")
    out = torch.full((K, wb), 0xA5, dtype=torch.uint8, device="cuda")
    ws = bs.decompress_lz4_windows_workspace(st.buf.numel(), size, 2, K, window, b)
    result = torch.zeros(1, dtype=torch.int64, device="cuda")
    status = torch.zeros(K, dtype=torch.int64, device="cuda")
    news = [torch.tensor(ss, dtype=torch.int64, device="cuda") for ss in sets]
    torch.cuda.synchronize()

    def call():
        bs.decompress_lz4_windows_dev(st.buf, size, torch.uint8, starts, window, b, out=out, workspace=ws,
                                      result=result, status=status, offsets=st.offs, elem_size=2, sync=False)

    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        call()
    side.synchronize()
    assert int(result.item()) == K * wb
    assert out.cpu().numpy().tobytes() == expected(st, starts.tolist(), window).tobytes()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        call()
    for ss, new in zip(sets, news):
        starts.copy_(new)
        out.fill_(0xA5)
        result.zero_()
        status.zero_()
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert int(result.item()) == K * wb
        assert status.cpu().tolist() == [wb] * K
        assert out.cpu().numpy().tobytes() == expected(st, ss, window).tobytes()
