"""Window decode over a set of streams (bshuf_lz4_stream_set_dev,
bshuf_decompress_lz4_windows_set_dev): K windows of one length, window i in
stream ids[i] at starts[i], both device tensors -- byte for byte against slices
of the CPU oracle's decode of the oracle's streams.

Every call writes into an output filled with 0xA5 that has 64 guard bytes in
front and behind, which must come back untouched -- as must the slice of a
window that is not decoded.  Every case runs on a set whose block indexes are
supplied and on one whose indexes the set rebuilt.  No tolerances: tobytes()
equality."""
import copy

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


class Set:
    """Streams of one element and block size, and the two sets of them."""

    def __init__(self, bs, torch, streams, bufs=None):
        self.bs, self.torch, self.streams = bs, torch, streams
        self.E, self.block = streams[0].E, streams[0].block
        self.sizes = [st.size for st in streams]
        self.nb_max = max(st.nb for st in streams)
        self.bufs = [st.buf for st in streams] if bufs is None else bufs
        self._sets = {}

    def sset(self, supplied):
        if supplied not in self._sets:
            offs = [st.offs for st in self.streams] if supplied else None
            self._sets[supplied] = self.bs.lz4_stream_set_dev(self.bufs, self.sizes, self.E, self.block,
                                                              offsets=offs)
        return self._sets[supplied]

    def Mw(self, window):
        return min((window + self.block - 2) // self.block + 1, self.nb_max)

    def good(self, i, start, window):
        if not 0 <= i < len(self.streams):
            return False
        st = self.streams[i]
        return window <= st.size and 0 <= start <= st.size - window and st.nb >= self.Mw(window)

    def statuses(self, ids, starts, window):
        wb = window * self.E
        return [wb if self.good(i, s, window) else -71 for i, s in zip(ids, starts)]

    def expected(self, ids, starts, window, status):
        """(K, window * E) bytes: the oracle's slices; 0xA5 where the window is not written."""
        wb = window * self.E
        exp = np.full((len(ids), wb), 0xA5, dtype=np.uint8)
        for k, (i, s) in enumerate(zip(ids, starts)):
            if status[k] == wb:
                exp[k] = self.streams[i].want[s * self.E:(s + window) * self.E]
        return exp

    def run(self, ids, starts, window, supplied=True, shift=0, sset=None, want_status=None, want_result=None):
        """One call, sync=False; checks the output, the guards, the statuses and the result."""
        torch, E = self.torch, self.E
        if not isinstance(ids, torch.Tensor):
            ids = torch.tensor(list(ids), dtype=torch.int64, device="cuda")
        if not isinstance(starts, torch.Tensor):
            starts = torch.tensor(list(starts), dtype=torch.int64, device="cuda")
        K, wb = starts.numel(), window * E
        whole = torch.full((GUARD + shift + K * wb + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
        out = whole[GUARD + shift:GUARD + shift + K * wb]
        status = torch.full((K,), 12345, dtype=torch.int64, device="cuda")
        o, res = self.bs.decompress_lz4_windows_set_dev(self.sset(supplied) if sset is None else sset,
                                                        torch.uint8, ids, starts, window, out=out,
                                                        status=status, elem_size=E, sync=False)
        torch.cuda.synchronize()
        assert o is out
        hid, hst = ids.cpu().tolist(), starts.cpu().tolist()
        if want_status is None:
            want_status = self.statuses(hid, hst, window)
        assert status.cpu().tolist() == want_status
        if want_result is None:
            bad = [c for c in want_status if c < 0]
            want_result = K * wb if not bad else (-71 if -71 in bad else bad[-1])
        assert int(res.item()) == want_result
        got = whole.cpu().numpy()
        lo = GUARD + shift
        assert got[:lo].tobytes() == b"\xa5" * lo, "bytes in front of the windows were written"
        assert got[lo + K * wb:].tobytes() == b"\xa5" * GUARD, "bytes behind the windows were written"
        exp = self.expected(hid, hst, window, want_status)
        body = got[lo:lo + K * wb].reshape(K, wb)
        if body.tobytes() != exp.tobytes():
            rows = np.nonzero((body != exp).any(axis=1))[0]
            raise AssertionError("windows %s (ids %s, starts %s) of %d differ, window %d E %d"
                                 % (rows[:8].tolist(), [hid[i] for i in rows[:8]],
                                    [hst[i] for i in rows[:8]], K, window, E))
        return status, res

    def both(self, ids, starts, window, **kw):
        self.run(ids, starts, window, supplied=True, **kw)
        self.run(ids, starts, window, supplied=False, **kw)


SMALL = [3 * 64 + 40 + 5,   # four blocks and a tail
         128,               # two blocks, no tail
         5,                 # tail only
         6 * 64 + 7,
         64 + 24]           # a full and a partial block


@pytest.mark.parametrize("E", [1, 2, 4, 8, 3, 12])
def test_every_pair_of_a_small_set(bs, torch, make, E):
    """Every (stream, valid start) pair of every window length in one shuffled
    call, and in the same call one window per stream that cannot take a window
    of that length: -71, its slice untouched."""
    S = Set(bs, torch, [make(E, 64, n, gen=1 if E != 4 else 2) for n in SMALL])
    assert [st.nb for st in S.streams] == [4, 2, 0, 6, 2]
    for supplied in (True, False):
        assert S.sset(supplied).status.cpu().tolist() == [0] * 5
    for window in (1, 2, 8, 63, 64, 65, 66, 131):
        Mw = S.Mw(window)
        pairs, short = [], []
        for i, st in enumerate(S.streams):
            if st.nb >= Mw and st.size >= window:
                pairs += [(i, s) for s in range(st.size - window + 1)]
            else:
                short.append(i)
                pairs.append((i, 0))
        assert 2 in short and (window < 66 or short == [1, 2, 4])
        order = np.random.default_rng(window).permutation(len(pairs))
        ids = [pairs[k][0] for k in order]
        starts = [pairs[k][1] for k in order]
        want = S.statuses(ids, starts, window)
        assert want.count(-71) == len(short)
        S.both(ids, starts, window, want_status=want, want_result=-71)
    # no window refused: the byte count
    S.both([0, 3, 3, 1], [7, 300, 0, 64], 64)


DEFAULT = [5 * 4096 + 1000 + 3, 2 * 4096, 9 * 4096 + 8]


@pytest.mark.parametrize("window", [100, 4098])
def test_default_blocks_device_made_ids_and_starts(bs, torch, make, window):
    """A window of 4098 elements needs three blocks, so the stream of two takes
    none of that length (-71); every other (id, start) is valid by construction."""
    b = 4096
    S = Set(bs, torch, [make(2, b, n) for n in DEFAULT])
    K = 257
    g = torch.Generator(device="cuda").manual_seed(11 + window)
    room = torch.tensor([n - window + 1 for n in DEFAULT], dtype=torch.int64, device="cuda")
    ids = torch.randint(0, 3, (K,), generator=g, device="cuda", dtype=torch.int64)
    starts = torch.randint(0, 2 ** 40, (K,), generator=g, device="cuda", dtype=torch.int64) % room[ids]
    assert set(ids.cpu().tolist()) == {0, 1, 2}
    for shift in (0, 1, 3):
        S.both(ids, starts, window, shift=shift)
    # a real dtype: (K, window) of it, from streams that take the window
    if window == 4098:
        ids = ids.clamp(max=1) * 2
        starts = starts % room[ids]
    for supplied in (True, False):
        y = bs.decompress_lz4_windows_set_dev(S.sset(supplied), torch.int16, ids, starts, window)
        assert y.dtype == torch.int16 and tuple(y.shape) == (K, window)
        hid, hst = ids.cpu().tolist(), starts.cpu().tolist()
        exp = S.expected(hid, hst, window, [window * 2] * K)
        assert y.cpu().numpy().tobytes() == exp.tobytes()


def test_one_stream_set_is_the_window_decode(bs, torch, make):
    b = 64
    size = 3 * b + 40 + 5
    st = make(2, b, size)
    S = Set(bs, torch, [st])
    for window in (1, 70, size):
        starts = [-1, 0, 5, size - window, size - window + 1, 2 ** 62, b - 1]
        K, wb = len(starts), window * 2
        t = torch.tensor(starts, dtype=torch.int64, device="cuda")
        for supplied in (True, False):
            out1 = torch.full((K, wb), 0xA5, dtype=torch.uint8, device="cuda")
            stat1 = torch.zeros(K, dtype=torch.int64, device="cuda")
            _, res1 = bs.decompress_lz4_windows_dev(st.buf, size, torch.uint8, t, window, b, out=out1,
                                                    status=stat1, offsets=st.offs if supplied else None,
                                                    elem_size=2, sync=False)
            status, res = S.run([0] * K, starts, window, supplied=supplied)
            torch.cuda.synchronize()
            assert status.cpu().tolist() == stat1.cpu().tolist()
            assert int(res.item()) == int(res1.item()) == -71
            assert out1.cpu().numpy().tobytes() == S.expected([0] * K, starts, window,
                                                              stat1.cpu().tolist()).tobytes()


def test_one_stream_and_set_calls_agree(bs, torch, make):
    """The two entry points run one window decode: the same shuffled starts --
    every valid one, one in front of the first and one behind the last -- go to
    the call over the stream and, with ids all zero, to the call over a set of
    that one stream.  Output bytes (0xA5-filled, with guards), per-window
    statuses and the result word are compared with each other, not with an
    expectation; index supplied to both, then rebuilt by both."""
    b = 64
    size = 3 * b + 40 + 5      # three full blocks, a partial one, a tail
    st = make(2, b, size)
    S = Set(bs, torch, [st])
    for window in (1, 65, size):
        wb = window * 2
        starts = list(range(-1, size - window + 2))
        K = len(starts)
        order = np.random.default_rng(window).permutation(K)
        t = torch.tensor([starts[k] for k in order], dtype=torch.int64, device="cuda")
        ids = torch.zeros(K, dtype=torch.int64, device="cuda")
        for supplied in (True, False):
            got = []
            for over_set in (False, True):
                whole = torch.full((GUARD + K * wb + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
                out = whole[GUARD:GUARD + K * wb]
                status = torch.full((K,), 12345, dtype=torch.int64, device="cuda")
                if over_set:
                    _, res = bs.decompress_lz4_windows_set_dev(S.sset(supplied), torch.uint8, ids, t, window,
                                                               out=out, status=status, elem_size=2, sync=False)
                else:
                    _, res = bs.decompress_lz4_windows_dev(st.buf, size, torch.uint8, t, window, b, out=out,
                                                           status=status, elem_size=2, sync=False,
                                                           offsets=st.offs if supplied else None)
                torch.cuda.synchronize()
                got.append((whole.cpu().numpy().tobytes(), status.cpu().tolist(), int(res.item())))
            one, over = got
            key = (window, supplied)
            assert one[1] == over[1], key
            assert one[2] == over[2] == -71, key
            assert one[0] == over[0], key
            # and they did something: two refused windows, the others written
            assert sorted(one[1])[:3] == [-71, -71, wb] and one[1].count(wb) == K - 2, key
            assert one[0][:GUARD] == one[0][-GUARD:] == b"\xa5" * GUARD, key


def test_out_of_range_ids_and_starts(bs, torch, make):
    b = 64
    S = Set(bs, torch, [make(2, b, n) for n in (3 * b + 40 + 5, 6 * b + 7, 5 * b)])
    count = 3
    for window in (1, 70, 2 * b):
        wb = window * 2
        ids, starts, want = [], [], []
        for i in (-1, count, 2 ** 40, -2 ** 63):
            ids.append(i)
            starts.append(0)
            want.append(-71)
        for i, st in enumerate(S.streams):
            for s, ok in ((-1, False), (0, True), (st.size - window, True), (st.size - window + 1, False),
                          (2 ** 62, False)):
                ids.append(i)
                starts.append(s)
                want.append(wb if ok else -71)
        S.both(ids, starts, window, want_status=want, want_result=-71)
        with pytest.raises(bs.BshufError) as e:
            bs.decompress_lz4_windows_set_dev(S.sset(True), torch.int16,
                                              torch.tensor(ids, dtype=torch.int64, device="cuda"),
                                              torch.tensor(starts, dtype=torch.int64, device="cuda"), window)
        assert e.value.args[1] == -71


def test_corruption_stays_local(bs, torch, make):
    """Block 2's header of one stream of three is destroyed.  With the indexes
    supplied, a window fails exactly when it holds elements of that block --
    also when the blocks decoded for it include the block and its elements do
    not.  With the indexes rebuilt by the set, that stream's records do not tile
    it: its status is -91 and so is every window in it; the others are served."""
    b = 128
    size = 5 * b + 24 + 5
    streams = [make(2, b, size), make(2, b, size + b), make(2, b, size - b)]
    hurt = streams[1]
    bad = hurt.buf.clone()
    o2 = int(hurt.offs[2].item())
    bad[o2:o2 + 4] = torch.tensor([0x7F, 0xFF, 0xFF, 0xFF], dtype=torch.uint8, device="cuda")
    with pytest.raises(bs.BshufError) as whole:
        bs.decompress_lz4_dev(bad, (hurt.size,), torch.int16, b, offsets=hurt.offs)
    code = whole.value.args[1]
    assert code < 0
    S = Set(bs, torch, streams, bufs=[streams[0].buf, bad, streams[2].buf])
    assert S.sset(True).status.cpu().tolist() == [0, 0, 0]
    assert S.sset(False).status.cpu().tolist() == [0, -91, 0]
    window = 26
    wb = window * 2
    #          blk 0  blk 2   1+2       blk 3     5+6+tail   blk 1 (2 decoded beside it)  2+3
    starts = [10, 2 * b + 1, 2 * b - 10, 3 * b + 5, 6 * b + 3, b + 100, 3 * b - 5]
    touches = [False, True, True, False, False, False, True]
    ids, sts, want, want91 = [], [], [], []
    for k, (s, t) in enumerate(zip(starts, touches)):
        ids += [1, k % 2 * 2]            # one on the hurt stream, one at the same start on another
        sts += [s, min(s, streams[2].size - window)]
        want += [code if t else wb, wb]
        want91 += [-91, wb]
    S.run(ids, sts, window, supplied=True, want_status=want, want_result=code)
    S.run(ids, sts, window, supplied=False, want_status=want91, want_result=-91)
    # no failing window: the byte count
    ok = [k for k in range(len(ids)) if want[k] == wb]
    S.run([ids[k] for k in ok], [sts[k] for k in ok], window, supplied=True)
    with pytest.raises(bs.BshufError) as e:
        bs.decompress_lz4_windows_set_dev(S.sset(True), torch.int16,
                                          torch.tensor(ids, dtype=torch.int64, device="cuda"),
                                          torch.tensor(sts, dtype=torch.int64, device="cuda"), window)
    assert e.value.args[1] == code


def test_shape_mismatch_touches_nothing(bs, torch, make):
    b = 64
    S = Set(bs, torch, [make(2, b, n) for n in (3 * b + 40 + 5, 6 * b + 7, 5 * b)])
    ids, starts = [0, 1, 2, 1], [0, 100, 17, 6 * b + 7 - 70]
    for window in (5, 70):
        for supplied in (True, False):
            S.run(ids, starts, window, supplied=supplied)
            for field, value in (("count", 4), ("count", 2), ("max_size", 7 * b + 7), ("max_size", 4 * b),
                                 ("block_size", 2 * b), ("block_size", 8)):
                other = copy.copy(S.sset(supplied))
                setattr(other, field, value)
                S.run(ids, starts, window, sset=other, want_status=[-71] * 4, want_result=-71)


def test_caller_workspace_and_argument_errors(bs, torch, make):
    b = 128
    size = 5 * b + 24 + 5
    S = Set(bs, torch, [make(2, b, size), make(2, b, size + b)])
    ids = torch.tensor([0, 1, 1], dtype=torch.int64, device="cuda")
    starts = torch.tensor([3, 4 * b + 7, 6 * b], dtype=torch.int64, device="cuda")
    exp = S.expected(ids.tolist(), starts.tolist(), 29, [58] * 3).tobytes()
    for supplied in (True, False):
        sset = S.sset(supplied)
        ws = bs.decompress_lz4_windows_set_workspace(sset, 3, 29)
        n = int(bs.lib.bshuf_decompress_lz4_windows_set_dev_workspace(size + b, 2, b, 3, 29))
        assert ws.numel() == n and ws.data_ptr() % 256 == 0
        y = bs.decompress_lz4_windows_set_dev(sset, torch.int16, ids, starts, 29, workspace=ws)
        assert y.cpu().numpy().tobytes() == exp
        with pytest.raises(bs.BshufError) as e:
            bs.decompress_lz4_windows_set_dev(sset, torch.int16, ids, starts, 29, workspace=ws[:n - 1])
        assert e.value.args[1] == -71
    sset = S.sset(True)
    with pytest.raises(bs.BshufError) as e:
        bs.decompress_lz4_windows_set_dev(sset, torch.int16, ids, starts, size + b + 1)
    assert e.value.args[1] == -71
    # the set built into a caller's workspace of the exact size
    import ctypes
    nbytes = (ctypes.c_size_t * 2)(*[st.buf.numel() for st in S.streams])
    sizes = (ctypes.c_size_t * 2)(*S.sizes)
    n = int(bs.lib.bshuf_lz4_stream_set_dev_workspace(ctypes.cast(nbytes, ctypes.c_void_p),
                                                      ctypes.cast(sizes, ctypes.c_void_p), 2, 2, b))
    ws = torch.empty(n, dtype=torch.uint8, device="cuda")
    own = bs.lz4_stream_set_dev(S.bufs, S.sizes, 2, b, workspace=ws)
    y = bs.decompress_lz4_windows_set_dev(own, torch.int16, ids, starts, 29)
    assert own.status.cpu().tolist() == [0, 0] and y.cpu().numpy().tobytes() == exp
    with pytest.raises(bs.BshufError) as e:
        bs.lz4_stream_set_dev(S.bufs, S.sizes, 2, b, workspace=ws[:n - 1])
    assert e.value.args[1] == -71
    # nothing to decode: result 0
    for K, window in ((0, 5), (3, 0)):
        out, res = bs.decompress_lz4_windows_set_dev(sset, torch.int16, ids[:K], starts[:K], window, sync=False)
        torch.cuda.synchronize()
        assert int(res.item()) == 0 and tuple(out.shape) == (K, window)
    # an empty set: no window can address it
    empty = bs.lz4_stream_set_dev([], [], 2, b)
    assert empty.count == 0
    out, res = bs.decompress_lz4_windows_set_dev(empty, torch.int16, ids[:0], starts[:0], 0, sync=False)
    torch.cuda.synchronize()
    assert int(res.item()) == 0
    for wrong in (starts.cpu(), starts.to(torch.int32), torch.stack([starts, starts], 1)[:, 0],
                  starts.tolist()):
        with pytest.raises(ValueError):
            bs.decompress_lz4_windows_set_dev(sset, torch.int16, ids, wrong, 29)
        with pytest.raises(ValueError):
            bs.decompress_lz4_windows_set_dev(sset, torch.int16, wrong, starts, 29)
    with pytest.raises(ValueError):
        bs.decompress_lz4_windows_set_dev(sset, torch.int16, ids[:2], starts, 29)


def test_nothing_reaches_the_host(bs, torch, make, monkeypatch):
    b = 4096
    S = Set(bs, torch, [make(2, b, n) for n in DEFAULT])
    ids = torch.tensor([0, 2, 0, 1], dtype=torch.int64, device="cuda")
    starts = torch.tensor([0, b - 1, 5 * b + 900, 17], dtype=torch.int64, device="cuda")
    window = 100
    out = torch.full((4, window), 0x5A5A, dtype=torch.int16, device="cuda")
    sets = [S.sset(True), S.sset(False)]
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
    for sset in sets:
        o, res = bs.decompress_lz4_windows_set_dev(sset, torch.int16, ids, starts, window, out=out, sync=False)
    calls = list(seen)
    monkeypatch.undo()
    assert not calls, "a sync=False call read a tensor on the host: %s" % [n for n, _ in calls]
    torch.cuda.synchronize()
    assert int(res.item()) == 4 * window * 2
    exp = S.expected(ids.tolist(), starts.tolist(), window, [window * 2] * 4)
    assert out.cpu().numpy().tobytes() == exp.tobytes()


def test_capture_and_replay(bs, torch, make):
    """One captured call, replayed with other ids and starts in the same tensors."""
    b = 4096
    sizes = [5 * b + 1000 + 3, 4 * b + 24 + 5, 9 * b + 8]
    S = Set(bs, torch, [make(2, b, n) for n in sizes])
    K, window = 64, 4098
    wb = window * 2
    covered = [n - n % 8 for n in sizes]
    plans = [
        ([(i * 7) % 3 for i in range(K)], lambda k, i: (k % 3) * b),                    # block-aligned
        ([(i * 5 + 1) % 3 for i in range(K)], lambda k, i: b - 1 + (k % 2) * b),        # straddling from bs - 1 on
        ([i % 2 for i in range(K)], lambda k, i: sizes[i] - window - (k % 3)),          # partial block and tail
    ]
    sets = [(ids, [f(k, i) for k, i in enumerate(ids)]) for ids, f in plans]
    assert all(S.good(i, s, window) for ids, ss in sets for i, s in zip(ids, ss))
    assert all(s + window > covered[i] for i, s in zip(*sets[2]))
    assert sets[0][0] != sets[1][0] != sets[2][0]
    ids = torch.tensor([i % 3 for i in range(K)], dtype=torch.int64, device="cuda")
    starts = torch.tensor([5 + i for i in range(K)], dtype=torch.int64, device="cuda")
    out = torch.full((K, wb), 0xA5, dtype=torch.uint8, device="cuda")
    sset = S.sset(True)
    ws = bs.decompress_lz4_windows_set_workspace(sset, K, window)
    result = torch.zeros(1, dtype=torch.int64, device="cuda")
    status = torch.zeros(K, dtype=torch.int64, device="cuda")
    news = [(torch.tensor(i, dtype=torch.int64, device="cuda"), torch.tensor(s, dtype=torch.int64, device="cuda"))
            for i, s in sets]
    torch.cuda.synchronize()

    def call():
        bs.decompress_lz4_windows_set_dev(sset, torch.uint8, ids, starts, window, out=out, workspace=ws,
                                          result=result, status=status, elem_size=2, sync=False)

    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        call()
    side.synchronize()
    assert int(result.item()) == K * wb
    assert out.cpu().numpy().tobytes() == S.expected(ids.tolist(), starts.tolist(), window, [wb] * K).tobytes()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        call()
    for (hid, hst), (ni, ns) in zip(sets, news):
        ids.copy_(ni)
        starts.copy_(ns)
        out.fill_(0xA5)
        result.zero_()
        status.zero_()
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert int(result.item()) == K * wb
        assert status.cpu().tolist() == [wb] * K
        assert out.cpu().numpy().tobytes() == S.expected(hid, hst, window, [wb] * K).tobytes()
