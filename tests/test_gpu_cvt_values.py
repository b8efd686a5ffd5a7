"""Decode to float by value: the tables of tests/cvt_values.py -- signed zeros,
subnormals, ties, the overflow edges, non-finite float32 sources, 32-bit
integers above 2**24 with a scale, witnesses of the fused multiply-add and of
the two roundings -- through every path of the span routine of every gather
instantiation, for all 21 kind pairs.

The layouts (cvt_values.Layout) decide which value meets which path; that they
hold every (value, path) pair is asserted on the CPU (tests/test_cvt_values.py),
as is that a kernel with an unfused multiply-add, a single rounding, truncation,
a flush to zero, saturation, float64 integer sources or a sign-less zero would
change an expected bit.  Here the outputs are compared bit for bit with
cvt_values.ref_bits; where the reference is NaN the output must be a NaN of the
destination type.  No tolerance.

As in test_gpu_cvt_decode.py: every output is 0xA5 between 64 guard bytes, and
statuses, offsets and results are compared with the plain entry's on the same
arguments."""
import numpy as np
import pytest

from tests import cvt_values as V
from tests.test_gpu_cvt_decode import (BLOCK, Conv, Out, dev, env, expect_tiles, expect_windows, gs,  # noqa: F401
                                       ragged_expect, replay)
from tests.test_gpu_range_decode import Stream

pytestmark = pytest.mark.gpu

PAIR_IDS = ["%s-%s" % p for p in V.PAIRS]
assert BLOCK == V.BLOCK


class Rig:
    """The streams of one source kind's layout on the device, and the set of
    them with every index supplied (True) and rebuilt by the set (False)."""

    def __init__(self, env, src):
        self.lay = lay = V.layout(src)
        self.streams = []
        for i in range(lay.nstreams):
            data = lay.data(i)
            buf = env.oracle.compress_lz4(data, BLOCK)
            st = Stream(env.bs, env.torch, env.oracle, buf, data.size, data.dtype.itemsize, BLOCK, index=False)
            assert st.want.tobytes() == data.tobytes()
            st.offs = env.bs.api.block_index_dev(st.buf, data.size, st.E, BLOCK)
            self.streams.append(st)
        bufs = [s.buf for s in self.streams]
        offs = [s.offs for s in self.streams]
        self.sets = {True: env.bs.lz4_stream_set_dev(bufs, lay.sizes, lay.S, BLOCK, offsets=offs),
                     False: env.bs.lz4_stream_set_dev(bufs, lay.sizes, lay.S, BLOCK)}
        n = lay.nstreams
        assert self.sets[True].status.cpu().tolist() == [0] * n == self.sets[False].status.cpu().tolist()
        self._refs = {}

    def refs(self, cv):
        """Per stream, the reference's bytes of the whole stream."""
        key = (cv.dst, cv.scale, V.fbits(cv.offset))
        if key not in self._refs:
            self._refs[key] = [V.ref_bits(self.lay.data(i), cv.scale, cv.offset, cv.dst).view(np.uint8)
                               for i in range(self.lay.nstreams)]
        return self._refs[key]


def rig_of(env, src):
    key = ("values", src)
    if key not in env._streams:
        env._streams[key] = Rig(env, src)
    return env._streams[key]


def convs(env, pair):
    return [Conv(env.torch, pair[0], pair[1], s, o) for s, o, _ in V.params(*pair)]


def check(out, exp, cv, what):
    """The output's body against the expected bytes, element by element of the
    destination type; the guards by Out."""
    t = np.uint32 if cv.D == 4 else np.uint16
    got = np.frombuffer(out.body().tobytes(), dtype=t)
    want = np.frombuffer(exp.tobytes(), dtype=t)
    assert got.size == want.size
    bad = V.mismatches(got, want, cv.dst)
    if bad.size:
        i = int(bad[0])
        raise AssertionError("%s -> %s scale %r offset %r, %s: %d elements differ, first at %d: got %#x, want %#x"
                             % (cv.src, cv.dst, cv.scale, cv.offset, what, bad.size, i, got[i], want[i]))


# --------------------------------------------------------------- 1. windows
def run_windows(env, rig, cv, d_starts, starts, window, doff, supplied, plain):
    torch, bs = env.torch, env.bs
    st = rig.streams[0]
    K = len(starts)
    out = Out(torch, K * window, cv.D, cv.tdst, doff)
    status = torch.full((K,), 12345, dtype=torch.int64, device="cuda")
    offs = st.offs if supplied else None
    _, res = bs.decompress_lz4_windows_dev(st.buf, st.size, cv.tsrc, d_starts, window, BLOCK, out=out.t,
                                           status=status, offsets=offs, sync=False, **cv.kw)
    want = [window * cv.S] * K
    assert status.cpu().tolist() == want and int(res.item()) == K * window * cv.S
    check(out, expect_windows(cv, rig.refs(cv), [0] * K, starts, window, want), cv,
          "window %d doff %d supplied %s starts %s" % (window, doff, supplied, starts[:3]))
    if plain:
        pstatus = torch.full((K,), 777, dtype=torch.int64, device="cuda")
        _, pres = bs.decompress_lz4_windows_dev(st.buf, st.size, torch.uint8, d_starts, window, BLOCK,
                                                status=pstatus, offsets=offs, sync=False, elem_size=cv.S)
        assert pstatus.cpu().tolist() == want and int(pres.item()) == int(res.item())


@pytest.mark.parametrize("pair", V.PAIRS, ids=PAIR_IDS)
def test_windows_one_stream(env, pair):
    """Every call of the layout with every parameter set, the index supplied;
    and every call with the index rebuilt, the parameter sets taking turns."""
    rig = rig_of(env, pair[0])
    cvs = convs(env, pair)
    lanes = set()
    for ci, (starts, window, doff) in enumerate(rig.lay.window_calls(cvs[0].D)):
        d_starts = dev(env.torch, starts)
        lanes.add(window * max(cvs[0].S, cvs[0].D) > 2048)
        for pi, cv in enumerate(cvs):
            run_windows(env, rig, cv, d_starts, starts, window, doff, True, plain=pi == 0)
            if pi == ci % len(cvs):
                run_windows(env, rig, cv, d_starts, starts, window, doff, False, plain=False)
    assert lanes == {False, True}


@pytest.mark.parametrize("pair", V.PAIRS, ids=PAIR_IDS)
def test_windows_over_a_set(env, pair):
    """The ends of the short streams, whose verbatim tails hold every value,
    and windows of the long one."""
    torch, bs = env.torch, env.bs
    rig = rig_of(env, pair[0])
    cvs = convs(env, pair)
    for ci, (ids, starts, window, doff) in enumerate(rig.lay.set_calls(cvs[0].D)):
        K = len(ids)
        d_ids, d_starts = dev(torch, ids), dev(torch, starts)
        want = [window * cvs[0].S] * K
        for pi, cv in enumerate(cvs):
            supplied = (pi + ci) % 2 == 0
            out = Out(torch, K * window, cv.D, cv.tdst, doff)
            status = torch.full((K,), 1, dtype=torch.int64, device="cuda")
            _, res = bs.decompress_lz4_windows_set_dev(rig.sets[supplied], cv.tsrc, d_ids, d_starts, window,
                                                       out=out.t, status=status, sync=False, **cv.kw)
            assert status.cpu().tolist() == want
            check(out, expect_windows(cv, rig.refs(cv), ids, starts, window, want), cv,
                  "set window %d ids %s starts %s" % (window, ids[:3], starts[:3]))
            if pi == 0:
                pstatus = torch.full((K,), 2, dtype=torch.int64, device="cuda")
                _, pres = bs.decompress_lz4_windows_set_dev(rig.sets[supplied], torch.uint8, d_ids, d_starts, window,
                                                            status=pstatus, sync=False, elem_size=cv.S)
                assert pstatus.cpu().tolist() == want and int(pres.item()) == int(res.item()) == K * window * cv.S


# ----------------------------------------------------------------- 2. ragged
def ragged_args(rig, D, over_set):
    """The layout's ragged calls; behind their windows the ends of the short
    streams (over a set) or of the long one."""
    lay = rig.lay
    calls, (t_ids, t_starts, t_counts) = lay.ragged_calls(D)
    if not over_set:
        t_ids, t_starts, t_counts = [0, 0], [lay.size - V.TAIL - 2, lay.covered], [V.TAIL + 2, V.TAIL]
    return [(ids + t_ids, starts + t_starts, counts + t_counts, mw, pitch, doff)
            for ids, starts, counts, mw, pitch, doff in calls]


def ragged_call(env, rig, over_set, supplied, dtype, ids, starts, counts, max_window, **kw):
    bs = env.bs
    if over_set:
        return bs.decompress_lz4_ragged_set_dev(rig.sets[supplied], dtype, ids, starts, counts, max_window, **kw)
    st = rig.streams[0]
    return bs.decompress_lz4_ragged_dev(st.buf, st.size, dtype, starts, counts, max_window, block_size=BLOCK,
                                        offsets=st.offs if supplied else None, **kw)


@pytest.mark.parametrize("over_set", [False, True], ids=["stream", "set"])
@pytest.mark.parametrize("pair", V.PAIRS, ids=PAIR_IDS)
def test_ragged(env, pair, over_set):
    """Packed and pitched, a wave and a workgroup per window (by max_window)."""
    torch = env.torch
    rig = rig_of(env, pair[0])
    cvs = convs(env, pair)
    lay = rig.lay
    for ci, (ids, starts, counts, max_window, pitch, doff) in enumerate(ragged_args(rig, cvs[0].D, over_set)):
        K = len(ids)
        capacity = K * pitch if pitch else sum(counts)
        d_ids, d_starts, d_counts = dev(torch, ids), dev(torch, starts), dev(torch, counts)
        for pi, cv in enumerate(cvs):
            supplied = (pi + ci) % 2 == 0
            want, want_offs, exp = ragged_expect(cv, rig.refs(cv), lay.sizes, ids, starts, counts, max_window,
                                                 capacity, pitch)
            assert min(want) >= 0
            out = Out(torch, capacity, cv.D, cv.tdst, doff)
            t = out.t.view(K, pitch) if pitch else out.t
            oo = torch.full((K + 1,), -5, dtype=torch.int64, device="cuda")
            _, _, status, res = ragged_call(env, rig, over_set, supplied, cv.tsrc, d_ids, d_starts, d_counts,
                                            max_window, out=t, out_offsets=oo, pitch=pitch, sync=False, **cv.kw)
            assert status.cpu().tolist() == want and oo.cpu().tolist() == want_offs
            assert int(res.item()) == sum(counts) * cv.S
            check(out, exp, cv, "ragged max_window %d pitch %d set %s" % (max_window, pitch, over_set))
            if pi == 0:
                poo = torch.full((K + 1,), -5, dtype=torch.int64, device="cuda")
                _, _, pstatus, pres = ragged_call(env, rig, over_set, supplied, torch.uint8, d_ids, d_starts,
                                                  d_counts, max_window, out_offsets=poo, pitch=pitch, sync=False,
                                                  elem_size=cv.S)
                assert pstatus.cpu().tolist() == want and poo.cpu().tolist() == want_offs
                assert int(pres.item()) == int(res.item())


# ------------------------------------------------------------------ 3. tiles
@pytest.mark.parametrize("over_set", [False, True], ids=["stream", "set"])
@pytest.mark.parametrize("pair", V.PAIRS, ids=PAIR_IDS)
def test_tiles(env, pair, over_set):
    """Rows of 16, 64 and 256 lanes; over a set also short rows that end in the
    short streams' verbatim tails."""
    torch, bs = env.torch, env.bs
    rig = rig_of(env, pair[0])
    cvs = convs(env, pair)
    lay = rig.lay
    st = rig.streams[0]
    calls = [([0] * len(starts), starts, rows, cols, pitch, doff)
             for starts, rows, cols, pitch, doff in lay.tile_calls(cvs[0].D)]
    if over_set:
        tails = list(range(1, lay.nstreams))
        cols, pitch = V.TAIL + 2, V.TAIL + 3
        calls.append((tails, [lay.small - pitch - cols] * len(tails), 2, cols, pitch, 1))
    lanes = set()
    for ci, (ids, starts, rows, cols, pitch, doff) in enumerate(calls):
        K = len(ids)
        lanes.add(lay.lanes_of_tiles(cvs[0].D, cols))
        d_ids, d_starts = dev(torch, ids), dev(torch, starts)
        want = [rows * cols * cvs[0].S] * K
        for pi, cv in enumerate(cvs):
            supplied = (pi + ci) % 2 == 0
            out = Out(torch, K * rows * cols, cv.D, cv.tdst, doff)
            status = torch.full((K,), 5, dtype=torch.int64, device="cuda")
            pstatus = torch.full((K,), 6, dtype=torch.int64, device="cuda")
            if over_set:
                _, res = bs.decompress_lz4_tiles_set_dev(rig.sets[supplied], cv.tsrc, d_ids, d_starts, rows, cols,
                                                         pitch, out=out.t, status=status, sync=False, **cv.kw)
                if pi == 0:
                    _, pres = bs.decompress_lz4_tiles_set_dev(rig.sets[supplied], torch.uint8, d_ids, d_starts, rows,
                                                              cols, pitch, status=pstatus, sync=False,
                                                              elem_size=cv.S)
            else:
                offs = st.offs if supplied else None
                _, res = bs.decompress_lz4_tiles_dev(st.buf, st.size, cv.tsrc, d_starts, rows, cols, pitch, BLOCK,
                                                     out=out.t, status=status, offsets=offs, sync=False, **cv.kw)
                if pi == 0:
                    _, pres = bs.decompress_lz4_tiles_dev(st.buf, st.size, torch.uint8, d_starts, rows, cols, pitch,
                                                          BLOCK, status=pstatus, offsets=offs, sync=False,
                                                          elem_size=cv.S)
            assert status.cpu().tolist() == want and int(res.item()) == sum(want)
            if pi == 0:
                assert pstatus.cpu().tolist() == want and int(pres.item()) == int(res.item())
            check(out, expect_tiles(cv, rig.refs(cv), ids, starts, rows, cols, pitch, want), cv,
                  "tiles %dx%d pitch %d set %s" % (rows, cols, pitch, over_set))
    assert lanes == {16, 64, 256}


# ---------------------------------------------------------- 4. captured call
def test_capture_ragged(env, gs):  # noqa: F811
    """One converting ragged call on the table stream, float32 -> float16 with
    the parameters that halve normals into subnormals, captured once and
    replayed twice with other starts and counts in the same device arrays."""
    torch, bs = env.torch, env.bs
    rig = rig_of(env, "float32")
    lay, st = rig.lay, rig.streams[0]
    cv = Conv(torch, "float32", "float16", 2.0 ** 125, 0.0)
    sh = lay.shapes(cv.D)
    max_window = sh["mid"]
    K = lay.L + 2
    plans = [(lay.steps(a, n) + [lay.size - 9, lay.covered], [n] * lay.L + [9, V.TAIL])
             for a, n in ((0, sh["mid"]), (1, sh["short"]))]
    src = [(dev(torch, s), dev(torch, c)) for s, c in plans]
    d_starts, d_counts = dev(torch, [0] * K), dev(torch, [0] * K)
    capacity = K * max_window
    ws = bs.decompress_lz4_ragged_workspace(st.buf.numel(), st.size, cv.S, K, max_window, BLOCK)
    out = Out(torch, capacity, cv.D, cv.tdst, 1)
    oo = torch.zeros(K + 1, dtype=torch.int64, device="cuda")
    status = torch.zeros(K, dtype=torch.int64, device="cuda")
    result = torch.zeros(1, dtype=torch.int64, device="cuda")

    def call():
        bs.decompress_lz4_ragged_dev(st.buf, st.size, cv.tsrc, d_starts, d_counts, max_window, out=out.t,
                                     out_offsets=oo, block_size=BLOCK, workspace=ws, result=result, status=status,
                                     offsets=st.offs, stream=gs.torch_stream, sync=False, **cv.kw)

    def fill(k):
        def f():
            out.whole.fill_(0xA5)
            d_starts.copy_(src[k][0])
            d_counts.copy_(src[k][1])
        return f

    def verify(k):
        starts, counts = plans[k]
        want, want_offs, exp = ragged_expect(cv, rig.refs(cv), lay.sizes, [0] * K, starts, counts, max_window,
                                             capacity, 0)
        assert status.cpu().tolist() == want and min(want) >= 0
        assert oo.cpu().tolist() == want_offs and int(result.item()) == sum(counts) * cv.S
        check(out, exp, cv, "replay %d" % k)

    replay(env, gs, call, [fill(0), fill(1)], verify)
