"""Decode to float: the converting twins of the window, ragged and tile decodes
(bshuf_decompress_lz4_{windows,ragged,tiles}[_set]_cvt_dev; Python: out_dtype=,
scale=, offset=).

The expected values never come from the library: they are the oracle's decode
of the oracle's stream, converted in numpy as

    r64 = float64(x) * float64(float32(scale)) + float64(float32(offset))
    y32 = r64.astype(float32)            then .astype(float16) / torch's bfloat16

Where the float64 computation is exact (asserted here with fractions), one
rounding to fp32 is what fmaf gives and the outputs are compared byte for byte.
With arbitrary parameters every output must lie within 1 ulp (of the
destination type) of r64: the fp32 fma is within 1/2 ulp32 of the exact value
and the second rounding adds 1/2 ulp of the destination -- a derived bound, not
a measured one.

Every call writes into an `out` filled with 0xA5 that has 64 guard bytes in
front and behind, which must come back untouched, as must every window or tile
that is refused or fails.  Statuses and results are compared word for word
with the plain entry's on the same arguments: they stay in source bytes.

Which VALUES meet the arithmetic on which path of the span routine -- signed
zeros, subnormals, ties, overflow edges, non-finite sources, 32-bit integers
with a scale -- is tests/test_gpu_cvt_values.py's part.

Not expressible from Python and so checked at the C entry only: cvt == NULL and
a misaligned `out` (torch refuses to make such a view)."""
import ctypes
import os
from fractions import Fraction

import numpy as np
import pytest

from tests import hip_graph as H
from tests.test_gpu_range_decode import Stream

pytestmark = pytest.mark.gpu

GUARD = 64
BLOCK = 64
SIZE = 40 * BLOCK + 24 + 5   # forty full blocks, a partial one of 24, a 5-element verbatim tail
COVERED = SIZE - 5
SRC = ["uint8", "int8", "uint16", "int16", "uint32", "int32", "float32"]
DST = ["float32", "float16", "bfloat16"]
SWEEP = [("int16", "float32"), ("uint8", "float16"), ("float32", "bfloat16")]
B_SCALE, B_OFFSET = 2.0 ** -8 + 2.0 ** -12, -3.25
MANT = {"float32": 23, "float16": 10, "bfloat16": 7}
EMIN = {"float32": -126, "float16": -14, "bfloat16": -126}


class Env:
    def __init__(self, bs, torch, oracle):
        self.bs, self.torch, self.oracle = bs, torch, oracle
        self._streams = {}

    def data(self, kind, size, small=False, seed=0):
        rng = np.random.default_rng(1234 + seed + SRC.index(kind))
        dt = np.dtype(kind)
        if kind == "float32":
            # finite normal values, no zero: +-[0.125, 1000)
            v = rng.uniform(0.125, 1000.0, size) * rng.choice([-1.0, 1.0], size)
            a = v.astype(np.float32)
            assert np.isfinite(a).all() and (np.abs(a) >= np.finfo(np.float32).tiny).all()
            return a
        info = np.iinfo(dt)
        if small:
            lo, hi = max(info.min, -(1 << 24) + 1), min(info.max, (1 << 24) - 1)
        else:
            lo, hi = info.min, info.max
        a = rng.integers(lo, hi, size, endpoint=True, dtype=np.int64)
        # runs, so that blocks compress; and the type's extremes
        a[size // 3:size // 3 + 200] = a[size // 3]
        a[:4] = [lo, hi, 0, 1]
        if not small and dt.itemsize == 4:
            a[4:8] = [1 << 24, (1 << 24) + 1, hi - 1, (1 << 24) - 1]
        return a.astype(dt)

    def stream(self, kind, size=SIZE, small=False, seed=0):
        key = (kind, size, small, seed)
        if key not in self._streams:
            data = self.data(kind, size, small, seed)
            buf = self.oracle.compress_lz4(data, BLOCK)
            st = Stream(self.bs, self.torch, self.oracle, buf, size, data.dtype.itemsize, BLOCK, index=False)
            assert st.want.tobytes() == data.tobytes()
            st.offs = self.bs.api.block_index_dev(st.buf, size, st.E, BLOCK)
            st.data = st.want.view(data.dtype)   # the ORACLE's decode, typed
            st.kind = kind
            self._streams[key] = st
        return self._streams[key]


@pytest.fixture(scope="module")
def env(oracle):
    import torch

    import bitshuffle_amd
    assert bitshuffle_amd.using_HIP(), "no HIP device: the GPU suite must run on MI355X"
    assert torch.cuda.is_available()
    return Env(bitshuffle_amd, torch, oracle)


class Conv:
    """One conversion and its reference."""

    def __init__(self, torch, src, dst, scale=1.0, offset=0.0):
        self.torch, self.src, self.dst = torch, src, dst
        self.scale, self.offset = float(scale), float(offset)
        self.S, self.D = np.dtype(src).itemsize, 4 if dst == "float32" else 2
        self.tsrc, self.tdst = getattr(torch, src), getattr(torch, dst)
        self.kw = dict(out_dtype=self.tdst, scale=self.scale, offset=self.offset)

    def struct(self):
        from bitshuffle_amd._lib import Cvt
        return Cvt(SRC.index(self.src), DST.index(self.dst), self.scale, self.offset)

    def r64(self, x):
        return x.astype(np.float64) * np.float64(np.float32(self.scale)) + np.float64(np.float32(self.offset))

    def assert_exact(self, x):
        """The float64 computation of r64 is exact for every element of x."""
        s, o = Fraction(float(np.float32(self.scale))), Fraction(float(np.float32(self.offset)))
        r = self.r64(x)
        for xi, ri in zip(x.tolist(), r.tolist()):
            assert Fraction(xi) * s + o == Fraction(ri), (self.src, self.scale, self.offset, xi)

    def ref(self, x):
        """The reference's bytes for source elements x."""
        with np.errstate(over="ignore"):
            y32 = self.r64(x).astype(np.float32)
            if self.dst == "float32":
                y = y32
            elif self.dst == "float16":
                y = y32.astype(np.float16)
            else:
                y = self.torch.from_numpy(y32.copy()).to(self.torch.bfloat16).view(self.torch.int16).numpy()
        return np.ascontiguousarray(y).view(np.uint8).reshape(-1)

    def values(self, raw):
        """Destination bytes -> float64 values."""
        if self.dst == "float32":
            return raw.view(np.float32).astype(np.float64)
        if self.dst == "float16":
            return raw.view(np.float16).astype(np.float64)
        return (raw.view(np.uint16).astype(np.uint32) << 16).view(np.float32).astype(np.float64)

    def assert_within_1ulp(self, raw, x):
        r = self.r64(x)
        got = self.values(raw)
        _, e = np.frexp(r)                       # r = m * 2**e, 0.5 <= |m| < 1
        e = np.maximum(e - 1, EMIN[self.dst])
        ulp = np.ldexp(1.0, e - MANT[self.dst])
        worst = np.max(np.abs(got - r) / ulp) if r.size else 0.0
        print("%s -> %s scale %r offset %r: worst error %.3f ulp" % (self.src, self.dst, self.scale, self.offset,
                                                                      worst))
        assert np.isfinite(got).all() and worst <= 1.0


class Out:
    """`n` destination elements of 0xA5 between guards, element 0 `doff`
    elements behind a 16-byte boundary."""

    def __init__(self, torch, n, esize, tdtype, doff=0):
        self.lo, self.nbytes = GUARD + doff * esize, n * esize
        self.whole = torch.full((self.lo + self.nbytes + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
        assert self.whole.data_ptr() % 16 == 0
        self.t = self.whole[self.lo:self.lo + self.nbytes].view(tdtype)

    def body(self):
        got = self.whole.cpu().numpy()
        assert got[:self.lo].tobytes() == b"\xa5" * self.lo, "bytes in front of the output were written"
        assert got[self.lo + self.nbytes:].tobytes() == b"\xa5" * GUARD, "bytes behind the output were written"
        return got[self.lo:self.lo + self.nbytes]

    def check(self, exp, what=""):
        body = self.body()
        if body.tobytes() != exp.tobytes():
            bad = np.nonzero(body != exp)[0]
            raise AssertionError("%s: %d bytes differ, first at %d" % (what, bad.size, bad[0]))


def dev(torch, vals):
    return torch.tensor(list(vals), dtype=torch.int64, device="cuda")


def expect_windows(cv, refs, ids, starts, window, status):
    """(K * window * D) bytes: 0xA5 where the window is not written."""
    wb = window * cv.D
    exp = np.full(len(starts) * wb, 0xA5, dtype=np.uint8)
    for k, (i, s) in enumerate(zip(ids, starts)):
        if status[k] >= 0:
            exp[k * wb:(k + 1) * wb] = refs[i][s * cv.D:(s + window) * cv.D]
    return exp


def run_windows(env, st, cv, ref, starts, window, doff=0, offsets="own", buf=None, want_status=None,
                compare_plain=False):
    """One converting window call on one stream; returns (status, result)."""
    torch, bs = env.torch, env.bs
    K = len(starts)
    d_starts = dev(torch, starts)
    out = Out(torch, K * window, cv.D, cv.tdst, doff)
    status = torch.full((K,), 12345, dtype=torch.int64, device="cuda")
    offs = st.offs if offsets == "own" else offsets
    src = st.buf if buf is None else buf
    o, res = bs.decompress_lz4_windows_dev(src, st.size, cv.tsrc, d_starts, window, BLOCK, out=out.t,
                                           status=status, offsets=offs, sync=False, **cv.kw)
    assert o is out.t
    got_status = status.cpu().tolist()
    if window == 0:
        # the plain entry's rule: nothing is decoded, the result is 0, no status is written
        assert got_status == [12345] * K and int(res.item()) == 0
        out.check(np.zeros(0, dtype=np.uint8))
        return got_status, 0
    if want_status is None:
        want_status = [window * cv.S if 0 <= s <= st.size - window else -71 for s in starts]
    assert got_status == want_status, (starts, window)
    out.check(expect_windows(cv, [ref], [0] * K, starts, window, want_status),
              "%s->%s window %d doff %d starts %s" % (cv.src, cv.dst, window, doff, starts[:6]))
    if compare_plain:
        pout = torch.full((max(K * window * cv.S, 1),), 0xA5, dtype=torch.uint8, device="cuda")
        pstatus = torch.full((K,), 777, dtype=torch.int64, device="cuda")
        _, pres = bs.decompress_lz4_windows_dev(src, st.size, torch.uint8, d_starts, window, BLOCK, out=pout,
                                                status=pstatus, offsets=offs, sync=False, elem_size=cv.S)
        assert pstatus.cpu().tolist() == got_status
        assert int(pres.item()) == int(res.item())
    return got_status, int(res.item())


# --------------------------------------------------------------- 1. windows
def lane_rule_lengths(cv):
    """One length on each side of the window gather's thresholds: fewer than 32
    source bytes go singly; a wave per window up to 2048 bytes of the larger
    of source and destination, else a workgroup."""
    single = 32 // cv.S
    edge = 2048 // max(cv.S, cv.D)
    return sorted(set(list(range(0, single + 2)) + [edge, edge + 1]))


@pytest.mark.parametrize("pair", SWEEP, ids=["%s-%s" % p for p in SWEEP])
def test_windows_alignment_sweep(env, pair):
    """Every source element offset within a 16-byte granule x every destination
    element offset within 16 bytes x the lengths of the lane rule, with the
    index supplied and rebuilt; parameters (B), bit-exact."""
    cv = Conv(env.torch, pair[0], pair[1], B_SCALE, B_OFFSET)
    st = env.stream(pair[0])
    cv.assert_exact(st.data)
    ref = cv.ref(st.data)
    per = 16 // cv.S
    for window in lane_rule_lengths(cv):
        # every source offset, in a full block, across blocks and up to the stream's end
        starts = [3 * BLOCK + j for j in range(per)] + [SIZE - window - j for j in range(per)]
        for doff in range(16 // cv.D):
            run_windows(env, st, cv, ref, starts, window, doff=doff)
            run_windows(env, st, cv, ref, starts, window, doff=doff, offsets=None)


def exact_params(src):
    """(scale, offset) with an exact float64 reference for this source kind:
    (C) always; (A) and (B) where product and sum fit 53 bits."""
    ps = [(1.0, 0.0)]
    if np.dtype(src).itemsize < 4 or src == "float32":
        ps += [(float(np.float32(1.0) / np.float32(3.0)), 0.0), (B_SCALE, B_OFFSET)]
    return ps


@pytest.mark.parametrize("dst", DST)
@pytest.mark.parametrize("src", SRC)
def test_every_pair_bit_exact(env, src, dst):
    """(A) a scale with a full 24-bit significand, (B) a few bits each, (C)
    scale 1 offset 0, which must be numpy's astype -- on the whole value range
    of every kind, 32-bit integers at and above 2**24 included."""
    st = env.stream(src)
    per = 16 // st.E
    for scale, offset in exact_params(src):
        cv = Conv(env.torch, src, dst, scale, offset)
        cv.assert_exact(st.data)
        ref = cv.ref(st.data)
        if (scale, offset) == (1.0, 0.0):
            y32 = st.data.astype(np.float32)
            if dst == "float32":
                assert np.array_equal(ref.view(np.float32), y32)
            elif dst == "float16":
                with np.errstate(over="ignore"):
                    assert np.array_equal(ref.view(np.float16), y32.astype(np.float16))
        for window, starts in ((1, [0, 7, SIZE - 1]), (37, [0, 5, BLOCK - 3, SIZE - 37]),
                               (300, [1, 2 * BLOCK + per - 1, SIZE - 300]), (SIZE, [0])):
            run_windows(env, st, cv, ref, starts, window, doff=1)
        # the values at the start of the stream: the type's extremes
        run_windows(env, st, cv, ref, [0], 16, offsets=None)


@pytest.mark.parametrize("dst", DST)
@pytest.mark.parametrize("src", SRC[:6])
def test_general_parameters_within_one_ulp(env, src, dst):
    """A mean / std normalisation with arbitrary floats; 32-bit integers with
    |x| < 2**24."""
    torch, bs = env.torch, env.bs
    st = env.stream(src, small=True, seed=7)
    assert np.abs(st.data.astype(np.int64)).max() < (1 << 24)
    # (a std that keeps 2**24 / std inside float16's range)
    mean, std = {1: (101.7, 57.3), 2: (1234.567, 57.3), 4: (123456.7, 5730.1)}[st.E]
    cv = Conv(torch, src, dst, 1.0 / std, -mean / std)
    K, window = 8, SIZE // 8
    starts = [k * window + (k % 3) for k in range(K)]
    starts[-1] = SIZE - window
    out = Out(torch, K * window, cv.D, cv.tdst, 1)
    bs.decompress_lz4_windows_dev(st.buf, st.size, cv.tsrc, dev(torch, starts), window, BLOCK, out=out.t,
                                  offsets=st.offs, **cv.kw)
    x = np.concatenate([st.data[s:s + window] for s in starts])
    cv.assert_within_1ulp(out.body(), x)


def test_f16_overflows_to_inf(env):
    st = env.stream("uint16")
    cv = Conv(env.torch, "uint16", "float16", 2.0, 0.0)   # 65504 < 2 * x for x above 32752
    cv.assert_exact(st.data)
    ref = cv.ref(st.data)
    assert np.isinf(ref.view(np.float16)).any() and np.isfinite(ref.view(np.float16)).any()
    run_windows(env, st, cv, ref, [0, 33, SIZE - 700], 700)


# ------------------------------------------------------------ 2. stream ends
@pytest.mark.parametrize("pair", SWEEP + [("int32", "float32"), ("uint16", "bfloat16"), ("int8", "float32")],
                         ids=lambda p: "%s-%s" % p)
def test_stream_ends_and_odd_stream_addresses(env, pair):
    """Windows that end in the partial last block, end in the verbatim tail and
    lie wholly in it, of a stream at an odd byte address: the tail's elements
    are then misaligned for their own size."""
    torch = env.torch
    cv = Conv(torch, pair[0], pair[1], B_SCALE if pair[0] != "int32" else 1.0, B_OFFSET if pair[0] != "int32" else 0.0)
    st = env.stream(pair[0])
    assert SIZE % BLOCK != 0 and SIZE % 8 != 0
    cv.assert_exact(st.data)
    ref = cv.ref(st.data)
    odd = torch.empty(st.buf.numel() + 1, dtype=torch.uint8, device="cuda")
    odd[1:] = st.buf
    assert odd[1:].data_ptr() % 2 == 1
    cases = [(30, [COVERED - 34, COVERED - 30]),            # end in the partial block
             (20, [SIZE - 20, SIZE - 21, COVERED - 19]),    # end in the tail
             (3, [COVERED, COVERED + 1, SIZE - 3]),         # wholly in the tail
             (5, [COVERED]), (1, [SIZE - 1, COVERED]),
             (200, [SIZE - 200, SIZE - 201])]
    for window, starts in cases:
        for buf in (None, odd[1:]):
            run_windows(env, st, cv, ref, starts, window, doff=1, buf=buf)
            run_windows(env, st, cv, ref, starts, window, doff=0, buf=buf, offsets=None)


# ------------------------------------------------ 3. bad and failing windows
def corrupt(env, st, blk):
    bad = st.buf.clone()
    o = int(st.offs[blk].item())
    bad[o:o + 4] = env.torch.tensor([0x7F, 0xFF, 0xFF, 0xFF], dtype=env.torch.uint8, device="cuda")
    with pytest.raises(env.bs.BshufError) as whole:
        env.bs.decompress_lz4_dev(bad, (st.size,), env.torch.uint8, BLOCK, offsets=st.offs, elem_size=st.E)
    assert whole.value.args[1] < 0
    return bad, whole.value.args[1]


@pytest.mark.parametrize("pair", SWEEP, ids=lambda p: "%s-%s" % p)
def test_bad_and_failing_windows(env, pair):
    cv = Conv(env.torch, pair[0], pair[1], B_SCALE, B_OFFSET)
    st = env.stream(pair[0])
    ref = cv.ref(st.data)
    window = 26
    # starts outside [0, size - window]: -71, the slice untouched, the others converted
    starts = [5, -1, SIZE - window, SIZE - window + 1, 1 << 40, 3 * BLOCK]
    status, res = run_windows(env, st, cv, ref, starts, window, doff=1, compare_plain=True)
    assert status == [window * cv.S, -71, window * cv.S, -71, -71, window * cv.S] and res == -71
    status, res = run_windows(env, st, cv, ref, starts, window, offsets=None, compare_plain=True)
    assert res == -71
    # no bad window: the result is the SOURCE byte count
    status, res = run_windows(env, st, cv, ref, [5, 70, 9], window, compare_plain=True)
    assert res == 3 * window * cv.S
    # block 2 corrupt, index supplied: a window with an element of it reports the
    # decode's code and is not written; its neighbours are converted
    bad, code = corrupt(env, st, 2)
    starts = [10, 2 * BLOCK + 1, 2 * BLOCK - 10, 3 * BLOCK, 2 * BLOCK - window, SIZE - window]
    touches = [False, True, True, False, False, False]
    want = [code if t else window * cv.S for t in touches]
    status, res = run_windows(env, st, cv, ref, starts, window, doff=1, buf=bad, want_status=want,
                              compare_plain=True)
    assert res == code


# ------------------------------------------------------ 4. windows over a set
class SetRig:
    """Three streams of different lengths; stream 1's block-2 header is
    destroyed.  `supplied`: every index given (stream 1 then fails per block);
    else stream 1's index is rebuilt by the set and its records do not tile it
    (-91 for every window in it)."""

    def __init__(self, env, kind):
        self.env = env
        self.streams = [env.stream(kind), env.stream(kind, SIZE + BLOCK, seed=1), env.stream(kind, SIZE - BLOCK, seed=2)]
        self.bad, self.code = corrupt(env, self.streams[1], 2)
        self.bufs = [self.streams[0].buf, self.bad, self.streams[2].buf]
        self.sizes = [s.size for s in self.streams]
        self.E = self.streams[0].E
        offs = [s.offs for s in self.streams]
        self.sets = {True: env.bs.lz4_stream_set_dev(self.bufs, self.sizes, self.E, BLOCK, offsets=offs),
                     False: env.bs.lz4_stream_set_dev(self.bufs, self.sizes, self.E, BLOCK,
                                                      offsets=[offs[0], None, offs[2]])}
        assert self.sets[True].status.cpu().tolist() == [0, 0, 0]
        assert self.sets[False].status.cpu().tolist() == [0, -91, 0]
        self.clean = env.bs.lz4_stream_set_dev([s.buf for s in self.streams], self.sizes, self.E, BLOCK, offsets=offs)

    def refs(self, cv):
        return [cv.ref(s.data) for s in self.streams]


@pytest.mark.parametrize("pair", [("int16", "float32"), ("uint8", "bfloat16")], ids=lambda p: "%s-%s" % p)
def test_windows_over_a_set(env, pair):
    torch, bs = env.torch, env.bs
    cv = Conv(torch, pair[0], pair[1], B_SCALE, B_OFFSET)
    rig = SetRig(env, pair[0])
    refs = rig.refs(cv)
    window = 26
    wb = window * cv.S
    ids = [0, 1, 1, 2, -1, 3, 0, 2, 1, 2]
    starts = [7, 10, 2 * BLOCK + 1, rig.sizes[2] - window, 5, 5, rig.sizes[0] - window + 1, 0, 3 * BLOCK, -3]
    for supplied in (True, False):
        want = []
        for i, s in zip(ids, starts):
            if not 0 <= i < 3 or not 0 <= s <= rig.sizes[i] - window:
                want.append(-71)
            elif i == 1 and not supplied:
                want.append(-91)
            elif i == 1 and s <= 3 * BLOCK - 1 and s + window > 2 * BLOCK:
                want.append(rig.code)
            else:
                want.append(wb)
        K = len(ids)
        d_ids, d_starts = dev(torch, ids), dev(torch, starts)
        out = Out(torch, K * window, cv.D, cv.tdst, 3)
        status = torch.full((K,), 1, dtype=torch.int64, device="cuda")
        _, res = bs.decompress_lz4_windows_set_dev(rig.sets[supplied], cv.tsrc, d_ids, d_starts, window, out=out.t,
                                                   status=status, sync=False, **cv.kw)
        assert status.cpu().tolist() == want
        out.check(expect_windows(cv, refs, ids, starts, window, want), "set, supplied %s" % supplied)
        pstatus = torch.full((K,), 2, dtype=torch.int64, device="cuda")
        _, pres = bs.decompress_lz4_windows_set_dev(rig.sets[supplied], torch.uint8, d_ids, d_starts, window,
                                                    status=pstatus, sync=False, elem_size=cv.S)
        assert pstatus.cpu().tolist() == want and int(pres.item()) == int(res.item()) == -71


# ------------------------------------------------------------------ 5. tiles
def tile_G(rows, cols, pitch, nb):
    so = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "bitshuffle_amd", "libbshuf_hostcheck.so")
    h = ctypes.CDLL(so)
    out = (ctypes.c_int64 * 3)()
    h.bshuf_hostcheck_tile_shape.argtypes = [ctypes.c_int64] * 5 + [ctypes.POINTER(ctypes.c_int64)]
    h.bshuf_hostcheck_tile_shape(rows, cols, pitch, BLOCK, nb, out)
    return out[1]


def expect_tiles(cv, refs, ids, starts, rows, cols, pitch, status):
    tb = rows * cols * cv.D
    exp = np.full(len(starts) * tb, 0xA5, dtype=np.uint8)
    for k, (i, s) in enumerate(zip(ids, starts)):
        if status[k] >= 0:
            for r in range(rows):
                a = s + r * pitch
                exp[k * tb + r * cols * cv.D:k * tb + (r + 1) * cols * cv.D] = refs[i][a * cv.D:(a + cols) * cv.D]
    return exp


TILE_PITCH = 520
TILE_SIZE = 26 * TILE_PITCH + 24 + 5


@pytest.mark.parametrize("pair", [("int16", "float32"), ("uint8", "float16"), ("float32", "bfloat16")],
                         ids=lambda p: "%s-%s" % p)
def test_tiles_one_stream(env, pair):
    """cols on each side of the tile gather's lane thresholds (1024 and 2048
    bytes of the larger of a row's source and destination bytes), rows above
    256 / T, G == 1 and G > 1, a last row that reaches the tail, a bad tile and
    a tile with a failing block, which is not written at all."""
    torch, bs = env.torch, env.bs
    cv = Conv(torch, pair[0], pair[1], B_SCALE, B_OFFSET)
    st = env.stream(pair[0], TILE_SIZE, seed=3)
    cv.assert_exact(st.data)
    ref = cv.ref(st.data)
    wide = max(cv.S, cv.D)
    e16, e64 = 1024 // wide, 2048 // wide
    shapes = [(18, e16, TILE_PITCH), (18, 13, TILE_PITCH), (6, e16 + 1, TILE_PITCH), (6, min(e64, TILE_PITCH), TILE_PITCH)]
    if e64 + 1 <= TILE_PITCH:
        shapes.append((3, e64 + 1, TILE_PITCH))
    else:
        shapes.append((3, e64 + 1, e64 + 1))
    shapes.append((7, TILE_PITCH, TILE_PITCH))   # whole rows: one group
    Gs = set()
    bad, code = corrupt(env, st, 9)
    for rows, cols, pitch in shapes:
        span = (rows - 1) * pitch + cols
        assert span <= TILE_SIZE
        Gs.add(min(tile_G(rows, cols, pitch, st.nb), 2))
        starts = [0, 3, TILE_SIZE - span, -1, TILE_SIZE - span + 1, pitch + 7 if pitch + 7 + span <= TILE_SIZE else 1]
        want = [rows * cols * cv.S if 0 <= s <= TILE_SIZE - span else -71 for s in starts]
        for offsets, doff in ((st.offs, 1), (None, 0)):
            out = Out(torch, len(starts) * rows * cols, cv.D, cv.tdst, doff)
            status = torch.full((len(starts),), 5, dtype=torch.int64, device="cuda")
            d_starts = dev(torch, starts)
            _, res = bs.decompress_lz4_tiles_dev(st.buf, st.size, cv.tsrc, d_starts, rows, cols, pitch, BLOCK,
                                                 out=out.t, status=status, offsets=offsets, sync=False, **cv.kw)
            assert status.cpu().tolist() == want
            out.check(expect_tiles(cv, [ref], [0] * len(starts), starts, rows, cols, pitch, want),
                      "tiles %dx%d pitch %d" % (rows, cols, pitch))
            pstatus = torch.full((len(starts),), 6, dtype=torch.int64, device="cuda")
            _, pres = bs.decompress_lz4_tiles_dev(st.buf, st.size, torch.uint8, d_starts, rows, cols, pitch, BLOCK,
                                                  status=pstatus, offsets=offsets, sync=False, elem_size=cv.S)
            assert pstatus.cpu().tolist() == want and int(pres.item()) == int(res.item()) == -71
        # block 9 (elements 576..639) fails: tiles with an element of it are left alone
        starts = [0, 3, TILE_SIZE - span, 9 * BLOCK + 1]
        want = []
        for s in starts:
            hit = any(a < 10 * BLOCK and a + cols > 9 * BLOCK for a in range(s, s + rows * pitch, pitch))
            want.append(code if hit else rows * cols * cv.S)
        out = Out(torch, len(starts) * rows * cols, cv.D, cv.tdst, 2)
        status = torch.full((len(starts),), 5, dtype=torch.int64, device="cuda")
        bs.decompress_lz4_tiles_dev(bad, st.size, cv.tsrc, dev(torch, starts), rows, cols, pitch, BLOCK, out=out.t,
                                    status=status, offsets=st.offs, sync=False, **cv.kw)
        assert status.cpu().tolist() == want
        assert code in want
        out.check(expect_tiles(cv, [ref], [0] * len(starts), starts, rows, cols, pitch, want), "failing tile")
    assert Gs == {1, 2}, "the shapes must cover one group and several"


def test_tiles_over_a_set(env):
    torch, bs = env.torch, env.bs
    cv = Conv(torch, "int16", "float16", B_SCALE, B_OFFSET)
    rig = SetRig(env, "int16")
    refs = rig.refs(cv)
    rows, cols, pitch = 5, 40, 100
    span = (rows - 1) * pitch + cols
    ids = [0, 2, 1, 1, 3, 0, 2]
    starts = [11, rig.sizes[2] - span, 3 * BLOCK, 0, 0, rig.sizes[0] - span + 1, 64]
    want = []
    for i, s in zip(ids, starts):
        if not 0 <= i < 3 or not 0 <= s <= rig.sizes[i] - span:
            want.append(-71)
        elif i == 1 and any(a < 3 * BLOCK and a + cols > 2 * BLOCK for a in range(s, s + rows * pitch, pitch)):
            want.append(rig.code)
        else:
            want.append(rows * cols * cv.S)
    assert rig.code in want
    d_ids, d_starts = dev(torch, ids), dev(torch, starts)
    out = Out(torch, len(ids) * rows * cols, cv.D, cv.tdst, 5)
    status = torch.full((len(ids),), 5, dtype=torch.int64, device="cuda")
    _, res = bs.decompress_lz4_tiles_set_dev(rig.sets[True], cv.tsrc, d_ids, d_starts, rows, cols, pitch, out=out.t,
                                             status=status, sync=False, **cv.kw)
    assert status.cpu().tolist() == want
    out.check(expect_tiles(cv, refs, ids, starts, rows, cols, pitch, want), "tiles over a set")
    pstatus = torch.full((len(ids),), 6, dtype=torch.int64, device="cuda")
    _, pres = bs.decompress_lz4_tiles_set_dev(rig.sets[True], torch.uint8, d_ids, d_starts, rows, cols, pitch,
                                              status=pstatus, sync=False, elem_size=cv.S)
    assert pstatus.cpu().tolist() == want and int(pres.item()) == int(res.item()) == -71


# ----------------------------------------------------------------- 6. ragged
def ragged_expect(cv, refs, sizes, ids, starts, counts, max_window, capacity, pitch):
    """(status, offsets, bytes of `capacity` destination elements)."""
    status, offs, at = [], [0], 0
    exp = np.full(capacity * cv.D, 0xA5, dtype=np.uint8)
    for k, (i, s, n) in enumerate(zip(ids, starts, counts)):
        good = 0 <= i < len(sizes) and 0 <= n <= max_window and 0 <= s <= sizes[i] - n
        place = k * pitch if pitch else at
        fits = pitch or n == 0 or n <= capacity - at
        if good and fits:
            status.append(n * cv.S)
            exp[place * cv.D:(place + n) * cv.D] = refs[i][s * cv.D:(s + n) * cv.D]
        else:
            status.append(-71)
        at += n if good else 0
        offs.append(at)
    return status, offs, exp


@pytest.mark.parametrize("pitched", [False, True])
@pytest.mark.parametrize("over_set", [False, True])
def test_ragged(env, over_set, pitched):
    torch, bs = env.torch, env.bs
    cv = Conv(torch, "int16", "bfloat16" if over_set else "float32", B_SCALE, B_OFFSET)
    for max_window in (600, 150):    # 2400 destination bytes: a workgroup per window; 600: a wave
        if over_set:
            rig = SetRig(env, "int16")
            sizes, refs, sset = rig.sizes, [cv.ref(s.data) for s in rig.streams], rig.clean
            ids = [0, 1, 2, 0, 5, 1, 2, 0, 1]
        else:
            st = env.stream("int16")
            sizes, refs = [SIZE], [cv.ref(st.data)]
            ids = [0] * 9
        counts = [0, 1, max_window, max_window + 1, 40, 33, 5, max_window, 77]
        starts = [3, SIZE - BLOCK - 1, 9, 0, 100, -1, sizes[ids[6]] - 5, 64, 2 * BLOCK - 1]
        K = len(ids)
        pitch = max_window + 3 if pitched else 0
        # packed: room for everything but the last good window
        total = sum(n for i, s, n in zip(ids, starts, counts)
                    if 0 <= i < len(sizes) and 0 <= n <= max_window and 0 <= s <= sizes[i] - n)
        capacity = K * pitch if pitched else total - 10
        want, want_offs, exp = ragged_expect(cv, refs, sizes, ids, starts, counts, max_window, capacity, pitch)
        if not pitched:
            assert want[-1] == -71 and want[-2] >= 0, "one window is refused for capacity"
        d_ids, d_starts, d_counts = dev(torch, ids), dev(torch, starts), dev(torch, counts)
        for offsets in ((None,) if over_set else ("own", None)):
            out = Out(torch, capacity, cv.D, cv.tdst, 1)
            t = out.t.view(K, pitch) if pitched else out.t
            oo = torch.full((K + 1,), -5, dtype=torch.int64, device="cuda")
            poo = oo.clone()
            pout = torch.full((capacity * cv.S,), 0xA5, dtype=torch.uint8, device="cuda")
            pout = pout.view(K, pitch * cv.S) if pitched else pout
            kw = dict(out_offsets=oo, pitch=pitch, sync=False)
            pkw = dict(out=pout, out_offsets=poo, pitch=pitch, sync=False, elem_size=cv.S)
            if over_set:
                _, _, status, res = bs.decompress_lz4_ragged_set_dev(sset, cv.tsrc, d_ids, d_starts, d_counts,
                                                                     max_window, out=t, **kw, **cv.kw)
                _, _, pstatus, pres = bs.decompress_lz4_ragged_set_dev(sset, torch.uint8, d_ids, d_starts, d_counts,
                                                                       max_window, **pkw)
            else:
                offs = st.offs if offsets == "own" else None
                _, _, status, res = bs.decompress_lz4_ragged_dev(st.buf, SIZE, cv.tsrc, d_starts, d_counts,
                                                                 max_window, out=t, block_size=BLOCK, offsets=offs,
                                                                 **kw, **cv.kw)
                _, _, pstatus, pres = bs.decompress_lz4_ragged_dev(st.buf, SIZE, torch.uint8, d_starts, d_counts,
                                                                   max_window, block_size=BLOCK, offsets=offs, **pkw)
            assert status.cpu().tolist() == want == pstatus.cpu().tolist()
            assert oo.cpu().tolist() == want_offs == poo.cpu().tolist()
            assert int(res.item()) == int(pres.item()) == -71
            out.check(exp, "ragged set %s pitched %s" % (over_set, pitched))
        # without refused windows: the result is off[K] * elem_size, source bytes
        good = [k for k in range(K) if want[k] >= 0]
        g = [dev(torch, [v[k] for k in good]) for v in (ids, starts, counts)]
        cap = sum(counts[k] for k in good) if not pitched else len(good) * pitch
        out = Out(torch, cap, cv.D, cv.tdst, 0)
        t = out.t.view(len(good), pitch) if pitched else out.t
        if over_set:
            _, o2, _, res = bs.decompress_lz4_ragged_set_dev(sset, cv.tsrc, g[0], g[1], g[2], max_window, out=t,
                                                             pitch=pitch, sync=False, **cv.kw)
        else:
            _, o2, _, res = bs.decompress_lz4_ragged_dev(st.buf, SIZE, cv.tsrc, g[1], g[2], max_window, out=t,
                                                         pitch=pitch, block_size=BLOCK, sync=False, **cv.kw)
        assert int(res.item()) == sum(counts[k] for k in good) * cv.S == int(o2[-1].item()) * cv.S


# ------------------------------------------------------------ 7. host errors
def test_host_errors_c_entries(env):
    """Each refusal is -71 before anything is enqueued: the output stays 0xA5."""
    from bitshuffle_amd._lib import Cvt, lib
    torch = env.torch
    st = env.stream("int16")
    rig = SetRig(env, "int16")
    starts = dev(torch, [0, 5])
    ids = dev(torch, [0, 2])
    counts = dev(torch, [4, 4])
    whole = torch.full((4096,), 0xA5, dtype=torch.uint8, device="cuda")
    res = torch.full((1,), 99, dtype=torch.int64, device="cuda")
    oo = torch.zeros(3, dtype=torch.int64, device="cuda")
    outp = whole.data_ptr() + 64
    p = lambda t: ctypes.c_void_p(t.data_ptr())

    def calls(es, out, cvt):
        table = p(rig.clean.table)
        return [
            lib.bshuf_decompress_lz4_windows_cvt_dev(p(st.buf), st.buf.numel(), SIZE, es, BLOCK, p(starts), 2, 8,
                                                     out, None, 0, p(res), None, None, None, cvt),
            lib.bshuf_decompress_lz4_windows_set_cvt_dev(table, 3, rig.clean.max_size, es, BLOCK, p(ids), p(starts),
                                                         2, 8, out, None, 0, p(res), None, None, cvt),
            lib.bshuf_decompress_lz4_ragged_cvt_dev(p(st.buf), st.buf.numel(), SIZE, es, BLOCK, p(starts), p(counts),
                                                    2, 8, out, 64, 0, p(oo), None, 0, p(res), None, None, None, cvt),
            lib.bshuf_decompress_lz4_ragged_set_cvt_dev(table, 3, rig.clean.max_size, es, BLOCK, p(ids), p(starts),
                                                        p(counts), 2, 8, out, 64, 0, p(oo), None, 0, p(res), None,
                                                        None, cvt),
            lib.bshuf_decompress_lz4_tiles_cvt_dev(p(st.buf), st.buf.numel(), SIZE, es, BLOCK, p(starts), 2, 2, 4,
                                                   16, out, None, 0, p(res), None, None, None, cvt),
            lib.bshuf_decompress_lz4_tiles_set_cvt_dev(table, 3, rig.clean.max_size, es, BLOCK, p(ids), p(starts), 2,
                                                       2, 4, 16, out, None, 0, p(res), None, None, cvt),
        ]

    ok = Cvt(3, 0, 1.0, 0.0)   # int16 -> float32
    refusals = [
        (2, outp, ctypes.byref(Cvt(0, 0, 1.0, 0.0))),    # a 1-byte kind for 2-byte elements
        (2, outp, ctypes.byref(Cvt(5, 1, 1.0, 0.0))),    # a 4-byte kind
        (3, outp, ctypes.byref(ok)),                     # elem_size 3
        (8, outp, ctypes.byref(ok)),                     # elem_size 8
        (2, outp, ctypes.byref(Cvt(7, 0, 1.0, 0.0))),    # unknown source kind
        (2, outp, ctypes.byref(Cvt(-1, 0, 1.0, 0.0))),
        (2, outp, ctypes.byref(Cvt(3, 3, 1.0, 0.0))),    # unknown destination kind
        (2, outp, None),                                 # cvt == NULL
        (2, outp + 2, ctypes.byref(ok)),                 # out not aligned to float32
        (2, outp + 1, ctypes.byref(Cvt(3, 2, 1.0, 0.0))),  # out not aligned to bfloat16
    ]
    for es, out, cvt in refusals:
        assert calls(es, ctypes.c_void_p(out), cvt) == [-71] * 6, (es, out - outp)
    # an out that is too small, where the entry is told its size: pitched ragged rows
    too_small = lib.bshuf_decompress_lz4_ragged_cvt_dev(p(st.buf), st.buf.numel(), SIZE, 2, BLOCK, p(starts),
                                                        p(counts), 2, 8, ctypes.c_void_p(outp), 15, 8, p(oo), None, 0,
                                                        p(res), None, None, None, ctypes.byref(ok))
    assert too_small == -71
    torch.cuda.synchronize()
    assert whole.cpu().numpy().tobytes() == b"\xa5" * 4096 and int(res.item()) == 99
    # the same arguments with a valid conversion are accepted
    assert calls(2, ctypes.c_void_p(outp), ctypes.byref(ok)) == [0] * 6
    torch.cuda.synchronize()


def test_host_errors_python(env):
    torch, bs = env.torch, env.bs
    st = env.stream("int16")
    rig = SetRig(env, "int16")
    s2, i2, c2 = dev(torch, [0, 5]), dev(torch, [0, 2]), dev(torch, [4, 4])
    f32 = torch.float32

    def six(dtype, **kw):
        w = kw.pop("wout", None)
        r = kw.pop("rout", None)
        t = kw.pop("tout", None)
        return [
            lambda: bs.decompress_lz4_windows_dev(st.buf, SIZE, dtype, s2, 8, BLOCK, out=w, **kw),
            lambda: bs.decompress_lz4_windows_set_dev(rig.clean, dtype, i2, s2, 8, out=w, **kw),
            lambda: bs.decompress_lz4_ragged_dev(st.buf, SIZE, dtype, s2, c2, 8, block_size=BLOCK, out=r, pitch=8, **kw),
            lambda: bs.decompress_lz4_ragged_set_dev(rig.clean, dtype, i2, s2, c2, 8, out=r, pitch=8, **kw),
            lambda: bs.decompress_lz4_tiles_dev(st.buf, SIZE, dtype, s2, 2, 4, 16, BLOCK, out=t, **kw),
            lambda: bs.decompress_lz4_tiles_set_dev(rig.clean, dtype, i2, s2, 2, 4, 16, out=t, **kw),
        ]

    small = torch.empty(15, dtype=f32, device="cuda")
    half = torch.empty(64, dtype=torch.float16, device="cuda")
    cases = [six(torch.float64, out_dtype=f32),                  # an 8-byte kind
             six(torch.int64, out_dtype=f32),
             six(torch.bool, out_dtype=f32),                     # an unknown kind
             six(torch.int16, out_dtype=torch.float64),          # an unknown destination
             six(torch.int16, out_dtype=torch.int32),
             six(torch.uint8, out_dtype=f32, elem_size=3),       # elem_size= does not go with out_dtype
             six(torch.int16, out_dtype=f32, elem_size=2),
             six(torch.int16, out_dtype=f32, wout=small, rout=small, tout=small),   # out too small
             six(torch.int16, out_dtype=f32, wout=half, rout=half, tout=half)]      # out of another dtype
    for fns in cases:
        for fn in fns:
            with pytest.raises(ValueError):
                fn()
    # a kind whose size is not the set's element size
    for fn in six(torch.uint8, out_dtype=f32)[1::2]:
        with pytest.raises(ValueError):
            fn()
    # ... and of a single stream the size comes from the dtype: int16's calls are accepted
    for fn in six(torch.int16, out_dtype=f32):
        fn()


# ---------------------------------------------------------- 8. graph capture
@pytest.fixture
def gs():
    g = H.GraphStream()
    yield g
    g.close()


def replay(env, gs, call, fills, check):
    """Captures call() once, replays it twice; fills[k]() changes the device
    arrays before replay k (stream-ordered), check(k) compares its output."""
    torch = env.torch
    torch.cuda.synchronize()
    g = gs.capture(lambda: (call(), 0)[1])
    try:
        assert set(g.types) <= {H.KERNEL, H.MEMCPY, H.MEMSET}, g.names()
        assert g.is_linear_chain()
        g.instantiate()
        for k, fill in enumerate(fills):
            with torch.cuda.stream(gs.torch_stream):
                fill()
            g.launch()
            gs.synchronize()
            check(k)
    finally:
        g.destroy()


def test_capture_windows_set(env, gs):
    torch, bs = env.torch, env.bs
    cv = Conv(torch, "int16", "float32", B_SCALE, B_OFFSET)
    rig = SetRig(env, "int16")
    refs = rig.refs(cv)
    window, K = 100, 4
    plans = [([0, 2, 0, 2], [5, 70, SIZE - window, 0]), ([2, 0, 7, 0], [64, 1, 0, -1])]
    src = [(dev(torch, i), dev(torch, s)) for i, s in plans]
    d_ids, d_starts = dev(torch, [0] * K), dev(torch, [0] * K)
    ws = bs.decompress_lz4_windows_set_workspace(rig.clean, K, window)
    out = Out(torch, K * window, cv.D, cv.tdst, 1)
    status = torch.zeros(K, dtype=torch.int64, device="cuda")
    result = torch.zeros(1, dtype=torch.int64, device="cuda")

    def call():
        bs.decompress_lz4_windows_set_dev(rig.clean, cv.tsrc, d_ids, d_starts, window, out=out.t, workspace=ws,
                                          result=result, status=status, stream=gs.torch_stream, sync=False, **cv.kw)

    def fill(k):
        def f():
            out.whole.fill_(0xA5)
            d_ids.copy_(src[k][0])
            d_starts.copy_(src[k][1])
        return f

    def check(k):
        ids, starts = plans[k]
        want = [window * cv.S if 0 <= i < 3 and 0 <= s <= rig.sizes[i] - window else -71
                for i, s in zip(ids, starts)]
        assert status.cpu().tolist() == want
        out.check(expect_windows(cv, refs, ids, starts, window, want), "replay %d" % k)

    replay(env, gs, call, [fill(0), fill(1)], check)


def test_capture_tiles(env, gs):
    torch, bs = env.torch, env.bs
    cv = Conv(torch, "uint8", "bfloat16", B_SCALE, B_OFFSET)
    st = env.stream("uint8")
    ref = cv.ref(st.data)
    rows, cols, pitch, K = 6, 50, 100, 3
    span = (rows - 1) * pitch + cols
    plans = [[0, 17, SIZE - span], [SIZE - span + 1, 300, 1]]
    src = [dev(torch, s) for s in plans]
    d_starts = dev(torch, [0] * K)
    ws = bs.decompress_lz4_tiles_workspace(st.buf.numel(), SIZE, 1, K, rows, cols, pitch, BLOCK)
    out = Out(torch, K * rows * cols, cv.D, cv.tdst, 3)
    status = torch.zeros(K, dtype=torch.int64, device="cuda")
    result = torch.zeros(1, dtype=torch.int64, device="cuda")

    def call():
        bs.decompress_lz4_tiles_dev(st.buf, SIZE, cv.tsrc, d_starts, rows, cols, pitch, BLOCK, out=out.t,
                                    workspace=ws, result=result, status=status, offsets=st.offs,
                                    stream=gs.torch_stream, sync=False, **cv.kw)

    def fill(k):
        def f():
            out.whole.fill_(0xA5)
            d_starts.copy_(src[k])
        return f

    def check(k):
        starts = plans[k]
        want = [rows * cols * cv.S if 0 <= s <= SIZE - span else -71 for s in starts]
        assert status.cpu().tolist() == want
        out.check(expect_tiles(cv, [ref], [0] * K, starts, rows, cols, pitch, want), "replay %d" % k)

    replay(env, gs, call, [fill(0), fill(1)], check)


# ------------------------------------------- 9. out_dtype=None changes nothing
def test_defaults_change_nothing(env):
    torch, bs = env.torch, env.bs
    st = env.stream("int16")
    rig = SetRig(env, "int16")
    s, i, c = dev(torch, [3, 70, SIZE - 50]), dev(torch, [0, 2, 1]), dev(torch, [50, 0, 17])
    s_set = dev(torch, [3, 70, 5 * BLOCK])
    none = dict(out_dtype=None, scale=1.0, offset=0.0)
    pairs = [
        lambda **kw: bs.decompress_lz4_windows_dev(st.buf, SIZE, torch.int16, s, 50, BLOCK, **kw),
        lambda **kw: bs.decompress_lz4_windows_set_dev(rig.clean, torch.int16, i, s_set, 50, **kw),
        lambda **kw: bs.decompress_lz4_tiles_dev(st.buf, SIZE, torch.int16, s_set, 3, 20, 64, BLOCK, **kw),
        lambda **kw: bs.decompress_lz4_tiles_set_dev(rig.clean, torch.int16, i, s_set, 3, 20, 64, **kw),
    ]
    for fn in pairs:
        a, b = fn(), fn(**none)
        assert a.dtype == b.dtype == torch.int16 and a.shape == b.shape
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    ragged = [
        lambda **kw: bs.decompress_lz4_ragged_dev(st.buf, SIZE, torch.int16, s, c, 50, block_size=BLOCK, **kw),
        lambda **kw: bs.decompress_lz4_ragged_set_dev(rig.clean, torch.int16, i, s_set, c, 50, **kw),
    ]
    for fn in ragged:
        a, b = fn(), fn(**none)
        n = int(a[1][-1].item())
        assert a[0].dtype == b[0].dtype == torch.int16
        assert a[0][:n].cpu().numpy().tobytes() == b[0][:n].cpu().numpy().tobytes()
        assert a[1].cpu().tolist() == b[1].cpu().tolist() and a[2].cpu().tolist() == b[2].cpu().tolist()
