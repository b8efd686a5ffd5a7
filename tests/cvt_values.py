"""Decode to float by value: tables of chosen source values and parameters, the
reference, wrong variants of it, and the layouts that put every table value on
every path of the converting span (tests/test_cvt_values.py on the CPU,
tests/test_gpu_cvt_values.py on the GPU).

The rule: y = dst(fmaf(float32(x), scale, offset)) -- one fp32
fused multiply-add, every rounding to nearest even, overflow to infinity.

Two statements of it live here.  `ref_bits` is the vectorised one the GPU
tests compare with, through float64:

    r64 = float64(x32) * float64(float32(scale)) + float64(float32(offset))
    y32 = r64.astype(float32), then astype(float16) / an integer restatement
    of round-to-nearest-even for bfloat16

`model_bits` is a scalar one in exact rational arithmetic (fractions) with its
own rounding routine; the CPU test holds the two against each other on every
(value, parameters) entry, so y32 is a single rounding of the exact value even
where r64 is not exact.  model_bits also takes a `wrong=` flag: the variants of
the sensitivity test.

Comparison is of bits.  Only where the reference is NaN is the output merely
required to be a NaN of the destination type.  There is no tolerance."""
import ctypes
import math
import os
from fractions import Fraction

import numpy as np

SRC = ["uint8", "int8", "uint16", "int16", "uint32", "int32", "float32"]
DST = ["float32", "float16", "bfloat16"]
PAIRS = [(s, d) for s in SRC for d in DST]
DSIZE = {"float32": 4, "float16": 2, "bfloat16": 2}
BLOCK = 64
TAIL = 7          # elements of a stream's verbatim tail
PARTIAL = 24      # elements of the partial last block

f32 = np.float32


def fbits(v):
    """The bits of float32(v)."""
    return int(np.array([v], dtype=np.float32).view(np.uint32)[0])


# ------------------------------------------------------------------ the tables
# (value, reason); float32 sources as bit patterns
_EVERY_INT = [
    (0, "zero: with (-1, -0.0) the result is -0 and keeps its sign"),
    (1, "with 2**-25 / 2**-134 a tie that goes to 0; with an offset the ties 2049 and 257"),
    (2, "2 * 2**127 overflows the fma"),
    (3, "fused witness with (1 + 2**-23, -3); 3 * 2**-26 rounds up to the smallest half subnormal; 2051, 259"),
    (5, "odd: a tie between subnormals at 2**-25 / 2**-134 that goes down to even"),
    (7, "odd: such a tie that goes up to even"),
    (64, "65440 + 64 = 65504, the largest half"),
    (79, "65440 + 79 = 65519, the last value that rounds to 65504"),
    (80, "65440 + 80 = 65520, the tie that goes to inf"),
    (100, "a plain value"),
]
_WIDE_INT = [
    (257, "bfloat16 tie to even, down to 256"),
    (259, "bfloat16 tie to even, up to 260"),
    (771, "771 * float32(1/3): rounded twice differs from rounded once, to bfloat16"),
    (2049, "half tie to even, down to 2048"),
    (2051, "half tie to even, up to 2052"),
    (4097, "fused witness with (1 + 2**-12, -4098): 2**-12 fused, 0 unfused"),
    (6147, "6147 * float32(1/3): rounded twice differs from rounded once, to half"),
]
_HALF_EDGE = [
    (65504, "the largest half"),
    (65519, "rounds to 65504"),
    (65520, "the tie that goes to inf"),
]
_ABOVE_2_24 = [
    ((1 << 24) + 1, "a tie in (float)x, down to 2**24"),
    ((1 << 24) + 3, "a tie in (float)x, up to 2**24 + 4"),
]
TABLE = {
    "uint8": _EVERY_INT + [(255, "the largest"), (128, "the sign bit of the signed kind"), (254, "even, large")],
    "int8": _EVERY_INT + [(127, "the largest"), (-128, "the smallest"), (-1, "minus one"), (-2, "-2 * 2**127 = -inf"),
                          (-3, "the fused witness, negative"), (-80, "a negative value of some size")],
    "uint16": _EVERY_INT + _WIDE_INT + _HALF_EDGE + [(65535, "the largest"), (32768, "the sign bit of int16")],
    "int16": _EVERY_INT + _WIDE_INT + [(32767, "the largest"), (-32768, "the smallest"), (-1, "minus one"),
                                       (-2, "-2 * 2**127 = -inf"), (-2049, "half tie, negative"),
                                       (-2051, "half tie, negative"), (-257, "bfloat16 tie, negative"),
                                       (-259, "bfloat16 tie, negative")],
    "uint32": _EVERY_INT + _WIDE_INT + _HALF_EDGE + _ABOVE_2_24 + [
        (0xFFFFFF7F, "2**32 - 129: (float)x rounds down to 2**32 - 256"),
        (0xFFFFFF80, "2**32 - 128: a tie in (float)x, up to 2**32"),
        (0xFFFFFFFF, "the largest: (float)x is 2**32"),
        (0x80000000, "the sign bit of int32"),
        (0x7FFFFFFF, "2**31 - 1: (float)x is 2**31")],
    "int32": _EVERY_INT + _WIDE_INT + _HALF_EDGE + _ABOVE_2_24 + [
        (-(1 << 24) - 1, "a tie in (float)x, negative"),
        (-(1 << 24) - 3, "a tie in (float)x, negative"),
        (-(1 << 31), "INT32_MIN"),
        ((1 << 31) - 1, "INT32_MAX: (float)x is 2**31"),
        ((1 << 31) - 1 - 64, "INT32_MAX - 64: (float)x rounds up to 2**31"),
        ((1 << 31) - 1 - 65, "INT32_MAX - 65: (float)x rounds down to 2**31 - 128"),
        (-1, "minus one"), (-2, "-2 * 2**127 = -inf"), (-65520, "the half tie that goes to -inf"),
        (-65519, "rounds to -65504")],
    "float32": [
        (0x00000000, "+0"), (0x80000000, "-0"),
        (0x7F800000, "+inf"), (0xFF800000, "-inf"),
        (0x7FC00000, "a quiet NaN"), (0x7FC00001, "a quiet NaN with a payload in the low mantissa bits"),
        (0xFFC01234, "a negative quiet NaN with a payload"),
        (0x00000001, "the smallest subnormal"), (0x80000001, "the smallest subnormal, negative"),
        (0x007FFFFF, "the largest subnormal"), (0x807FFFFF, "the largest subnormal, negative"),
        (0x00000003, "subnormal 3 * 2**-149: halved it is a tie that goes up to 2 * 2**-149"),
        (0x00800000, "the smallest normal: halved it is a subnormal"), (0x80800000, "the smallest normal, negative"),
        (0x00800001, "the smallest normal and one ulp: halved it is a tie in the subnormals"),
        (0x7F7FFFFF, "FLT_MAX: doubled it is inf"), (0xFF7FFFFF, "-FLT_MAX"),
        (0x7F7F8000, "the tie above the largest bfloat16: inf"), (0x7F7F7FFF, "the last value that stays 0x7F7F"),
        (0xFF7F8000, "that tie, negative"), (0x7F7F8001, "above that tie"),
        (fbits(1.0), "one"), (fbits(-1.0), "minus one"),
        (fbits(3.0), "fused witness with (1 + 2**-23, -3)"), (fbits(-3.0), "the same, negative"),
        (fbits(4097.0), "fused witness with (1 + 2**-12, -4098)"),
        (fbits(6147.0), "6147 * float32(1/3): rounded twice differs from rounded once, to half"),
        (fbits(771.0), "771 * float32(1/3): rounded twice differs from rounded once, to bfloat16"),
        (fbits(65504.0), "the largest half"), (fbits(65519.0), "rounds to 65504"),
        (fbits(65520.0), "the tie that goes to inf in half"), (fbits(-65504.0), "the largest half, negative"),
        (fbits(-65519.0), "rounds to -65504"), (fbits(-65520.0), "the tie that goes to -inf in half"),
        (fbits(2049.0), "half tie, down"), (fbits(2051.0), "half tie, up"),
        (fbits(2049.0) + 1, "just above a half tie: up"),
        (fbits(257.0), "bfloat16 tie, down"), (fbits(259.0), "bfloat16 tie, up"),
        (fbits(2.0 ** -24), "the smallest half subnormal"), (fbits(2.0 ** -25), "a tie that goes to 0 in half"),
        (fbits(-2.0 ** -25), "a tie that goes to -0 in half"),
        (fbits(3 * 2.0 ** -25), "a tie between half subnormals, up to 2 * 2**-24"),
        (fbits(3 * 2.0 ** -26), "rounds up to the smallest half subnormal"),
        (fbits(1023 * 2.0 ** -24), "the largest half subnormal"),
        (fbits(2.0 ** -14), "the smallest normal half"),
        (fbits(2.0 ** -133), "the smallest bfloat16 subnormal"), (fbits(2.0 ** -134), "a tie to 0 in bfloat16"),
        (fbits(3 * 2.0 ** -134), "a tie between bfloat16 subnormals, up"),
        (fbits(-3 * 2.0 ** -134), "the same, negative"),
        (fbits(0.1), "a plain value with a full significand"),
    ],
}

# (scale, offset, reason)
_P_EVERY = [
    (1.0, 0.0, "the cast alone"),
    (-1.0, -0.0, "fmaf(0, -1, -0.0) is -0; every sign flipped"),
    (1.0 + 2.0 ** -23, -3.0, "fused witness at x = 3: 3 * 2**-23 fused, 2**-21 unfused"),
    (1.0 + 2.0 ** -12, -4098.0, "fused witness at x = 4097: 2**-12 fused, 0 unfused"),
    (float(f32(1.0) / f32(3.0)), 0.0, "a full significand: y32 on 16-bit midpoints (6147, 771)"),
]
_P_INT = {
    "float32": [
        (2.0 ** -149, 0.0, "exact fp32 subnormal results"),
        (2.0 ** 127, 0.0, "the fma overflows to +-inf from |x| = 2"),
        (2.0 ** -20, 2049.0, "kept for every destination: a sum the fp32 rounding moves"),
    ],
    "float16": [
        (2.0 ** -24, 0.0, "exact half subnormals"),
        (2.0 ** -25, 0.0, "odd x: a tie between half subnormals, x = 1 ties to 0"),
        (2.0 ** -26, 0.0, "x = 3 rounds up to the smallest half subnormal"),
        (1.0, 65440.0, "the overflow edge: x = 64 stays 65504, 79 gives 65504, 80 ties to inf"),
        (-1.0, -65440.0, "the same edge, negative"),
        (1.0, 2048.0, "ties of both parities: x = 1 gives 2048, x = 3 gives 2052"),
        (2.0 ** -20, 2049.0, "x = 1: y32 is the midpoint 2049, so 2048; rounded once it is 2050"),
        (2.0 ** 127, 0.0, "the fma overflows to +-inf"),
        (-(2.0 ** -20), 2049.0 + 2.0 ** -12, "x = 1: y32 rounds up past the midpoint 2049; a truncating fma gives 2049"),
    ],
    "bfloat16": [
        (1.0, 256.0, "ties of both parities: x = 1 gives 256, x = 3 gives 260"),
        (2.0 ** -133, 0.0, "exact bfloat16 subnormals"),
        (2.0 ** -134, 0.0, "odd x: a tie between bfloat16 subnormals, x = 1 ties to 0"),
        (2.0 ** -20, 257.0, "x = 1: y32 is the midpoint 257, so 256; rounded once it is 258"),
        (2.0 ** 127, 0.0, "the fma overflows to +-inf"),
        (-(2.0 ** -20), 257.0 + 2.0 ** -15, "x = 1: y32 rounds up past the midpoint 257; a truncating fma gives 257"),
    ],
}
_P_INT32 = [
    (0.5, 0.25, "x = 2**24 + 1: 2**23 from (float)x, 2**23 + 1 from float64(x)"),
    (2.0 ** -4, -(2.0 ** 20), "x = 2**24 + 1: 0 from (float)x, 2**-4 from float64(x)"),
    (2.0 ** 120, 0.0, "the fma overflows to +-inf from |x| = 2**8"),
]
_P_F32 = [
    (1.0, -0.0, "the identity that keeps -0 (x + -0.0)"),
    (2.0, 0.0, "FLT_MAX doubles to inf; subnormals double exactly"),
    (0.5, 0.0, "moves normals into subnormals, ties among subnormals"),
    (0.0, 0.0, "inf * 0 is NaN; finite * 0 keeps the product's sign"),
    (2.0 ** 125, 0.0, "fp32 subnormal inputs become half subnormals: 2**-149 * 2**125 = 2**-24"),
    (2.0 ** -20, 2049.0, "x = 1: y32 is the half midpoint 2049"),
    (2.0 ** -20, 257.0, "x = 1: y32 is the bfloat16 midpoint 257"),
    (-(2.0 ** -20), 2049.0 + 2.0 ** -12, "x = 1: y32 rounds up past the half midpoint 2049"),
    (-(2.0 ** -20), 257.0 + 2.0 ** -15, "x = 1: y32 rounds up past the bfloat16 midpoint 257"),
]


def params(src, dst):
    """The parameter sets of a kind pair: [(scale, offset, reason)]."""
    if src == "float32":
        return _P_EVERY + _P_F32
    ps = _P_EVERY + _P_INT[dst]
    if np.dtype(src).itemsize == 4:
        ps = ps + _P_INT32
    return ps


def table_array(src):
    """The table's values as an array of the source kind."""
    vals = [v for v, _ in TABLE[src]]
    if src == "float32":
        return np.array(vals, dtype=np.uint32).view(np.float32)
    a = np.array(vals, dtype=np.int64).astype(np.dtype(src))
    assert a.astype(np.int64).tolist() == vals, src
    return a


# -------------------------------------------------- the reference, vectorised
def bf16_rne(u):
    """float32 bits (uint32 array, no NaN among them) -> bfloat16 bits, to
    nearest even."""
    u = u.astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def to_dst_bits(y32, dst):
    """float32 array -> the destination's bits (uint32 / uint16 array)."""
    y32 = np.ascontiguousarray(y32, dtype=np.float32)
    if dst == "float32":
        return y32.view(np.uint32).copy()
    if dst == "float16":
        with np.errstate(over="ignore", under="ignore"):
            return y32.astype(np.float16).view(np.uint16)
    u = y32.view(np.uint32)
    nan = np.isnan(y32)
    out = bf16_rne(np.where(nan, 0, u))
    out[nan] = 0x7FC0
    return out


def x32_of(x):
    return x.astype(np.float32)


def r64_of(x, scale, offset):
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        return x32_of(x).astype(np.float64) * np.float64(f32(scale)) + np.float64(f32(offset))


def ref_bits(x, scale, offset, dst):
    """The reference's bits for source elements x (an array of a source kind)."""
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        y32 = r64_of(x, scale, offset).astype(np.float32)
    return to_dst_bits(y32, dst)


def is_nan_bits(bits, dst):
    if dst == "float32":
        return (bits & 0x7FFFFFFF) > 0x7F800000
    if dst == "float16":
        return (bits & 0x7FFF) > 0x7C00
    return (bits & 0x7FFF) > 0x7F80


def mismatches(got, exp, dst):
    """Indices where `got` is not `exp`: bit for bit, but any NaN of the
    destination type where exp is NaN."""
    nan = is_nan_bits(exp, dst)
    ok = np.where(nan, is_nan_bits(got, dst), got == exp)
    return np.nonzero(~ok)[0]


# ------------------------------------------- the rule again, scalar and exact
FMT = {"float32": (23, -126, 127), "float16": (10, -14, 15), "bfloat16": (7, -126, 127)}
INF = float("inf")


def round_to(q, fmt, trunc=False):
    """Fraction q != 0 -> the nearest value of a binary format (mantissa bits,
    emin, emax) as a Python float, ties to even (or truncated), subnormals
    gradual, overflow to inf (truncation: to the largest finite)."""
    mant, emin, emax = FMT[fmt]
    sign = -1.0 if q < 0 else 1.0
    a = abs(q)
    e = a.numerator.bit_length() - a.denominator.bit_length()
    if Fraction(2) ** e > a:
        e -= 1
    assert Fraction(2) ** e <= a < Fraction(2) ** (e + 1)
    e = max(e, emin)
    ulp = Fraction(2) ** (e - mant)
    n = a / ulp
    k = n.numerator // n.denominator
    rem = n - k
    if not trunc and (rem > Fraction(1, 2) or (rem == Fraction(1, 2) and k % 2 == 1)):
        k += 1
    v = k * ulp
    big = (Fraction(2) - Fraction(2) ** -mant) * Fraction(2) ** emax
    if v > big:
        return sign * INF
    return sign * float(v)   # exact: every format here is narrower than a double


def largest(fmt):
    mant, _, emax = FMT[fmt]
    return float((Fraction(2) - Fraction(2) ** -mant) * Fraction(2) ** emax)


def smallest_normal(fmt):
    return float(Fraction(2) ** FMT[fmt][1])


WRONG = ["unfused", "once", "trunc_fma", "trunc_cvt", "ftz_in", "ftz_fma", "ftz_cvt", "saturate", "via_f64",
         "no_sign_of_zero"]


def wrong_applies(wrong, src, dst):
    """Whether a wrong variant can show in the bytes of a kind pair at all."""
    if wrong in ("once", "trunc_cvt", "ftz_cvt"):
        return dst != "float32"          # there is no second rounding to fp32
    if wrong == "ftz_in":
        return src == "float32"          # only fp32 sources have subnormals
    if wrong == "ftz_fma":
        # a flushed fp32 subnormal is far below half the smallest half subnormal: zero either way
        return dst != "float16"
    if wrong == "via_f64":
        return src in ("uint32", "int32")
    return True


def _signed_zero(neg):
    return -0.0 if neg else 0.0


def _neg(v):
    return math.copysign(1.0, v) < 0


def model_y32(src, x, scale, offset, wrong=None):
    """fmaf(float32(x), scale, offset) as a Python float (inf, nan included),
    from exact arithmetic; `wrong`: one of WRONG, or None for the rule.
    x: an int, or for float32 the bit pattern."""
    s, o = float(f32(scale)), float(f32(offset))
    if src == "float32":
        xv = float(np.array([x], dtype=np.uint32).view(np.float32)[0])
        if wrong == "ftz_in" and xv != 0 and abs(xv) < smallest_normal("float32"):
            xv = _signed_zero(xv < 0)
    elif wrong == "via_f64":
        xv = float(x)
    else:
        xv = float(np.array([x], dtype=np.int64).astype(np.float32)[0])
    if math.isnan(xv):
        return xv
    if math.isinf(xv):
        if s == 0:
            return float("nan")
        return -xv if _neg(s) else xv     # (offset is finite)
    p = Fraction(xv) * Fraction(s)
    pneg = _neg(xv) != _neg(s)
    trunc = wrong == "trunc_fma"
    if wrong == "unfused" and p != 0:
        p32 = round_to(p, "float32")
        if math.isinf(p32):
            return p32
        p = Fraction(p32)
    q = p + Fraction(o)
    if q == 0:
        y = _signed_zero(pneg and _neg(o)) if p == 0 else 0.0
    else:
        y = round_to(q, "float32", trunc)
    if wrong == "ftz_fma" and y != 0 and abs(y) < smallest_normal("float32"):
        y = _signed_zero(y < 0)
    if wrong == "saturate" and math.isinf(y):
        y = math.copysign(largest("float32"), y)
    if wrong == "once":
        return (y, q)
    return y


def model_bits(src, dst, x, scale, offset, wrong=None):
    """The destination's bits of one element by the rule, or by a wrong variant
    of it."""
    y = model_y32(src, x, scale, offset, wrong)
    q = None
    if isinstance(y, tuple):
        y, q = y
    if dst != "float32" and not math.isnan(y) and not math.isinf(y) and y != 0:
        if wrong == "once" and q is not None and q != 0:
            z = round_to(q, dst)                      # the exact sum, rounded once
        else:
            z = round_to(Fraction(y), dst, wrong == "trunc_cvt")
        if z == 0:
            z = _signed_zero(y < 0)
        if wrong == "ftz_cvt" and z != 0 and abs(z) < smallest_normal(dst):
            z = _signed_zero(z < 0)
        if wrong == "saturate" and math.isinf(z):
            z = math.copysign(largest(dst), z)
        y = z
    if wrong == "no_sign_of_zero" and y == 0:
        y = 0.0
    y32 = np.array([y], dtype=np.float32)           # exact: y is a value of dst
    if dst == "float32":
        return int(y32.view(np.uint32)[0])
    if dst == "float16":
        return int(y32.astype(np.float16).view(np.uint16)[0])
    return 0x7FC0 if math.isnan(y) else int(y32.view(np.uint32)[0]) >> 16


def entry_is_finite(src, x):
    if src == "float32":
        xv = float(np.array([x], dtype=np.uint32).view(np.float32)[0])
        return math.isfinite(xv)
    return True


def r64_is_exact(src, x, scale, offset):
    """Whether the float64 computation of r64 is the exact value (finite x)."""
    xa = np.array([x], dtype=np.uint32).view(np.float32) if src == "float32" else np.array([x], dtype=np.int64)
    r = float(r64_of(xa, scale, offset)[0])
    exact = Fraction(float(x32_of(xa)[0])) * Fraction(float(f32(scale))) + Fraction(float(f32(offset)))
    return math.isfinite(r) and Fraction(r) == exact


# ------------------------------------------------------------ path classifier
HERE = os.path.dirname(os.path.abspath(__file__))
SO = os.path.join(HERE, "..", "bitshuffle_amd", "libbshuf_hostcheck.so")
_lib = None


def hostcheck():
    global _lib
    if _lib is None:
        if not os.path.exists(SO):
            import bitshuffle_amd._lib as L
            L.build()
        h = ctypes.CDLL(SO)
        h.bshuf_hostcheck_cvt_span.argtypes = [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_int, ctypes.c_int,
                                               ctypes.c_int64, ctypes.POINTER(ctypes.c_int64)]
        h.bshuf_hostcheck_cvt_span.restype = None
        _lib = h
    return _lib


_span_cache = {}


def span_paths(src16, dst16, S, D, n):
    """The path of each of the n elements of one span (span_cvt, by
    cvt_span_plan): 'single' (a short span), 'head', 'unit-aligned',
    'unit-shifted[k]' (k the word offset r >> 2 of its instantiation), 'chunk',
    'tail'."""
    key = (src16 % 16, dst16 % 16, S, D, n)
    if key not in _span_cache:
        out = (ctypes.c_int64 * 6)()
        hostcheck().bshuf_hostcheck_cvt_span(key[0], key[1], S, D, n, out)
        head, nu, nc, tail, ue, r = list(out)
        if n * S < 32:
            assert head == n and nu == nc == tail == 0
            paths = ["single"] * n
        else:
            unit = "unit-aligned" if r == 0 else "unit-shifted[%d]" % (r >> 2)
            paths = ["head"] * head + [unit] * (nu * ue) + ["chunk"] * (nc * (16 // D)) + ["tail"] * tail
        assert len(paths) == n, key
        _span_cache[key] = paths
    return _span_cache[key]


_all_paths = {}


def all_paths(S, D):
    """Every path a span of S-byte elements written as D-byte elements can take
    (without 'vtail'), found by enumeration."""
    if (S, D) not in _all_paths:
        found = set()
        for so in range(0, 16, S):
            for do in range(0, 16, D):
                for n in range(0, 81):
                    found.update(span_paths(so, do, S, D, n))
        _all_paths[(S, D)] = found
    return _all_paths[(S, D)]


def piece_paths(S, D, start, n, covered, dst_elem):
    """Paths of elements [start, start + n) of a stream whose first `covered`
    elements are in blocks (staging areas are 16-byte aligned and blocks a
    multiple of 16 bytes, so the source's offset follows from `start`), written
    `dst_elem` elements behind a 16-byte boundary of the output."""
    clip = max(0, min(start + n, covered) - start)
    paths = list(span_paths(start * S, dst_elem * D, S, D, clip)) if clip else []
    return paths + ["vtail"] * (n - clip)


# -------------------------------------------------------------------- layouts
class Layout:
    """The streams of one source kind and the calls on them for one
    destination size.

    Stream 0: the table, cyclically, with a run so that blocks compress; an
    odd period, so that windows 16 elements apart see every value at every
    position (16 elements keep the source's offset within its granule for
    every element size).  Streams 1..: short ones whose 7-element verbatim
    tails together hold every value."""

    def __init__(self, src):
        self.src = src
        self.S = np.dtype(src).itemsize
        self.vals = table_array(src)
        self.nv = len(self.vals)
        self.cyc = list(range(self.nv)) + ([0] if self.nv % 2 == 0 else [])
        self.L = len(self.cyc)
        assert math.gcd(self.L, 16) == 1
        S = self.S
        longest = 2048 // max(S, 2) + 3 * 16
        need = 16 * self.L + 2 * (longest + 16) + 16
        self.run = 160
        nb = -(-(need + self.run + BLOCK) // BLOCK)
        self.size = nb * BLOCK + PARTIAL + TAIL
        self.covered = self.size - TAIL
        idx = np.array([self.cyc[p % self.L] for p in range(self.size)])
        self.run_lo = nb * BLOCK - self.run - 10
        assert self.run_lo >= need
        idx[self.run_lo:self.run_lo + self.run] = idx[self.run_lo]
        self.small = 2 * BLOCK + 8 + TAIL
        self.idx = [idx]
        for j in range(-(-self.L // TAIL)):
            shift = TAIL * j - (self.small - TAIL)
            self.idx.append(np.array([self.cyc[(p + shift) % self.L] for p in range(self.small)]))
        self.sizes = [len(i) for i in self.idx]
        self.nstreams = len(self.idx)
        held = set()
        for i in self.idx[1:]:
            held.update(i[-TAIL:].tolist())
        assert held == set(range(self.nv))

    def data(self, i):
        return self.vals[self.idx[i]]

    def covered_of(self, i):
        return self.sizes[i] - TAIL

    # ---- the shapes of a destination size
    def shapes(self, D):
        S = self.S
        epc = 16 // D
        ue = max(16 // S, epc)
        wide = max(S, D)
        return dict(epc=epc, ue=ue, wide=wide, short=31 // S, mid=3 * ue, long=2048 // wide + 3 * ue,
                    per=16 // S)

    def steps(self, a, n):
        """L starts 16 elements apart from a: every value at every position."""
        starts = [a + 16 * m for m in range(self.L)]
        assert starts[-1] + n <= self.run_lo
        return starts

    def window_calls(self, D):
        """[(starts, window, doff)] on stream 0.  With window a multiple of the
        destination chunk every window of a call has the same cut: doff 1 gives
        a head of epc - 1 and a tail of 1, doff epc - 1 the reverse; 3 units'
        worth leaves the most rest chunks there can be."""
        sh = self.shapes(D)
        calls = []
        for a in range(sh["per"]):
            calls.append((self.steps(a, sh["short"]), sh["short"], 1))
            calls.append((self.steps(a, sh["mid"]), sh["mid"], 1))
            calls.append((self.steps(a, sh["mid"]), sh["mid"], sh["epc"] - 1))
            calls.append((self.steps(a, sh["long"]), sh["long"], 1))
        # into and inside the verbatim tail
        calls.append(([self.size - sh["mid"] - j for j in range(TAIL + 1)], sh["mid"], 1))
        calls.append(([self.size - 3, self.covered, self.covered + 1], 3, 0))
        return calls

    def set_calls(self, D):
        """[(ids, starts, window, doff)] over the set: the ends of the short
        streams, whose tails hold every value, and windows of stream 0."""
        sh = self.shapes(D)
        calls = []
        tails = list(range(1, self.nstreams))
        for n in (sh["mid"], TAIL, 1):
            for back in range(0, TAIL if n == 1 else 1):
                calls.append((tails, [self.small - n - back] * len(tails), n, 1))
        for a in (0, 1 % sh["per"]):
            starts = self.steps(a, sh["mid"])
            calls.append(([0] * len(starts), starts, sh["mid"], 1))
        calls.append(([0, 1, 0, 2], [5, 0, self.size - sh["mid"], self.small - sh["mid"]], sh["mid"], 0))
        return calls

    def aligned_and_shifted(self, D, doff=1):
        """Two source offsets (elements): with the destination `doff` elements
        behind a boundary, units that start on a source granule, and ones that
        do not."""
        sh = self.shapes(D)
        head = (-doff) % sh["epc"]
        a0 = (-head) % sh["per"]
        return a0, (a0 + 1) % sh["per"]

    def ragged_calls(self, D):
        """[(ids, starts, counts, max_window, pitch, doff)]: groups of L windows
        of one count each, 16 elements apart; counts that are multiples of the
        destination chunk keep the cut the same within a group when packed, and
        the short spans come last.  Both lane instantiations by max_window."""
        sh = self.shapes(D)
        a0, a1 = self.aligned_and_shifted(D)
        ids, starts, counts = [], [], []
        for a, n in ((a0, sh["mid"]), (a1, sh["mid"]), (a0, sh["short"])):
            st = self.steps(a, n)
            starts += st
            counts += [n] * len(st)
            ids += [0] * len(st)
        # the ends of the short streams (over a set), else of stream 0
        t_ids = list(range(1, self.nstreams))
        t_starts = [self.small - TAIL - 2] * len(t_ids)
        t_counts = [TAIL + 2] * len(t_ids)
        calls = []
        for max_window in (sh["mid"], sh["long"]):
            pitch = -(-max_window // sh["epc"]) * sh["epc"] + sh["epc"]
            for p in (0, pitch):
                calls.append((ids, starts, counts, max_window, p, 1))
        return calls, (t_ids, t_starts, t_counts)

    def tile_calls(self, D):
        """[(starts, rows, cols, pitch, doff)] on stream 0: L two-row tiles 16
        elements apart, cols a multiple of the destination chunk (every row of a
        call has the same cut), on each side of 1024 and 2048 bytes of the
        wider side; and rows short enough to go singly."""
        sh = self.shapes(D)
        a0, a1 = self.aligned_and_shifted(D)
        e16, e64 = 1024 // sh["wide"], 2048 // sh["wide"]
        calls = []
        for cols in (e16, e16 + 3 * sh["ue"], e64, e64 + 3 * sh["ue"]):
            pitch = cols + 16
            for a in (a0, a1):
                starts = self.steps(a, pitch + cols)
                calls.append((starts, 2, cols, pitch, 1))
        cols = sh["short"]
        calls.append((self.steps(0, 32 + cols), 2, cols, 32, 1))
        return calls

    # ---- coverage: {(value index, path)} of a call
    def cover_piece(self, D, i, start, n, dst_elem, into):
        paths = piece_paths(self.S, D, start, n, self.covered_of(i), dst_elem)
        for v, p in zip(self.idx[i][start:start + n].tolist(), paths):
            into.add((v, p))

    def cover_windows(self, D, ids, starts, window, doff, into):
        for k, (i, s) in enumerate(zip(ids, starts)):
            assert 0 <= s <= self.sizes[i] - window
            self.cover_piece(D, i, s, window, doff + k * window, into)

    def cover_ragged(self, D, ids, starts, counts, pitch, doff, into):
        at = 0
        for k, (i, s, n) in enumerate(zip(ids, starts, counts)):
            assert 0 <= s <= self.sizes[i] - n
            self.cover_piece(D, i, s, n, doff + (k * pitch if pitch else at), into)
            at += n

    def cover_tiles(self, D, ids, starts, rows, cols, pitch, doff, into):
        for k, (i, s) in enumerate(zip(ids, starts)):
            assert 0 <= s and s + (rows - 1) * pitch + cols <= self.sizes[i]
            for r in range(rows):
                self.cover_piece(D, i, s + r * pitch, cols, doff + (k * rows + r) * cols, into)

    def lanes_of_tiles(self, D, cols):
        lb = cols * max(self.S, D)
        return 16 if lb <= 1024 else 64 if lb <= 2048 else 256


_layouts = {}


def layout(src):
    if src not in _layouts:
        _layouts[src] = Layout(src)
    return _layouts[src]


def every_pair(lay, paths):
    return {(v, p) for v in range(lay.nv) for p in paths}


SUBSET = ["single", "unit-aligned", "unit-shifted", "tail"]   # what ragged and tile layouts must hold


def fold_shifted(cover):
    """{(value, path)} with the unit-shifted instantiations folded into one."""
    return {(v, "unit-shifted" if p.startswith("unit-shifted") else p) for v, p in cover}
