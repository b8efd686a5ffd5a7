"""The converting gathers' span cut (bitshuffle_amd/csrc/cvt_span.h,
cvt_span_plan, through libbshuf_hostcheck.so) against an element-by-element
restatement: span_cvt (window_copy.h) walks a span of n source elements of S
bytes exactly as simulated here -- head elements singly, units of whole source
granules that become whole 16-byte chunks of the destination, rest chunks from
single loads, tail elements singly.  For every source byte offset 0..15 that an
S-byte element can have, every destination offset 0..15 that a D-byte element
can have, S in {1, 2, 4}, D in {2, 4} and n in 0..80:

* every destination byte of the span is written exactly once, none outside it,
  and element i of the source is the one that lands in element i;
* 16-byte stores are 16-byte aligned and cover only whole chunks of the span;
* every 16-byte source granule that is read holds a byte of the span."""
import ctypes
import os

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SO = os.path.join(HERE, "..", "bitshuffle_amd", "libbshuf_hostcheck.so")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(SO):
        import bitshuffle_amd._lib as L
        L.build()
    h = ctypes.CDLL(SO)
    h.bshuf_hostcheck_cvt_span.argtypes = [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_int, ctypes.c_int,
                                           ctypes.c_int64, ctypes.POINTER(ctypes.c_int64)]
    h.bshuf_hostcheck_cvt_span.restype = None
    return h


def plan(lib, src, dst, S, D, n):
    out = (ctypes.c_int64 * 6)()
    lib.bshuf_hostcheck_cvt_span(src, dst, S, D, n, out)
    return dict(zip(("head", "nu", "nc", "tail", "ue", "r"), out))


def walk(p, src, dst, S, D, n):
    """span_cvt's accesses for plan p.  Returns (writes, granules): writes maps
    a destination byte address to the source element it comes from, each byte
    written once; granules is the set of 16-byte source granule numbers read.
    `stores16`: the addresses of the 16-byte stores."""
    writes, granules, stores16 = {}, set(), []
    epc = 16 // D

    def put(e, wide):
        for b in range(D):
            a = dst + e * D + b
            assert a not in writes, "destination byte %d written twice" % a
            writes[a] = e
        if not wide:
            # a single load of one S-aligned element
            lo = src + e * S
            assert lo % S == 0
            granules.add(lo // 16)
            assert (lo + S - 1) // 16 == lo // 16

    for e in range(p["head"]):
        put(e, False)
    if p["head"] == n:
        assert p["nu"] == p["nc"] == p["tail"] == 0
        return writes, granules, stores16
    s = src + p["head"] * S          # where the units' source starts
    d = dst + p["head"] * D
    assert d % 16 == 0
    assert p["r"] == s % 16
    ue = p["ue"]
    assert ue == max(16 // S, 16 // D)
    G, NC = ue * S // 16, ue * D // 16
    assert G * 16 == ue * S and NC * 16 == ue * D
    q = s // 16                      # the aligned granule the units start in
    for u in range(p["nu"]):
        for j in range(G + (1 if p["r"] else 0)):
            granules.add(q + u * G + j)
        for k in range(ue):
            put(p["head"] + u * ue + k, True)
        for c in range(NC):
            stores16.append(d + (u * NC + c) * 16)
    e0 = p["nu"] * ue
    assert p["nc"] < NC or p["nc"] == 0
    for c in range(p["nc"]):
        for k in range(epc):
            e = p["head"] + e0 + c * epc + k
            put(e, False)
        stores16.append(d + (e0 + c * epc) * D)
    e1 = e0 + p["nc"] * epc
    assert p["tail"] < epc
    for k in range(p["tail"]):
        put(p["head"] + e1 + k, False)
    assert p["head"] + e1 + p["tail"] == n
    return writes, granules, stores16


@pytest.mark.parametrize("D", [2, 4])
@pytest.mark.parametrize("S", [1, 2, 4])
def test_every_offset_and_length(lib, S, D):
    base_s, base_d = 0x1000, 0x8000
    for so in range(0, 16, S):
        for do in range(0, 16, D):
            for n in range(0, 81):
                src, dst = base_s + so, base_d + do
                p = plan(lib, src, dst, S, D, n)
                writes, granules, stores16 = walk(p, src, dst, S, D, n)
                what = "S %d D %d src+%d dst+%d n %d: %r" % (S, D, so, do, n, p)
                # every byte of the span once (walk asserts "at most once"), none outside
                assert sorted(writes) == list(range(dst, dst + n * D)), what
                for a, e in writes.items():
                    assert e == (a - dst) // D, what
                # whole aligned chunks only
                for a in stores16:
                    assert a % 16 == 0 and dst <= a and a + 16 <= dst + n * D, what
                # every granule read holds a byte of the span
                for g in granules:
                    assert g * 16 < src + n * S and g * 16 + 16 > src, what
                # fewer than 32 source bytes go singly; else whole chunks wherever one fits
                if n * S < 32:
                    assert p["head"] == n and not stores16, what
                else:
                    first = (dst + 15) // 16 * 16
                    last = (dst + n * D) // 16 * 16
                    assert sorted(stores16) == list(range(first, last, 16)), what
                    assert p["head"] == (first - dst) // D and p["tail"] == (dst + n * D - last) // D, what


def test_source_offsets_outside_the_element_grid_are_not_planned_wrong(lib):
    """Only the low four bits of the two addresses matter."""
    for S, D in ((1, 4), (2, 2), (4, 2)):
        for n in (0, 7, 33, 80):
            a = plan(lib, 0x10 + 4, 0x20 + 8, S, D, n)
            b = plan(lib, 0xABC0 + 4, 0x7770 + 8, S, D, n)
            assert a == b
