"""The piece plan of the range decode (bitshuffle_amd/csrc/range_plan.h via
libbshuf_hostcheck.so): for every stream size up to three blocks and a tail,
and every range of it, the pieces -- head edge, interior blocks, tail edge,
tail span -- cover each element of the range exactly once and nothing else,
go to the dense destination offsets, and have the shape the kernels rely on:
interior blocks whole, at most two edge blocks with a proper clip, the tail
span inside the verbatim tail."""
import ctypes
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOSTCHECK = os.path.join(ROOT, "bitshuffle_amd", "libbshuf_hostcheck.so")

I64P = ctypes.POINTER(ctypes.c_int64)


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(HOSTCHECK):
        import subprocess
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "bitshuffle_amd"), HOSTCHECK])
    lib = ctypes.CDLL(HOSTCHECK)
    lib.bshuf_hostcheck_range_pieces.restype = None
    lib.bshuf_hostcheck_range_pieces.argtypes = [ctypes.c_int64] * 6 + [I64P]
    lib.bshuf_hostcheck_range_pieces_n.restype = None
    lib.bshuf_hostcheck_range_pieces_n.argtypes = [ctypes.c_int64] * 3 + [I64P] * 3 + [ctypes.c_int64, I64P]
    return lib


def pieces_n(lib, size, bs, E, starts, counts, dst0):
    n = len(starts)
    out = np.empty((n, 14), dtype=np.int64)
    p = lambda a: a.ctypes.data_as(I64P)  # noqa: E731
    lib.bshuf_hostcheck_range_pieces_n(size, bs, E, p(starts), p(counts), p(dst0), n, p(out))
    return out


def all_ranges(size):
    """Every (start, count) with start + count <= size."""
    starts = np.repeat(np.arange(size + 1), np.arange(size + 1, 0, -1))
    first = np.cumsum(np.arange(size + 1, 0, -1)) - np.arange(size + 1, 0, -1)
    counts = np.arange(len(starts)) - first[starts]
    return starts.astype(np.int64), counts.astype(np.int64)


def layout(size, bs):
    nfull = size // bs
    last = size % bs - size % 8
    return nfull, last, nfull * bs + last


@pytest.mark.parametrize("E", [1, 3])
@pytest.mark.parametrize("bs", [8, 16, 128])
def test_pieces_cover_every_range_exactly(lib, bs, E):
    for size in range(3 * bs + 8):
        nfull, last, covered = layout(size, bs)
        nb = nfull + (1 if last else 0)
        starts, counts = all_ranges(size)
        assert int((starts + counts).max()) == size and len(starts) == (size + 1) * (size + 2) // 2
        dst0 = (starts * 7 + counts * 3) % 41  # some byte offset of the output per range
        r = pieces_n(lib, size, bs, E, starts, counts, dst0)
        b0, b1, idst = r[:, 0], r[:, 1], r[:, 2]
        hb, hlo, hhi, hdst = r[:, 3], r[:, 4], r[:, 5], r[:, 6]
        tb, tlo, thi, tdst = r[:, 7], r[:, 8], r[:, 9], r[:, 10]
        slo, sn, sdst = r[:, 11], r[:, 12], r[:, 13]
        has_h, has_t, has_i, has_s = hhi > hlo, thi > tlo, b1 > b0, sn > 0
        # shape: clips inside their block, a proper part of it; interior blocks exist
        blk_m = lambda b: np.where(b < nfull, bs, last)  # noqa: E731
        for has, b, lo, hi in ((has_h, hb, hlo, hhi), (has_t, tb, tlo, thi)):
            assert np.all(~has | ((b >= 0) & (b < nb)))
            assert np.all(~has | ((lo >= 0) & (hi <= blk_m(b))))
            assert np.all(~has | (hi - lo < blk_m(b))), "an edge block covered whole"
            assert np.all(has | (hi == lo))
        assert np.all(b1 >= b0) and np.all(~has_i | ((b0 >= 0) & (b1 <= nb)))
        assert np.all(~(has_h & has_t) | (hb < tb)), "one block as two edges"
        assert np.all(~(has_h & has_i) | (hb == b0 - 1)) and np.all(~(has_t & has_i) | (tb == b1))
        # the tail span lies in the verbatim tail [covered, size)
        assert np.all(sn >= 0) and np.all(~has_s | ((slo >= 0) & (slo + sn <= size - covered)))
        # the pieces as element intervals, in order: each begins where the one
        # before it ended, the first at `start`, the last ends at start + count
        # -- every element of the range once, none outside it -- and each goes
        # to the dense offset of its first element
        iv = (
            (has_h, hb * bs + hlo, hhi - hlo, hdst),
            (has_i, b0 * bs, np.minimum(b1 * bs, covered) - b0 * bs, idst),
            (has_t, tb * bs + tlo, thi - tlo, tdst),
            (has_s, covered + slo, sn, sdst),
        )
        cur = starts.copy()
        for has, a, n, dst in iv:
            assert np.all(~has | (n > 0))
            assert np.all(~has | (a == cur)), (size, bs)
            assert np.all(~has | (dst == dst0 + (a - starts) * E)), (size, bs)
            cur = cur + np.where(has, n, 0)
        assert np.all(cur == starts + counts), (size, bs)


@pytest.mark.parametrize("bs,E", [(8, 1), (16, 3)])
def test_pieces_element_by_element(lib, bs, E):
    """The same property counted element by element, one call per range."""
    out = (ctypes.c_int64 * 14)()
    for size in range(3 * bs + 8):
        nfull, last, covered = layout(size, bs)
        for start in range(size + 1):
            for count in range(size - start + 1):
                lib.bshuf_hostcheck_range_pieces(size, bs, E, start, count, 5, out)
                hits = np.zeros(size, dtype=np.int64)
                dst = np.full(size, -1, dtype=np.int64)

                def mark(a, n, d):
                    hits[a:a + n] += 1
                    dst[a:a + n] = d + E * np.arange(n)
                b0, b1 = out[0], out[1]
                if b1 > b0:
                    mark(b0 * bs, min(b1 * bs, covered) - b0 * bs, out[2])
                for o in (3, 7):
                    if out[o + 2] > out[o + 1]:
                        mark(out[o] * bs + out[o + 1], out[o + 2] - out[o + 1], out[o + 3])
                if out[12] > 0:
                    mark(covered + out[11], out[12], out[13])
                want = np.zeros(size, dtype=np.int64)
                want[start:start + count] = 1
                assert np.array_equal(hits, want), (size, start, count)
                assert np.array_equal(dst[start:start + count], 5 + E * np.arange(count))
