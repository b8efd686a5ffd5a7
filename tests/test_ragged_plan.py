"""The plan of the ragged window decode (bitshuffle_amd/csrc/window_plan.h,
ragged_plan / ragged_good, via libbshuf_hostcheck.so -- the function
k_ragged_plan runs per window on the device).

Exhaustive for small streams: block sizes 8, 16 and 64; sizes without a partial
block, with one, with a tail, and of fewer than 8 elements; element sizes 1, 2
and 3; every max_window from 1 to the stream's size, every count from -1 to
max_window + 1 and every start from -1 to one behind the last valid one.  The
plan is compared with a restatement in plain integer arithmetic and, for the
smallest block size, with an element-by-element one."""
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
    lib.bshuf_hostcheck_ragged_plan.restype = None
    lib.bshuf_hostcheck_ragged_plan.argtypes = ([ctypes.c_int64, I64P] + [ctypes.c_int64] * 4
                                                + [I64P, I64P, I64P, ctypes.c_int64, I64P])
    lib.bshuf_hostcheck_window_plan.restype = None
    lib.bshuf_hostcheck_window_plan.argtypes = [ctypes.c_int64] * 3 + [I64P, I64P, ctypes.c_int64, I64P]
    return lib


def _p(a):
    return a.ctypes.data_as(I64P)


def ragged(lib, nstreams, sizes, bs, E, max_window, Mw, ids, counts, starts):
    sizes = np.ascontiguousarray(sizes, dtype=np.int64)
    ids, counts, starts = (np.ascontiguousarray(a, dtype=np.int64) for a in (ids, counts, starts))
    out = np.empty((len(starts), 12), dtype=np.int64)
    lib.bshuf_hostcheck_ragged_plan(nstreams, _p(sizes), bs, E, max_window, Mw, _p(ids), _p(counts), _p(starts),
                                    len(starts), _p(out))
    return out


def fixed(lib, size, bs, E, window, starts):
    starts = np.ascontiguousarray(starts, dtype=np.int64)
    windows = np.full(len(starts), window, dtype=np.int64)
    out = np.empty((len(starts), 12), dtype=np.int64)
    lib.bshuf_hostcheck_window_plan(size, bs, E, _p(windows), _p(starts), len(starts), _p(out))
    return out


def blocks_of(size, bs):
    last = size % bs - size % 8
    nb = size // bs + (1 if last else 0)
    return nb, size // bs * bs + last, last


def window_blocks(size, bs, window):
    return min((window + bs - 2) // bs + 1, blocks_of(size, bs)[0])


def sizes_for(bs):
    """No partial block; a partial block; a partial block (when bs allows one) and a tail; < 8 elements."""
    n = 2 if bs < 64 else 1
    part = bs // 2 if bs > 8 else 0
    return sorted({(n + 1) * bs, n * bs + part, n * bs + part + 5, 5})


def rows_for(size, max_window):
    """Every (count, start): counts -1 .. max_window + 1, starts -1 .. size - count + 1."""
    cs, ss = [], []
    for count in range(-1, max_window + 2):
        s = np.arange(-1, max(size - max(count, 0), 0) + 2, dtype=np.int64)
        ss.append(s)
        cs.append(np.full(len(s), count, dtype=np.int64))
    return np.concatenate(cs), np.concatenate(ss)


def check(key, r, size, bs, E, max_window, Mw, counts, starts, known=None):
    """r against the restatement; returns the mask of good windows."""
    nb, covered, slast = blocks_of(size, bs)
    gMw, b0, nfull, last, bad, clip_lo, clip_n, tail_lo, tail_n, t0, t1, eff = r.T
    good = (counts >= 0) & (counts <= max_window) & (starts >= 0) & (starts <= size - counts)
    if known is not None:
        good &= known
    assert (gMw == Mw).all(), key
    assert (bad == (~good).astype(np.int64)).all(), key
    assert (eff == np.where(good, counts, 0)).all(), key
    # refused: b0 0, nothing to copy, no live block
    assert not r[~good][:, [1, 5, 6, 7, 8, 9, 10]].any(), key
    # the blocks decoded lie in the stream, or, a stream shorter than Mw blocks, are all of it
    m = min(Mw, nb)
    assert ((b0 >= 0) & (b0 + Mw <= max(nb, Mw))).all(), key
    assert (nfull + (last > 0) == m).all(), key
    ends = (b0 + m == nb) & (slast != 0) & (m > 0)
    assert (last == np.where(ends, slast, 0)).all(), key
    g = good
    c, s = counts[g], starts[g]
    end = s + c
    lo_c, hi_c = np.minimum(s, covered), np.minimum(end, covered)      # decoded part
    lo_t, hi_t = np.maximum(s, covered), np.maximum(end, covered)      # tail part
    # clip and tail span tile [start, start + count) exactly
    assert (clip_n[g] == (hi_c - lo_c) * E).all(), key
    assert (tail_n[g] == (hi_t - lo_t) * E).all(), key
    assert (clip_n[g] + tail_n[g] == c * E).all(), key
    has = clip_n[g] > 0
    assert (b0[g][has] * bs * E + clip_lo[g][has] == s[has] * E).all(), key
    assert (clip_lo[g][~has] == 0).all(), key
    hast = tail_n[g] > 0
    assert (covered * E + tail_lo[g][hast] == lo_t[hast] * E).all(), key
    # [t0, t1): exactly the blocks that hold clip bytes, inside [0, Mw) and inside the stream
    want_t0 = np.where(has, lo_c // bs - b0[g], 0)
    want_t1 = np.where(has, (hi_c - 1) // bs - b0[g] + 1, 0)
    assert (t0[g] == want_t0).all() and (t1[g] == want_t1).all(), key
    assert ((t0[g] >= 0) & (t0[g] <= t1[g]) & (t1[g] <= Mw)).all(), key
    assert (b0[g] + t1[g] <= nb).all(), key
    return good


@pytest.mark.parametrize("E", [1, 2, 3])
@pytest.mark.parametrize("bs", [8, 16, 64])
def test_every_max_window_count_and_start(lib, bs, E):
    for size in sizes_for(bs):
        for max_window in range(1, size + 1):
            Mw = window_blocks(size, bs, max_window)
            counts, starts = rows_for(size, max_window)
            r = ragged(lib, -1, [size], bs, E, max_window, Mw, np.zeros_like(counts), counts, starts)
            key = (size, bs, E, max_window)
            good = check(key, r, size, bs, E, max_window, Mw, counts, starts)
            assert good.any() and (~good).any(), key
            # count == max_window: every field is window_plan's
            full = counts == max_window
            f = fixed(lib, size, bs, E, max_window, starts[full])
            assert (f[:, :11] == r[full][:, :11]).all(), key


@pytest.mark.parametrize("E", [1, 3])
def test_element_by_element(lib, E):
    """bs = 8: the clip's and the tail span's bytes, taken from a stream whose byte
    i holds i, are the window's; the live blocks are those an element lies in."""
    bs = 8
    for size in (5, 16, 29):
        nb, covered, _ = blocks_of(size, bs)
        stream = np.arange(size * E)
        for max_window in range(1, size + 1):
            Mw = window_blocks(size, bs, max_window)
            counts, starts = rows_for(size, max_window)
            r = ragged(lib, -1, [size], bs, E, max_window, Mw, np.zeros_like(counts), counts, starts)
            for row, c, s in zip(r.tolist(), counts.tolist(), starts.tolist()):
                _, b0, nfull, last, bad, clip_lo, clip_n, tail_lo, tail_n, t0, t1, _ = row
                if bad:
                    continue
                staged = stream[b0 * bs * E:min(b0 + Mw, nb) * bs * E][:(nfull * bs + last) * E]
                got = np.concatenate([staged[clip_lo:clip_lo + clip_n],
                                      stream[covered * E:][tail_lo:tail_lo + tail_n]])
                assert got.tolist() == stream[s * E:(s + c) * E].tolist(), (size, E, max_window, c, s)
                live = sorted({e // bs - b0 for e in range(s, s + c) if e < covered})
                assert live == list(range(t0, t1)), (size, E, max_window, c, s)


@pytest.mark.parametrize("bs", [8, 16])
def test_streams_of_a_set_with_fewer_blocks_than_mw(lib, bs):
    """Mw comes from the set's largest stream; a stream with fewer blocks plans
    good, from block 0 on, with no live block at or behind its last one."""
    E = 2
    big = 6 * bs + 5
    seen_short = False
    for small in range(0, 3 * bs):
        nb = blocks_of(small, bs)[0]
        for max_window in (1, bs, bs + 1, 2 * bs + 3, 4 * bs, big):
            Mw = window_blocks(big, bs, max_window)
            counts, starts = rows_for(small, min(max_window, small + 1))
            for sid in (0, 1, 2, -1, 3):
                ids = np.full(len(counts), sid, dtype=np.int64)
                r = ragged(lib, 3, [small, big, small], bs, E, max_window, Mw, ids, counts, starts)
                known = np.full(len(counts), sid in (0, 1, 2))
                size = big if sid == 1 else (small if sid in (0, 2) else 0)
                key = (small, bs, max_window, sid)
                good = check(key, r, size, bs, E, max_window, Mw, counts, starts, known)
                if sid in (0, 2) and nb < Mw:
                    assert (r[good][:, 1] == 0).all(), key              # b0
                    assert (r[good][:, 10] <= nb).all(), key            # t1
                    assert (r[good][:, 2] + (r[good][:, 3] > 0) == nb).all(), key
                    seen_short = seen_short or bool((r[good][:, 6] > 0).any())
                if sid in (-1, 3):
                    assert not good.any(), key
    assert seen_short
