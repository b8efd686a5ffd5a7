"""The plan of the window decode over a set of streams
(bitshuffle_amd/csrc/window_plan.h, window_set_plan, via libbshuf_hostcheck.so --
the function k_window_plan runs per window of a set on the device) and the host side
of bshuf_lz4_stream_set_dev and bshuf_decompress_lz4_windows_set_dev.

The plan, for every stream size up to four blocks, every forced block count Mw
from 1 to 4, every window length that can need Mw blocks and every start from
one before the first valid one to one behind the last, at ids inside and
outside the set: a window is flagged bad exactly when its id is outside the
set, it is longer than its stream, its start is out of range or its stream has
fewer than Mw blocks; a good window decodes Mw consecutive blocks of its
stream, its decoded elements are one contiguous clip of them, the rest a span
of the verbatim tail, and the two together are exactly [start, start + window)."""
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
    lib.bshuf_hostcheck_window_set_plan.restype = None
    lib.bshuf_hostcheck_window_set_plan.argtypes = ([ctypes.c_int64, I64P] + [ctypes.c_int64] * 3
                                                    + [I64P, I64P, I64P, ctypes.c_int64, I64P])
    lib.bshuf_hostcheck_window_plan.restype = None
    lib.bshuf_hostcheck_window_plan.argtypes = [ctypes.c_int64] * 3 + [I64P, I64P, ctypes.c_int64, I64P]
    return lib


def _p(a):
    return a.ctypes.data_as(I64P)


def set_plans(lib, sizes, bs, E, Mw, ids, windows, starts):
    sizes = np.ascontiguousarray(sizes, dtype=np.int64)
    ids, windows, starts = (np.ascontiguousarray(a, dtype=np.int64) for a in (ids, windows, starts))
    out = np.empty((len(starts), 12), dtype=np.int64)
    lib.bshuf_hostcheck_window_set_plan(len(sizes), _p(sizes), bs, E, Mw, _p(ids), _p(windows), _p(starts),
                                        len(starts), _p(out))
    return out


def one_plans(lib, size, bs, E, windows, starts):
    windows, starts = (np.ascontiguousarray(a, dtype=np.int64) for a in (windows, starts))
    out = np.empty((len(starts), 12), dtype=np.int64)
    lib.bshuf_hostcheck_window_plan(size, bs, E, _p(windows), _p(starts), len(starts), _p(out))
    return out


def blocks_of(size, bs):
    last = size % bs - size % 8
    nb = size // bs + (1 if last else 0)
    return nb, size // bs * bs + last, last


def cases(size, bs, Mw):
    """(id, window, start) of a three-stream set whose streams 0 and 2 have `size` elements,
    for every window length of which a call can have Mw = min(M, nb_max) blocks per window:
    M == Mw, or M > Mw = nb_max, and then no stream has more than Mw blocks."""
    nb = blocks_of(size, bs)[0]
    rows = []
    for window in range(1, size + 2):                       # size + 1: longer than the stream
        M = (window + bs - 2) // bs + 1
        if M < Mw or (M > Mw and nb > Mw):
            continue
        for start in range(-1, max(size - window, 0) + 2):
            rows.append((0, window, start))
        for i in (-1, 2, 3):
            for start in sorted({-1, 0, max(size - window, 0), max(size - window, 0) + 1}):
                rows.append((i, window, start))
    return rows


@pytest.mark.parametrize("E", [1, 3])
@pytest.mark.parametrize("bs", [8, 16])
def test_set_plan_every_size_block_count_window_start_and_id(lib, bs, E):
    other = 4 * bs - 1
    for size in range(0, 4 * bs):
        nb, covered, last_s = blocks_of(size, bs)
        for Mw in range(1, 5):
            rows = cases(size, bs, Mw)
            if not rows:
                continue
            ids, ws, ss = (np.array(c, dtype=np.int64) for c in zip(*rows))
            r = set_plans(lib, [size, other, size], bs, E, Mw, ids, ws, ss)
            gMw, b0, nfull, last, bad, clip_lo, clip_n, tail_lo, tail_n, t0, t1, _ = r.T
            key = (size, bs, E, Mw)
            assert (gMw == Mw).all(), key
            # bad: exactly these four reasons
            want_bad = (ids < 0) | (ids >= 3) | (ws > size) | (ss < 0) | (ss > size - ws) | (nb < Mw)
            assert (bad == want_bad.astype(np.int64)).all(), key
            assert not r[want_bad][:, [1, 5, 6, 7, 8, 9, 10]].any(), key    # b0 0, nothing to copy
            g = ~want_bad
            if not g.any():
                continue
            ws, ss, b0, nfull, last = ws[g], ss[g], b0[g], nfull[g], last[g]
            clip_lo, clip_n, tail_lo, tail_n, t0, t1 = clip_lo[g], clip_n[g], tail_lo[g], tail_n[g], t0[g], t1[g]
            # Mw consecutive blocks inside the stream, the partial block only as the stream's last
            assert ((b0 >= 0) & (b0 + Mw <= nb)).all(), key
            assert (b0 == np.minimum(ss // bs, nb - Mw)).all(), key
            assert (nfull + (last != 0) == Mw).all(), key
            assert (last == np.where((b0 + Mw == nb) & (last_s != 0), last_s, 0)).all(), key
            # whole elements
            for a in (clip_lo, clip_n, tail_lo, tail_n):
                assert (a % E == 0).all() and (a >= 0).all(), key
            ce, te = clip_n // E, tail_n // E
            # the clip lies inside the Mw decoded blocks and inside the blocks' elements
            assert (clip_lo + clip_n <= (nfull * bs + last) * E).all(), key
            first = b0 * bs + clip_lo // E
            assert (first[ce > 0] == ss[ce > 0]).all() and (first + ce <= covered)[ce > 0].all(), key
            # clip plus tail span is [start, start + window)
            assert (ce + te == ws).all(), key
            assert (ce == np.clip(np.minimum(ss + ws, covered) - ss, 0, None)).all(), key
            tfirst = covered + tail_lo // E
            assert (tfirst[te > 0] == (ss + ce)[te > 0]).all() and (tfirst + te <= size)[te > 0].all(), key
            # [t0, t1): exactly the decoded blocks that hold clip elements
            want_t0 = np.where(ce > 0, ss // bs - b0, 0)
            want_t1 = np.where(ce > 0, (ss + ce - 1) // bs - b0 + 1, 0)
            assert (t0 == want_t0).all() and (t1 == want_t1).all(), key
            assert ((t0 >= 0) & (t1 <= Mw)).all(), key


@pytest.mark.parametrize("E", [1, 3])
def test_set_plan_against_a_model_in_elements(lib, E):
    """The same, element by element as lists (block size 8)."""
    bs = 8
    for size in range(0, 4 * bs):
        nb, covered, last_s = blocks_of(size, bs)
        for Mw in range(1, 5):
            rows = cases(size, bs, Mw)
            if not rows:
                continue
            ids, ws, ss = zip(*rows)
            r = set_plans(lib, [size, 4 * bs - 1, size], bs, E, Mw, ids, ws, ss)
            for (i, window, start), row in zip(rows, r.tolist()):
                _, b0, nfull, last, bad, clip_lo, clip_n, tail_lo, tail_n, t0, t1, _ = row
                key = (size, E, Mw, i, window, start)
                good = 0 <= i < 3 and window <= size and 0 <= start <= size - window and nb >= Mw
                assert bad == int(not good), key
                if bad:
                    assert (b0, clip_n, tail_n, t0, t1) == (0, 0, 0, 0, 0), key
                    continue
                elems = list(range(start, start + window))
                decoded = list(range(b0 * bs, b0 * bs + nfull * bs + last))
                assert decoded and decoded[-1] < covered and len(decoded) == (Mw * bs if not last
                                                                               else (Mw - 1) * bs + last_s), key
                f = b0 * bs + clip_lo // E
                clip = list(range(f, f + clip_n // E)) if clip_n else []
                tail = list(range(covered + tail_lo // E, covered + (tail_lo + tail_n) // E))
                assert clip == [e for e in elems if e < covered], key
                assert tail == [e for e in elems if e >= covered], key
                assert all(e in decoded for e in clip[:1] + clip[-1:]), key
                assert all(covered <= e < size for e in tail), key
                if clip:
                    assert (t0, t1) == (clip[0] // bs - b0, clip[-1] // bs - b0 + 1), key
                else:
                    assert t0 == t1 == 0, key


def test_set_plan_far_starts_and_ids(lib):
    """Starts and ids far outside are flagged without overflow."""
    sizes = [1000, 300]
    far = (-2 ** 62, 2 ** 62, 2 ** 63 - 1, -2 ** 63)
    for v in far:
        for ids, starts in (([0], [v]), ([v], [0]), ([v], [v])):
            row = set_plans(lib, sizes, 64, 2, 3, ids, [100], starts)[0].tolist()
            assert row[4] == 1 and row[1] == 0 and row[6] == 0 and row[8] == 0, (v, ids, starts)
    # the nearest ones that are fine
    row = set_plans(lib, sizes, 64, 2, 3, [1], [100], [200])[0].tolist()
    assert row[4] == 0 and row[6] + row[8] == 200


@pytest.mark.parametrize("E", [1, 3])
@pytest.mark.parametrize("bs", [8, 16])
def test_set_plan_is_the_window_plan_of_the_stream(lib, bs, E):
    """With Mw = min(M, blocks of the stream) the rows are bshuf_hostcheck_window_plan's."""
    for size in range(1, 4 * bs):
        nb = blocks_of(size, bs)[0]
        for window in range(1, size + 1):
            Mw = min((window + bs - 2) // bs + 1, nb)
            starts = list(range(-1, size - window + 2))
            ws = [window] * len(starts)
            a = set_plans(lib, [4 * bs - 1, size], bs, E, Mw, [1] * len(starts), ws, starts)
            b = one_plans(lib, size, bs, E, ws, starts)
            assert (b[:, 0] == Mw).all()
            assert a.tolist() == b.tolist(), (size, bs, E, window)


# ---- the C entry points, before the device is touched -------------------------

def _sizes(vals):
    arr = (ctypes.c_size_t * len(vals))(*vals)
    return ctypes.cast(arr, ctypes.c_void_p), arr


def _build(B, nbytes, sizes, E, block, set_ptr=256, set_bytes=None, ws=None, ws_bytes=0):
    pn, k1 = _sizes(nbytes)
    ps, k2 = _sizes(sizes)
    pin, k3 = _sizes([0] * len(sizes))
    if set_bytes is None:
        set_bytes = B.lib.bshuf_lz4_stream_set_dev_bytes(ps, len(sizes), E, block)
    return B.lib.bshuf_lz4_stream_set_dev(pin, pn, ps, len(sizes), E, block, None, set_ptr, set_bytes, ws,
                                          ws_bytes, None, None)


def _decode(B, count, max_size, E, block, K, window, set_ptr=256, ws=None, ws_bytes=0):
    return B.lib.bshuf_decompress_lz4_windows_set_dev(set_ptr, count, max_size, E, block, None, None, K, window,
                                                      None, ws, ws_bytes, None, None, None)


NB, SZ = [5000, 300, 7000], [10000, 5, 12000]


def test_set_host_errors_before_device():
    import bitshuffle_amd as B
    pn, k1 = _sizes(NB)
    ps, k2 = _sizes(SZ)
    nset = B.lib.bshuf_lz4_stream_set_dev_bytes(ps, 3, 2, 0)
    need = B.lib.bshuf_lz4_stream_set_dev_workspace(pn, ps, 3, 2, 0)
    assert nset > 0 and nset % 256 == 0 and need > 0 and need % 256 == 0
    # header, three 64-byte records, an index of 2 + 0 + 2 blocks
    assert nset >= 256 + 3 * 64 + 4 * 8
    assert _build(B, NB, SZ, 2, 12) == -81
    assert _build(B, NB, SZ, 2, 98304) == -71                          # above the LDS decoder's size
    assert _build(B, NB, SZ, 2, 0, set_bytes=nset - 1) == -71          # set too small
    assert _build(B, NB, SZ, 2, 0, set_ptr=256 + 16) == -71            # ... not 256-byte aligned
    assert _build(B, NB, SZ, 2, 0, set_ptr=None) == -71
    assert _build(B, NB, SZ, 2, 0, ws=256, ws_bytes=need - 1) == -71   # workspace too small
    assert _build(B, NB, SZ, 2, 0, ws=256 + 16, ws_bytes=need + 256) == -71
    # 2^31 blocks in all overflow the 32-bit work-block indexes
    huge = [2 ** 33, 2 ** 33]
    assert _build(B, [100, 100], huge, 1, 8, set_bytes=1 << 40) == -71
    hs, k3 = _sizes(huge)
    hn, k4 = _sizes([100, 100])
    # the size functions report the same refusals as 0
    assert B.lib.bshuf_lz4_stream_set_dev_bytes(hs, 2, 1, 8) == 0
    assert B.lib.bshuf_lz4_stream_set_dev_workspace(hn, hs, 2, 1, 8) == 0
    assert B.lib.bshuf_lz4_stream_set_dev_bytes(ps, 3, 2, 12) == 0
    assert B.lib.bshuf_lz4_stream_set_dev_bytes(ps, 3, 2, 98304) == 0
    assert B.lib.bshuf_lz4_stream_set_dev_workspace(pn, ps, 3, 2, 12) == 0
    assert B.lib.bshuf_lz4_stream_set_dev_workspace(pn, ps, 3, 2, 98304) == 0
    # an empty set is a set
    assert B.lib.bshuf_lz4_stream_set_dev_bytes(None, 0, 2, 0) >= 256


def test_windows_set_host_errors_before_device():
    import bitshuffle_amd as B
    f = B.lib.bshuf_decompress_lz4_windows_set_dev_workspace
    need = f(12000, 2, 0, 16, 100)
    assert need > 0
    assert _decode(B, 3, 12000, 2, 12, 16, 100) == -81
    assert _decode(B, 3, 12000, 2, 0, 16, 12001) == -71                       # window > max_size
    assert _decode(B, 3, 12000, 2, 0, 2 ** 31, 100) == -71                    # nwindows * M >= 2^31
    assert _decode(B, 3, 2 ** 24, 2, 0, 2 ** 20, 4096 * 2 ** 11) == -71       # 2^20 * 2049
    assert _decode(B, 3, 10 ** 6, 2, 98304, 16, 100) == -71                   # above the LDS decoder's size
    assert _decode(B, 3, 12000, 2, 0, 16, 100, ws=256, ws_bytes=need - 1) == -71
    assert _decode(B, 3, 12000, 2, 0, 16, 100, ws=256 + 16, ws_bytes=need + 256) == -71
    assert _decode(B, 3, 12000, 2, 0, 16, 100, set_ptr=256 + 16) == -71
    assert _decode(B, 3, 12000, 2, 0, 16, 100, set_ptr=None) == -71
    assert _decode(B, 2 ** 31, 12000, 2, 0, 16, 100) == -71
    assert f(12000, 2, 12, 16, 100) == 0
    assert f(12000, 2, 0, 16, 12001) == 0
    assert f(10 ** 6, 2, 98304, 16, 100) == 0
    assert f(12000, 2, 0, 2 ** 31, 100) == 0


def test_set_valid_arguments_need_a_device():
    import bitshuffle_amd as B
    if B.using_HIP():
        pytest.skip("HIP device present")
    pn, k1 = _sizes(NB)
    ps, k2 = _sizes(SZ)
    need = B.lib.bshuf_lz4_stream_set_dev_workspace(pn, ps, 3, 2, 0)
    assert _build(B, NB, SZ, 2, 0) == -70
    assert _build(B, NB, SZ, 2, 0, ws=256, ws_bytes=need) == -70
    assert _build(B, [], [], 2, 0) == -70
    need = B.lib.bshuf_decompress_lz4_windows_set_dev_workspace(12000, 2, 0, 16, 100)
    assert _decode(B, 3, 12000, 2, 0, 16, 100) == -70
    assert _decode(B, 3, 12000, 2, 0, 16, 100, ws=256, ws_bytes=need) == -70
    assert _decode(B, 3, 12000, 2, 0, 0, 100) == -70
    assert _decode(B, 0, 0, 2, 0, 4, 0) == -70


def test_windows_set_workspace_depends_on_the_shape_alone():
    import bitshuffle_amd as B
    f = B.lib.bshuf_decompress_lz4_windows_set_dev_workspace
    size = 10 ** 6
    prev = 0
    for K in (1, 2, 3, 16, 257, 4096):
        n = f(size, 2, 0, K, 5000)
        assert n > 0 and n >= prev and n % 256 == 0, K
        prev = n
    prev = 0
    for window in (1, 2, 4095, 4096, 4097, 4098, 8192, 65536, size):
        n = f(size, 2, 0, 64, window)
        assert n > 0 and n >= prev, window
        prev = n
    bs = B.default_block_size(2)
    # K staging areas of Mw blocks and K token-position areas are part of it
    assert f(size, 2, 0, 64, 4098) >= 64 * 3 * bs * 2 + 64 * 4 * (3 * (4 + 2 * bs) // 3 + 80)
    # Mw is capped by the largest stream's blocks, and by nothing else of the set:
    # the function takes no stream count, no stream lengths and no ids or starts
    assert f(2 * bs, 2, 0, 64, 2 * bs) == f(2 * bs + 7, 2, 0, 64, 2 * bs) < f(3 * bs, 2, 0, 64, 2 * bs)
    assert f(size, 2, 0, 64, 4098) == f(size + 12345, 2, 0, 64, 4098)
    # the set's size grows with the streams' block counts (in 256-byte steps)
    a, _k1 = _sizes([1000, 5])
    b, _k2 = _sizes([1000, 10 ** 6])
    assert 0 < B.lib.bshuf_lz4_stream_set_dev_bytes(a, 2, 2, 0) < B.lib.bshuf_lz4_stream_set_dev_bytes(b, 2, 2, 0)
