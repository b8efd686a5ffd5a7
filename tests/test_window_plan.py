"""The plan of the window decode (bitshuffle_amd/csrc/window_plan.h via
libbshuf_hostcheck.so -- the function k_window_plan runs per window on the
device) and the host side of bshuf_decompress_lz4_windows_dev.

The plan, for every stream size up to three blocks, a partial block and a
tail, every window length and every start from one before the first valid one
to one behind the last: every window of a call decodes the same number of
consecutive blocks; its decoded elements are one contiguous clip of them, the
rest a span of the verbatim tail, and the two together are exactly
[start, start + window); out-of-range starts are flagged and get nothing."""
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
    lib.bshuf_hostcheck_window_plan.restype = None
    lib.bshuf_hostcheck_window_plan.argtypes = [ctypes.c_int64] * 3 + [I64P, I64P, ctypes.c_int64, I64P]
    return lib


def plans(lib, size, bs, E, windows, starts):
    windows = np.ascontiguousarray(windows, dtype=np.int64)
    starts = np.ascontiguousarray(starts, dtype=np.int64)
    out = np.empty((len(starts), 12), dtype=np.int64)
    p = lambda a: a.ctypes.data_as(I64P)  # noqa: E731
    lib.bshuf_hostcheck_window_plan(size, bs, E, p(windows), p(starts), len(starts), p(out))
    return out


def model(size, bs, window, start):
    """The plan in elements: (Mw, b0, nfull, last, bad, clip elements, tail-span elements)."""
    nfull_s, last_s = size // bs, size % bs - size % 8
    nb, covered = nfull_s + (1 if last_s else 0), nfull_s * bs + last_s
    Mw = min((window + bs - 2) // bs + 1, nb)
    bad = start < 0 or start > size - window
    b0 = 0 if bad else max(0, min(start // bs, nb - Mw))
    ends = Mw > 0 and b0 + Mw == nb and last_s != 0
    elems = [] if bad else list(range(start, start + window))
    return (Mw, b0, Mw - 1 if ends else Mw, last_s if ends else 0, int(bad),
            [e for e in elems if e < covered], [e for e in elems if e >= covered])


@pytest.mark.parametrize("E", [1, 3])
@pytest.mark.parametrize("bs", [8, 16])
def test_window_plan_every_size_window_and_start(lib, bs, E):
    for size in range(0, 3 * bs + bs):
        nfull_s, last_s = size // bs, size % bs - size % 8
        nb, covered = nfull_s + (1 if last_s else 0), nfull_s * bs + last_s
        ws, ss = [], []
        for window in range(1, size + 1):
            for start in range(-1, size - window + 2):
                ws.append(window)
                ss.append(start)
        if not ws:
            continue
        r = plans(lib, size, bs, E, ws, ss)
        for (window, start, row) in zip(ws, ss, r.tolist()):
            Mw, b0, nfull, last, bad, clip_lo, clip_n, tail_lo, tail_n, t0, t1, _ = row
            key = (size, bs, E, window, start)
            mMw, mb0, mnfull, mlast, mbad, mclip, mtail = model(size, bs, window, start)
            # the same number of blocks for every start, inside the stream
            assert Mw == mMw == min((window + bs - 2) // bs + 1, nb), key
            assert 0 <= b0 and b0 + Mw <= nb and b0 == mb0, key
            assert (nfull, last) == (mnfull, mlast), key
            assert nfull + (1 if last else 0) == Mw, key
            assert bad == mbad == int(start in (-1, size - window + 1)), key
            if bad:
                assert (b0, clip_n, tail_n, t0, t1) == (0, 0, 0, 0, 0), key
                continue
            # the clip lies inside the Mw decoded blocks, whole elements of them
            decoded = nfull * bs + last
            assert clip_lo % E == 0 and clip_n % E == 0 and tail_lo % E == 0 and tail_n % E == 0, key
            assert 0 <= clip_lo and clip_lo + clip_n <= decoded * E, key
            first = b0 * bs + clip_lo // E
            clip = list(range(first, first + clip_n // E)) if clip_n else []
            tail = list(range(covered + tail_lo // E, covered + (tail_lo + tail_n) // E))
            assert all(e < covered for e in clip) and all(covered <= e < size for e in tail), key
            assert clip == mclip and tail == mtail, key
            assert clip + tail == list(range(start, start + window)), key
            # [t0, t1): exactly the decoded blocks that hold clip elements
            if clip:
                assert (t0, t1) == (clip[0] // bs - b0, clip[-1] // bs - b0 + 1), key
                assert 0 <= t0 < t1 <= Mw, key
            else:
                assert t0 == t1 == 0, key


def test_window_plan_far_starts(lib):
    """Starts far outside the array are flagged without overflow."""
    for start in (-2 ** 62, -5, 2 ** 62, 2 ** 63 - 1):
        row = plans(lib, 1000, 64, 2, [100], [start])[0].tolist()
        assert row[4] == 1 and row[1] == 0 and row[6] == 0 and row[8] == 0


# ---- the C entry points, before the device is touched -------------------------

def _call(B, in_nbytes, size, E, block, K, window, ws=None, ws_bytes=0):
    return B.lib.bshuf_decompress_lz4_windows_dev(None, in_nbytes, size, E, block, None, K, window, None,
                                                  ws, ws_bytes, None, None, None, None)


def test_windows_host_errors_before_device():
    import bitshuffle_amd as B
    need = B.lib.bshuf_decompress_lz4_windows_dev_workspace(5000, 10000, 2, 0, 16, 100)
    assert need > 0
    assert _call(B, 5000, 10000, 2, 12, 16, 100) == -81
    assert _call(B, 5000, 10000, 2, 0, 16, 10001) == -71                     # window > size
    assert _call(B, 5000, 10000, 2, 0, 2 ** 31, 100) == -71                  # nwindows * M >= 2^31
    assert _call(B, 5000, 2 ** 24, 2, 0, 2 ** 20, 4096 * 2 ** 11) == -71   # 2^20 * 2049
    assert _call(B, 5000, 10 ** 6, 2, 98304, 16, 100) == -71                 # above the LDS decoder's size
    assert _call(B, 5000, 10000, 2, 0, 16, 100, 256, need - 1) == -71        # workspace too small
    assert _call(B, 5000, 10000, 2, 0, 16, 100, 256 + 16, need + 256) == -71  # ... not 256-byte aligned
    # the workspace function reports the same refusals as 0
    assert B.lib.bshuf_decompress_lz4_windows_dev_workspace(5000, 10000, 2, 0, 16, 10001) == 0
    assert B.lib.bshuf_decompress_lz4_windows_dev_workspace(5000, 10 ** 6, 2, 98304, 16, 100) == 0


def test_windows_valid_arguments_need_a_device():
    import bitshuffle_amd as B
    if B.using_HIP():
        pytest.skip("HIP device present")
    need = B.lib.bshuf_decompress_lz4_windows_dev_workspace(5000, 10000, 2, 0, 16, 100)
    assert _call(B, 5000, 10000, 2, 0, 16, 100) == -70
    assert _call(B, 5000, 10000, 2, 0, 16, 100, 256, need) == -70
    assert _call(B, 5000, 10000, 2, 0, 0, 100) == -70


def test_windows_workspace_grows_with_the_call():
    import bitshuffle_amd as B
    f = B.lib.bshuf_decompress_lz4_windows_dev_workspace
    size, nbytes = 10 ** 6, 10 ** 6
    prev = 0
    for K in (1, 2, 3, 16, 257, 4096):
        n = f(nbytes, size, 2, 0, K, 5000)
        assert n > 0 and n >= prev and n % 256 == 0, K
        prev = n
    prev = 0
    for window in (1, 2, 4095, 4096, 4097, 4098, 8192, 65536, size):
        n = f(nbytes, size, 2, 0, 64, window)
        assert n > 0 and n >= prev, window
        prev = n
    # the size does not depend on anything but the call's shape: K staging
    # areas of Mw blocks are part of it
    bs = B.default_block_size(2)
    assert f(nbytes, size, 2, 0, 64, 4098) >= 64 * 3 * bs * 2
