"""The shape and the plan of the tile decode (bitshuffle_amd/csrc/tile_plan.h via
libbshuf_hostcheck.so -- tile_shape on the host, tile_group per (tile, group) in
k_tile_plan, tile_row per row in k_tile_gather) and the host side of
bshuf_decompress_lz4_tiles_dev and bshuf_decompress_lz4_tiles_set_dev.

The shape against a brute-force minimum over every rg.  The plan against a model:
an identity array is put into simulated staging areas following the group plans,
every row is gathered by its tile_row fields and compared with slicing, for every
start from two before the stream to two behind it."""
import ctypes
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOSTCHECK = os.path.join(ROOT, "bitshuffle_amd", "libbshuf_hostcheck.so")

I64 = ctypes.c_int64
I64P = ctypes.POINTER(ctypes.c_int64)


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(HOSTCHECK):
        import subprocess
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "bitshuffle_amd"), HOSTCHECK])
    lib = ctypes.CDLL(HOSTCHECK)
    lib.bshuf_hostcheck_tile_shape.restype = None
    lib.bshuf_hostcheck_tile_shape.argtypes = [I64] * 5 + [I64P]
    lib.bshuf_hostcheck_tile_rows.restype = ctypes.c_int
    lib.bshuf_hostcheck_tile_rows.argtypes = [I64, I64P, I64, I64] + [I64] * 7 + [I64P, I64P]
    lib.bshuf_hostcheck_window_plan.restype = None
    lib.bshuf_hostcheck_window_plan.argtypes = [I64] * 3 + [I64P, I64P, I64, I64P]
    lib.bshuf_hostcheck_window_set_plan.restype = None
    lib.bshuf_hostcheck_window_set_plan.argtypes = ([I64, I64P] + [I64] * 3 + [I64P, I64P, I64P, I64, I64P])
    return lib


def _p(a):
    return a.ctypes.data_as(I64P)


def shape(lib, rows, cols, pitch, bs, nb):
    out = np.empty(3, dtype=np.int64)
    lib.bshuf_hostcheck_tile_shape(rows, cols, pitch, bs, nb, _p(out))
    return tuple(out.tolist())


def run_blocks(W, bs):
    return (W + bs - 2) // bs + 1


def brute_shape(rows, cols, pitch, bs, nb):
    best = None
    for rg in range(1, rows + 1):
        G = -(-rows // rg)
        Mg = min(run_blocks((rg - 1) * pitch + cols, bs), nb)
        if best is None or G * Mg <= best[0]:       # ties: the larger rg
            best = (G * Mg, rg, G, Mg)
    return best[1:]


def blocks_of(size, bs):
    last = size % bs - size % 8
    nb = size // bs + (1 if last else 0)
    return nb, size // bs * bs + last, last


def tile(lib, sizes, bs, E, rows, cols, pitch, nb, start, id=0, ref=-1, one=True):
    """(bad, groups (G, 6), rows (rows, 8)) of one tile; one: of the one stream sizes[0]."""
    rg, G, Mg = shape(lib, rows, cols, pitch, bs, nb)
    sizes = np.ascontiguousarray(sizes, dtype=np.int64)
    groups = np.full((G, 6), -7, dtype=np.int64)
    rws = np.full((rows, 8), -7, dtype=np.int64)
    bad = lib.bshuf_hostcheck_tile_rows(-1 if one else len(sizes), _p(sizes), id, ref, bs, E, rows, cols, pitch,
                                        nb, start, _p(groups), _p(rws))
    return bad, groups, rws


# ---- the shape ------------------------------------------------------------------

@pytest.mark.parametrize("bs", [8, 16, 64])
def test_shape_is_the_brute_force_minimum(lib, bs):
    n = 0
    for rows in range(1, 13):
        for cols in (1, 3, 8, 20, 64, 100):
            for pitch in range(cols, 6 * bs + cols, 3):
                uncapped = run_blocks((rows - 1) * pitch + cols, bs)
                # blocks of the stream: far more than any run, a cap in the middle of the
                # search, a cap on everything but single rows, and very few
                for nb in sorted({10 ** 6, uncapped, max(uncapped // 2, 1), run_blocks(cols, bs), 2, 1}):
                    got = shape(lib, rows, cols, pitch, bs, nb)
                    assert got == brute_shape(rows, cols, pitch, bs, nb), (bs, rows, cols, pitch, nb)
                    n += 1
    assert n > 5000


def test_shape_reference_points(lib):
    big = 10 ** 6
    assert shape(lib, 3, 8, 100, 64, big) == (3, 1, 5)
    assert shape(lib, 3, 8, 256, 64, big) == (1, 3, 2)
    assert shape(lib, 7, 8, 117, 64, big) == (2, 4, 3)
    # an rg between a window per row and one run: 18 blocks against 24 and 23
    assert shape(lib, 12, 3, 123, 64, big) == (2, 6, 3)
    assert [-(-12 // rg) * run_blocks((rg - 1) * 123 + 3, 64) for rg in (2, 1, 12)] == [18, 24, 23]
    # the measured cases: images of 2048 int16 per row in 4096-element blocks, wide float32 rows
    assert shape(lib, 256, 256, 2048, 4096, 1024) == (256, 1, 129)
    assert shape(lib, 256, 256, 16384, 2048, big) == (1, 256, 2)
    # a stream without blocks: one group of nothing
    assert shape(lib, 5, 2, 3, 64, 0) == (5, 1, 0)


# ---- the plan against a model ----------------------------------------------------

SHAPES = [(1, 5, 5), (1, 1, 1), (3, 2, 5), (3, 3, 3), (4, 1, 9), (2, 8, 17), (5, 3, 4), (3, 2, 16), (2, 20, 23),
          (7, 1, 6), (3, 5, 33), (3, 2, 40), (5, 2, 36), (7, 1, 33)]


def sizes_of(bs):
    for nfull in range(4):
        for part in (0, 8):
            for tail in (0, 5):
                yield nfull * bs + part + tail
    # ... and streams long enough for tiles of several groups (pitches above two blocks)
    yield 15 * bs
    yield 15 * bs + 8 + 5


@pytest.mark.parametrize("E", [1, 2, 3])
def test_rows_gathered_from_simulated_areas_are_the_slices(lib, E):
    bs = 16
    seen_good = seen_tail = seen_groups = 0
    for size in sizes_of(bs):
        nb, covered, last_s = blocks_of(size, bs)
        ident = np.arange(size * E, dtype=np.int64)
        tail = ident[covered * E:]
        for rows, cols, pitch in SHAPES:
            span = (rows - 1) * pitch + cols
            rg, G, Mg = shape(lib, rows, cols, pitch, bs, nb)
            assert (rg, G, Mg) == brute_shape(rows, cols, pitch, bs, nb)
            for start in range(-2, size + 3):
                key = (size, E, rows, cols, pitch, start)
                bad, groups, rws = tile(lib, [size], bs, E, rows, cols, pitch, nb, start)
                want_bad = span > size or start < 0 or start > size - span
                assert bad == int(want_bad), key
                assert (groups[:, 4] == bad).all() and (groups[:, 0] == 0).all(), key
                # every group: Mg consecutive blocks inside the stream, the partial one only as its last
                b0, nfull, last = groups[:, 1], groups[:, 2], groups[:, 3]
                assert ((b0 >= 0) & (b0 + Mg <= nb)).all(), key
                assert (nfull + (last != 0) == Mg).all(), key
                assert (last == np.where((b0 + Mg == nb) & (last_s != 0) & (Mg > 0), last_s, 0)).all(), key
                if bad:
                    assert not rws.any() and not b0.any(), key      # nothing to copy, blocks [0, Mg)
                    continue
                seen_good += 1
                seen_groups += G > 1
                areas = []
                for g in range(G):
                    a = np.full(Mg * bs * E, -1, dtype=np.int64)
                    n = (nfull[g] * bs + last[g]) * E
                    a[:n] = ident[b0[g] * bs * E:b0[g] * bs * E + n]
                    areas.append(a)
                    assert b0[g] == min((start + g * rg * pitch) // bs, nb - Mg), key
                for r in range(rows):
                    g, lo, n, tlo, tn, t0, t1, _ = rws[r].tolist()
                    assert g == r // rg and n % E == 0 and tn % E == 0 and n >= 0 and tn >= 0, key
                    # every read lies inside [0, Mg * bs * E) of the row's area, and inside the tail
                    assert 0 <= lo and lo + n <= Mg * bs * E, key
                    assert 0 <= tlo and tlo + tn <= tail.size, key
                    got = np.concatenate([areas[g][lo:lo + n], tail[tlo:tlo + tn]])
                    s = start + r * pitch
                    assert got.tolist() == list(range(s * E, (s + cols) * E)), key + (r,)
                    # [t0, t1): exactly the group's blocks that hold the row's clip
                    if n:
                        e = s + n // E
                        assert (t0, t1) == (s // bs - b0[g], (e - 1) // bs - b0[g] + 1), key
                        assert 0 <= t0 < t1 <= Mg, key
                    else:
                        assert t0 == t1 == 0, key
                    seen_tail += tn > 0
    assert seen_good > 1000 and seen_tail > 100 and seen_groups > 100


def test_far_starts_are_bad_without_overflow(lib):
    for v in (-2 ** 62, 2 ** 62, 2 ** 63 - 1, -2 ** 63):
        bad, groups, rws = tile(lib, [1000], 64, 2, 3, 8, 100, 16, v)
        assert bad == 1 and not rws.any() and not groups[:, 1].any()


# ---- over a set -------------------------------------------------------------------

def test_set_rules_give_a_bad_tile_on_ref(lib):
    bs, E = 16, 2
    sizes = [6 * bs + 8 + 5, 3 * bs, 5, 9 * bs]         # 7, 3, 0 and 9 blocks
    ref, nb_max = 3, 9
    rows, cols, pitch = 3, 4, 20                        # span 44: one group of four blocks
    span = (rows - 1) * pitch + cols
    rg, G, Mg = shape(lib, rows, cols, pitch, bs, nb_max)
    assert (rg, G, Mg) == (3, 1, 4)

    def one(i, start):
        return tile(lib, sizes, bs, E, rows, cols, pitch, nb_max, start, id=i, ref=ref, one=False)

    for i in (-1, 4, 2 ** 40, -2 ** 63):                # id outside the set
        bad, groups, rws = one(i, 0)
        assert bad == 1 and groups[0].tolist() == [ref, 0, Mg, 0, 1, 0] and not rws.any()
    bad, groups, rws = one(2, 0)                        # span above the stream's size
    assert bad == 1 and groups[0, 0] == ref and not rws.any()
    assert span <= sizes[1]
    bad, groups, rws = one(1, 0)                        # fewer than Mg blocks
    assert bad == 1 and groups[0, 0] == ref and not rws.any()
    for i in (0, 3):                                    # the streams that take the tile: every start
        nb, covered, _ = blocks_of(sizes[i], bs)
        for start in range(-2, sizes[i] + 3):
            bad, groups, rws = one(i, start)
            good = 0 <= start <= sizes[i] - span
            assert bad == int(not good), (i, start)
            if not good:
                assert groups[0].tolist()[:2] == [ref, 0] and groups[0, 4] == 1 and not rws.any()
                continue
            # ... the one-stream plan of that stream with Mg forced by the set's largest stream
            assert groups[0, 0] == i and groups[0, 1] == min(start // bs, nb - Mg)
            for r in range(rows):
                g, lo, n, tlo, tn, t0, t1, _ = rws[r].tolist()
                s = start + r * pitch
                first = groups[0, 1] * bs + lo // E
                assert n // E + tn // E == cols
                assert (first == s or n == 0) and first + n // E <= covered
                assert tn == 0 or covered + tlo // E == s + n // E
    # no stream to serve a bad tile (a mismatched header): none
    bad, groups, rws = tile(lib, sizes, bs, E, rows, cols, pitch, nb_max, 0, id=7, ref=-1, one=False)
    assert bad == 1 and groups[0].tolist() == [-1, 0, Mg, 0, 1, 0]


@pytest.mark.parametrize("E", [1, 3])
@pytest.mark.parametrize("bs", [8, 16])
def test_one_row_is_the_window_plan(lib, bs, E):
    """rows == 1: one group, and group and row together are window_plan's /
    window_set_plan's window of cols elements, row for row."""
    for size in range(1, 4 * bs, 1 if bs == 8 else 5):
        nb = blocks_of(size, bs)[0]
        other = 4 * bs - 1
        for window in range(1, size + 1):
            starts = np.arange(-1, size - window + 2, dtype=np.int64)
            ws = np.full(len(starts), window, dtype=np.int64)
            want = np.empty((len(starts), 12), dtype=np.int64)
            lib.bshuf_hostcheck_window_plan(size, bs, E, _p(ws), _p(starts), len(starts), _p(want))
            Mw = int(want[0, 0])
            assert shape(lib, 1, window, window, bs, nb) == (1, 1, Mw)
            # over a set whose largest stream has the same Mw
            sizes = np.array([other, size], dtype=np.int64)
            nb_max = blocks_of(other, bs)[0]
            set_Mw = min(run_blocks(window, bs), nb_max)
            swant = np.empty((len(starts), 12), dtype=np.int64)
            ids = np.ones(len(starts), dtype=np.int64)
            lib.bshuf_hostcheck_window_set_plan(2, _p(sizes), bs, E, set_Mw, _p(ids), _p(ws), _p(starts),
                                                len(starts), _p(swant))
            for k, start in enumerate(starts.tolist()):
                for one, w, nbs in ((True, want[k], nb), (False, swant[k], nb_max)):
                    bad, groups, rws = tile(lib, [size] if one else sizes, bs, E, 1, window, window, nbs, start,
                                            id=1, ref=0, one=one)
                    key = (size, window, start, one)
                    assert bad == w[4], key
                    if bad:
                        assert not rws.any()
                        continue
                    assert groups[0, 1:5].tolist() == w[1:5].tolist(), key            # b0, nfull, last, bad
                    assert rws[0].tolist() == [0] + w[5:11].tolist() + [0], key       # clip, tail span, t0, t1


# ---- the C entry points, before the device is touched -------------------------------

def _one(B, size, E, block, K, rows, cols, pitch, in_nbytes=10 ** 6, ws=None, ws_bytes=0):
    return B.lib.bshuf_decompress_lz4_tiles_dev(256, in_nbytes, size, E, block, None, K, rows, cols, pitch, None,
                                                ws, ws_bytes, None, None, None, None)


def _set(B, count, max_size, E, block, K, rows, cols, pitch, set_ptr=256, ws=None, ws_bytes=0):
    return B.lib.bshuf_decompress_lz4_tiles_set_dev(set_ptr, count, max_size, E, block, None, None, K, rows, cols,
                                                    pitch, None, ws, ws_bytes, None, None, None)


def test_tiles_host_errors_before_device():
    import bitshuffle_amd as B
    f = B.lib.bshuf_decompress_lz4_tiles_dev_workspace
    fs = B.lib.bshuf_decompress_lz4_tiles_set_dev_workspace
    size = 2048 * 2048
    need = f(10 ** 6, size, 2, 0, 16, 256, 256, 2048)
    sneed = fs(size, 2, 0, 16, 256, 256, 2048)
    assert need > 0 and need % 256 == 0 and sneed > 0 and sneed % 256 == 0
    assert _one(B, size, 2, 12, 16, 256, 256, 2048) == -81
    assert _set(B, 3, size, 2, 12, 16, 256, 256, 2048) == -81
    for call, sizer in ((lambda *a, **k: _one(B, size, 2, 0, *a, **k), lambda *a: f(10 ** 6, size, 2, 0, *a)),
                        (lambda *a, **k: _set(B, 3, size, 2, 0, *a, **k), lambda *a: fs(size, 2, 0, *a))):
        assert call(16, 256, 256, 255) == -71                            # pitch < cols
        assert call(16, 2049, 256, 2048) == -71                          # span > size
        assert call(16, 2, 256, 2 ** 63) == -71                          # ... without overflow
        assert call(16, 2 ** 40, 2 ** 40, 2 ** 40) == -71
        assert call(2 ** 31, 1, 8, 8) == -71                             # ntiles * G >= 2^31
        assert call(2 ** 23, 256, 1, 16384) == -71                       # 2^23 tiles of 256 groups
        assert call(2 ** 24, 256, 256, 2048) == -71                      # ntiles * G * Mg >= 2^31
        n = sizer(16, 256, 256, 2048)
        assert call(16, 256, 256, 2048, ws=256, ws_bytes=n - 1) == -71   # workspace too small
        assert call(16, 256, 256, 2048, ws=256 + 16, ws_bytes=n + 256) == -71
        assert sizer(16, 256, 256, 255) == 0 and sizer(16, 2049, 256, 2048) == 0
        assert sizer(2 ** 24, 256, 256, 2048) == 0
    assert _one(B, 10 ** 6, 2, 98304, 16, 4, 4, 100) == -71              # above the LDS decoder's size
    assert _set(B, 3, 10 ** 6, 2, 98304, 16, 4, 4, 100) == -71
    assert f(10 ** 6, 10 ** 6, 2, 98304, 16, 4, 4, 100) == 0 and f(10 ** 6, size, 2, 12, 16, 4, 4, 100) == 0
    assert _set(B, 3, size, 2, 0, 16, 256, 256, 2048, set_ptr=256 + 16) == -71
    assert _set(B, 3, size, 2, 0, 16, 256, 256, 2048, set_ptr=None) == -71
    assert _set(B, 2 ** 31, size, 2, 0, 16, 256, 256, 2048) == -71


def test_tiles_valid_arguments_need_a_device():
    import bitshuffle_amd as B
    if B.using_HIP():
        pytest.skip("HIP device present")
    size = 2048 * 2048
    need = B.lib.bshuf_decompress_lz4_tiles_dev_workspace(10 ** 6, size, 2, 0, 16, 256, 256, 2048)
    assert _one(B, size, 2, 0, 16, 256, 256, 2048) == -70
    assert _one(B, size, 2, 0, 16, 256, 256, 2048, ws=256, ws_bytes=need) == -70
    assert _set(B, 3, size, 2, 0, 16, 256, 256, 2048) == -70
    for K, rows, cols in ((0, 4, 4), (4, 0, 4), (4, 4, 0)):             # nothing to decode still needs one
        assert _one(B, size, 2, 0, K, rows, cols, 2048) == -70
        assert _set(B, 3, size, 2, 0, K, rows, cols, 2048) == -70


def test_tiles_workspace_depends_on_the_shape_alone():
    import bitshuffle_amd as B
    f = B.lib.bshuf_decompress_lz4_tiles_dev_workspace
    fs = B.lib.bshuf_decompress_lz4_tiles_set_dev_workspace
    size = 2048 * 2048
    prev = 0
    for K in (1, 2, 3, 16, 257, 1024):
        n = fs(size, 2, 0, K, 256, 256, 2048)
        assert n > 0 and n >= prev and n % 256 == 0, K
        prev = n
    bs = B.default_block_size(2)
    assert bs == 4096
    # one group of 129 blocks per 256 x 256 tile of a 2048-wide int16 image, against the 512
    # blocks of 256 windows: staging areas and token positions of a quarter the size
    per_tile = 129 * bs * 2
    assert 64 * per_tile <= fs(size, 2, 0, 64, 256, 256, 2048) < 64 * 3 * per_tile
    wins = B.lib.bshuf_decompress_lz4_windows_set_dev_workspace(size, 2, 0, 64 * 256, 256)
    assert fs(size, 2, 0, 64, 256, 256, 2048) < wins / 3
    # rows a window each (pitch of four blocks): the windows' staging areas, fewer tables
    assert fs(size, 2, 0, 64, 128, 256, 16384) <= B.lib.bshuf_decompress_lz4_windows_set_dev_workspace(
        size, 2, 0, 64 * 128, 256)
    # Mg is capped by the largest stream's blocks
    assert fs(2 * bs, 2, 0, 8, 2, bs, bs) == fs(2 * bs + 7, 2, 0, 8, 2, bs, bs) < fs(3 * bs, 2, 0, 8, 2, bs, bs)
    assert f(10 ** 6, size, 2, 0, 64, 256, 256, 2048) > 0


def test_long_thin_tiles_need_no_search(lib):
    """pitch <= bs: the one run is the minimum whatever the rows, and the shape is there
    at once -- also for a tile of 10^9 rows of one element (pitch == cols)."""
    import time
    import bitshuffle_amd as B
    for bs in (8, 16, 64):
        for rows in range(1, 30):
            for cols in (1, 2, 7, 8, 9, 63, 64):
                for pitch in range(cols, bs + 1):
                    for nb in (1, 2, 5, 10 ** 6):
                        assert shape(lib, rows, cols, pitch, bs, nb) == brute_shape(rows, cols, pitch, bs, nb)
                        assert shape(lib, rows, cols, pitch, bs, nb)[0] == rows
    t0 = time.perf_counter()
    assert shape(lib, 10 ** 9, 1, 1, 4096, 10 ** 7) == (10 ** 9, 1, run_blocks(10 ** 9, 4096))
    assert shape(lib, 10 ** 9, 3, 4096, 4096, 10 ** 12)[:2] == (10 ** 9, 1)
    assert B.lib.bshuf_decompress_lz4_tiles_dev_workspace(10 ** 6, 2 * 10 ** 9, 1, 0, 1, 10 ** 9, 1, 1) > 0
    assert time.perf_counter() - t0 < 0.5


def test_lane_variants_are_accepted_and_their_own():
    """The values that force the gather's lanes per row (kTileLanes16 / 64 / 256) are taken
    by bshuf_set_variant, and are none of the encoder's and decoder's."""
    import bitshuffle_amd as B
    try:
        for v in (1 << 22, 1 << 23, (1 << 22) | (1 << 23)):
            assert B.lib.bshuf_set_variant(v) == 0, v
        assert B.lib.bshuf_set_variant(0x3000) == -71
    finally:
        assert B.lib.bshuf_set_variant(0) == 0
