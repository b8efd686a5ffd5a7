"""The launchers' path decisions (bitshuffle_amd/csrc/dispatch.h via
libbshuf_hostcheck.so) against their restatement tests/dispatch_model.py, and
the cells of the GPU sweep (tests/dispatch_cases.py) against the model: every
path the model can name is reached by a cell, at two or more element sizes
wherever the rule admits two."""
import ctypes
import os

import pytest

from tests import dispatch_cases as C
from tests import dispatch_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOSTCHECK = os.path.join(ROOT, "bitshuffle_amd", "libbshuf_hostcheck.so")
I64P = ctypes.POINTER(ctypes.c_int64)
I64 = ctypes.c_int64


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(HOSTCHECK):
        import subprocess
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "bitshuffle_amd"), HOSTCHECK])
    lib = ctypes.CDLL(HOSTCHECK)
    lib.bshuf_hostcheck_dispatch_consts.restype = None
    lib.bshuf_hostcheck_dispatch_consts.argtypes = [I64P]
    lib.bshuf_hostcheck_dispatch_reg_groups.argtypes = [ctypes.c_int, ctypes.c_int]
    lib.bshuf_hostcheck_dispatch_encode.restype = None
    lib.bshuf_hostcheck_dispatch_encode.argtypes = [ctypes.c_int, I64, I64, I64P, ctypes.c_int, I64P]
    lib.bshuf_hostcheck_dispatch_decode.restype = None
    lib.bshuf_hostcheck_dispatch_decode.argtypes = [ctypes.c_int, I64, I64P, ctypes.c_int, ctypes.c_int,
                                                    ctypes.c_int, I64P]
    lib.bshuf_hostcheck_dispatch_residues.restype = None
    lib.bshuf_hostcheck_dispatch_residues.argtypes = [ctypes.c_int, I64, I64, ctypes.c_int, ctypes.c_int, I64P]
    lib.bshuf_hostcheck_dispatch_pairs.restype = None
    lib.bshuf_hostcheck_dispatch_pairs.argtypes = [ctypes.c_int, I64, I64P]
    lib.bshuf_hostcheck_dispatch_transpose.argtypes = [ctypes.c_int, I64, I64]
    lib.bshuf_hostcheck_dispatch_rows16.argtypes = [ctypes.c_int, ctypes.c_int]
    return lib


BASE = 0x7F0000001000  # a 16-aligned address


def _addrs(residues):
    return (I64 * len(residues))(*[BASE + 0x1000 * i + r for i, r in enumerate(residues)])


ENC_KEYS = ("ek", "raw8", "desc", "wide", "wide_last", "large", "lds", "desc_off", "fast", "sreg")
DEC_KEYS = ("large", "ek", "stage_off", "lds", "cap")


def _row(enc, dec):
    return [int(enc[k]) for k in ENC_KEYS] + [int(dec[k]) for k in DEC_KEYS]


def host_residues(lib, E, nbytes, last, inplace=1, grec=0):
    """Rows of 15 words (the encoder's 10, the decoder's 5), one per residue."""
    out = (I64 * (16 * 15))()
    lib.bshuf_hostcheck_dispatch_residues(E, nbytes, last, inplace, grec, out)
    return [list(out[15 * r:15 * r + 15]) for r in range(16)]


def model_residues(E, nbytes, last, inplace=True, grec=False):
    return [_row(M.enc_launch(E, nbytes, last, (r,)), M.dec_launch(E, nbytes, (r,), inplace, grec))
            for r in range(16)]


def test_constants(lib):
    out = (I64 * len(M.CONST_ORDER))()
    lib.bshuf_hostcheck_dispatch_consts(out)
    for name, v in zip(M.CONST_ORDER, out):
        mine = getattr(M, name)
        assert (mine() if callable(mine) else mine) == int(v), name
    for ek in (0, 1, 2, 4, 8):
        assert lib.bshuf_hostcheck_dispatch_reg_groups(ek, 0) == M.reg_groups(ek), ek
        assert lib.bshuf_hostcheck_dispatch_reg_groups(ek, 1) == M.reg_groups4(ek), ek
    assert M.max_lds_decode_bytes() <= M.max_device_block_bytes() < M.LDS_BYTES


def _grid_sizes(E):
    """Every threshold rounded to E's groups, one group below and one above."""
    out = set()
    for T in [M.TABLE_BYTES] + [n for _, n in C.class_sizes(E)]:
        n = C.at_most(T, E)
        out |= {max(n - 8 * E, 8 * E), n, n + 8 * E}
    return sorted(n for n in out if n <= (2 ** 31 - 1) // 2)


GRID_E = list(range(1, 65)) + [1024]


def test_model_agrees_with_hostcheck_single(lib):
    """E in 1..64 and 1024, every threshold -8E / exact / +8E, all 16
    residues of the pointer; a partial block of none, one group and nearly a
    whole block's; the decoder's A/B variants' LDS budgets."""
    checked = 0
    for E in GRID_E:
        for n in _grid_sizes(E):
            for last in (0, 8 * E, C.partial_groups(n // (8 * E)) * 8 * E):
                assert host_residues(lib, E, n, last) == model_residues(E, n, last), (E, n, last)
                checked += 16
            for inplace, grec in ((0, 0), (0, 1)):
                assert host_residues(lib, E, n, 0, inplace, grec) == \
                    model_residues(E, n, 0, bool(inplace), bool(grec)), (E, n, inplace, grec)
    assert checked > 16 * 65 * 20 * 3


def test_model_agrees_with_hostcheck_batches_and_transposes(lib):
    """Batches of two residues (all 256 pairs); both residues of a transpose;
    the row rule of a tile."""
    out = (I64 * (256 * 15))()
    for E in GRID_E:
        sizes = [C.at_most(T, E) for T in (64, M.RAW_BYTES, M.TABLE_BYTES, M.FAST_MAX_BLOCK_BYTES,
                                           M.max_lds_decode_bytes())]
        for n in sizes if E <= 16 else sizes[1:3]:
            lib.bshuf_hostcheck_dispatch_pairs(E, n, out)
            for r in range(256):
                rs = (r // 16, r % 16)
                assert list(out[15 * r:15 * r + 15]) == \
                    _row(M.enc_launch(E, n, 0, rs), M.dec_launch(E, n, rs)), (E, n, rs)
        for r in range(256):
            assert bool(lib.bshuf_hostcheck_dispatch_transpose(E, BASE + r // 16, 2 * BASE + r % 16)) == \
                M.transpose_fast(E, r // 16, r % 16), (E, r)
    for P in list(range(1, 70)) + [255, 256, 257, 272, 512, 1023, 1024]:
        for ng in range(1, min(P, M.TILE_GROUPS) + 1):
            assert bool(lib.bshuf_hostcheck_dispatch_rows16(P, ng)) == M.rows16(P, ng), (P, ng)


# ---- the cell list reaches every path ----------------------------------------------
def _add(seen, paths, E):
    for p in paths:
        if p is not None:
            seen.setdefault(p, set()).add(E)


def _entry_paths(Es, sizes_of, partials_of, residues, batch_residues):
    """{entry: {path: set of E}} over element sizes Es, block bytes
    sizes_of(E), stream lengths partials_of(E, n) and pointer residues."""
    seen = {k: {} for k in ("exact", "fast", "decode", "shuf", "unshuf", "batch_exact", "batch_fast",
                            "batch_decode")}
    for E in Es:
        for n in sizes_of(E):
            bs = n // E
            for nelem in partials_of(E, n):
                # (the encoders' paths follow the data pointer alone, the
                # decoder's the decoded data's, which sits at the data offset)
                for ri in sorted({ri for ri, _ in residues}):
                    _add(seen["exact"], M.encode(E, bs, nelem, ri, 0), E)
                    _add(seen["decode"], M.decode(E, bs, nelem, 0, ri), E)
                    if n <= C.above(M.FAST_MAX_BLOCK_BYTES, E):
                        _add(seen["fast"], M.encode(E, bs, nelem, ri, 0, fast=True), E)
                for ri, ro in residues:
                    _add(seen["shuf"], M.transpose(E, bs, nelem, ri, ro, "shuf"), E)
                    _add(seen["unshuf"], M.transpose(E, bs, nelem, ri, ro, "unshuf"), E)
                for rs in batch_residues:
                    for key, fast in (("batch_exact", False), ("batch_fast", True)):
                        if fast and n > C.above(M.FAST_MAX_BLOCK_BYTES, E):
                            continue
                        state, per = M.encode_batch(E, bs, [nelem] * len(rs), rs, fast)
                        for pair in per:
                            _add(seen[key], [state + " " + p for p in pair if p], E)
                    state, per = M.decode_batch(E, bs, [nelem] * len(rs), rs)
                    for pair in per:
                        _add(seen["batch_decode"], [state + " " + p for p in pair if p], E)
    return seen


def _cell_lengths(E, n):
    return [nelem for _, nelem in C.streams(E, n)]


def _cell_paths():
    seen = _entry_paths(C.ELEM_SIZES, lambda E: [n for _, n in C.classes(E)], _cell_lengths, C.OFFSETS,
                        C.BATCH_RESIDUES)
    for E in C.ELEM_SIZES:  # the transposes' extra blocks
        for _, bs in C.transpose_extra_blocks():
            for ri, ro in C.OFFSETS:
                for what in ("shuf", "unshuf"):
                    _add(seen[what], M.transpose(E, bs, C.stream_elems(E, bs * E), ri, ro, what), E)
    return seen


def _universe_paths():
    """Every path the model names: element sizes up to 24 (every rule's
    classes: 1, the other register-transpose sizes, the rest), every threshold
    -8E / exact / +8E, partial blocks of 1, 3, 4 and 16 groups and nearly whole,
    all residues a pointer pair or a batch of three can differ by."""
    def lengths(E, n):
        bs = n // E
        P = bs // 8
        return sorted({3 * bs + 8 * g + 5 for g in (1, 3, 4, 16, C.partial_groups(P), P - 1) if 0 <= g < P})
    residues = [(a, b) for a in (0, 8, 4, 1) for b in (0, 8, 4, 1)]
    batches = [(0, 8, 1), (0, 8, 8), (0, 0, 0), (0, 0, 4), (8, 8, 8), (1, 1, 1)]

    def sizes(E):
        return _grid_sizes(E) + [(M.TILE_GROUPS + 16) * 8 * E, (M.TILE_GROUPS + 13) * 8 * E, 16 * 8 * E]
    return _entry_paths(list(range(1, 13)) + [16, 24], sizes, lengths, residues, batches)


def test_cells_reach_every_path():
    cells, universe = _cell_paths(), _universe_paths()
    missing, thin = [], []
    for entry, paths in universe.items():
        assert paths, entry
        for p, Es in sorted(paths.items()):
            got = cells[entry].get(p, set())
            if not got:
                missing.append((entry, p, sorted(Es)[:6]))
            elif len(Es) >= 2 and len(got) < 2:
                thin.append((entry, p, sorted(got), sorted(Es)[:6]))
    assert not missing, "paths no cell reaches: %r" % missing
    assert not thin, "paths reached at one element size only: %r" % thin
    # the three batch states, in both directions
    for entry in ("batch_exact", "batch_fast", "batch_decode"):
        states = {p.split(" ")[0] for p in cells[entry]}
        assert {"both", "al8", "neither"} <= states, (entry, states)


def test_range_lists_reach_both_groups():
    """The range decode's two groups: direct pieces at residues 0, 8, 4 and
    odd, and a list whose second group is 8-aligned throughout (staged for
    E != 1, byte stores by the E = 1 rule)."""
    seen_two = {}
    for E in C.RANGE_ELEM_SIZES:
        lists = C.range_lists(E)
        for shift in C.RANGE_OUT_SHIFTS:
            for name, ranges in lists.items():
                res = C.direct_residues(E, ranges, shift)
                assert len(res) >= 2
                one, two = M.range_groups(E, C.RANGE_BLOCK, res)
                assert one is not None
                if two is not None:
                    seen_two.setdefault(two, set()).add(E)
                if shift == 0 and name == "residues":
                    want = {0, 8} | ({4} if 4 % E == 0 or E == 3 else set()) | ({1} if E in (1, 3) else set())
                    assert want <= set(res), (E, res)
                if shift == 0 and name == "al8":
                    assert set(res) == {0, 8} and two[0] == "al8", (E, res, two)
    assert seen_two[("al8", "dec:ek0/stage-regs")] >= {2, 3, 4, 8}
    assert seen_two[("al8", "dec:ek0/bytes/E1-rule")] == {1}
    assert seen_two[("neither", "dec:ek0/bytes")] >= {1, 2, 3}


CELLS_PER_E = {1: 18, 2: 17, 3: 17, 4: 17, 5: 17, 8: 16, 12: 15, 16: 15}
FAST_CELLS = 78


def test_cell_count():
    """None can silently drop out."""
    per_E = {E: len(C.classes(E)) for E in C.ELEM_SIZES}
    assert per_E == CELLS_PER_E, per_E
    assert len(C.cells()) == sum(CELLS_PER_E.values())
    assert len(C.fast_cells()) == FAST_CELLS
    assert len(C.OFFSETS) == 8 and len(C.BATCH_RESIDUES) == 3
    for E in C.ELEM_SIZES:
        names = "+".join(name for name, _ in C.classes(E)).split("+")
        assert sorted(names) == sorted(n for n, _ in C.class_sizes(E)) and len(names) == 19, E
        for _, n in C.classes(E):
            assert n % (8 * E) == 0


