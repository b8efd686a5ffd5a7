"""The value tables of the converting gathers (tests/cvt_values.py), on the CPU:

* the reference the GPU tests compare with (float64, then one rounding to fp32,
  then the destination) against the rule restated in exact arithmetic, on every
  (value, parameters) entry of every kind pair; r64 exact wherever the table
  says so; the bfloat16 restatement against torch's CPU conversion;
* the results the tables were chosen for, by value;
* coverage: the window layouts put every table value on every path of the
  span routine (and, over the set, in a verbatim tail) for all 21 kind pairs;
  the ragged and tile layouts the stated subset, under every lane
  instantiation;
* sensitivity: every wrong variant of the rule changes at least one expected
  bit of every kind pair it can show in.  This is the evidence that the tables
  would catch such a kernel; it does not touch the kernels."""
import numpy as np
import pytest

from tests import cvt_values as V

PAIR_IDS = ["%s-%s" % p for p in V.PAIRS]


def entries(src, dst):
    for x, _ in V.TABLE[src]:
        for scale, offset, _ in V.params(src, dst):
            yield x, scale, offset


def test_tables_are_well_formed():
    for src in V.SRC:
        vals = [v for v, _ in V.TABLE[src]]
        assert len(set(vals)) == len(vals), src
        assert all(why for _, why in V.TABLE[src])
        V.table_array(src)
        for dst in V.DST:
            ps = V.params(src, dst)
            assert len({(V.fbits(s), V.fbits(o)) for s, o, _ in ps}) == len(ps)
            for s, o, why in ps:
                # the parameters are float32 values: nothing is lost on the way to the kernel
                assert float(V.f32(s)) == s and float(V.f32(o)) == o and why


@pytest.mark.parametrize("pair", V.PAIRS, ids=PAIR_IDS)
def test_reference_is_the_rule(pair):
    """ref_bits == model_bits on every entry; r64 is exact on every finite
    entry but float32 sources of large magnitude with an offset, where the sum
    needs more than 53 bits (the exact model decides there)."""
    src, dst = pair
    x = V.table_array(src)
    inexact = []
    for scale, offset, _ in V.params(src, dst):
        got = V.ref_bits(x, scale, offset, dst)
        want = np.array([V.model_bits(src, dst, xv, scale, offset) for xv, _ in V.TABLE[src]], dtype=got.dtype)
        bad = V.mismatches(got, want, dst)
        assert bad.size == 0, (src, dst, scale, offset, [V.TABLE[src][i][0] for i in bad])
        # NaN exactly where the model says NaN
        assert np.array_equal(V.is_nan_bits(got, dst), V.is_nan_bits(want, dst))
        for xv, _ in V.TABLE[src]:
            if V.entry_is_finite(src, xv) and not V.r64_is_exact(src, xv, scale, offset):
                inexact.append((xv, scale, offset))
    for xv, scale, offset in inexact:
        assert src == "float32" and offset != 0, (src, xv, scale, offset)
    if src != "float32":
        assert not inexact


def test_bf16_restatement_against_torch():
    import torch
    for src in V.SRC:
        x = V.table_array(src)
        for scale, offset, _ in V.params(src, "bfloat16"):
            with np.errstate(invalid="ignore", over="ignore", under="ignore"):
                y32 = V.r64_of(x, scale, offset).astype(np.float32)
            mine = V.to_dst_bits(y32, "bfloat16")
            theirs = torch.from_numpy(y32.copy()).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
            assert V.mismatches(theirs, mine, "bfloat16").size == 0, (src, scale, offset)


def one(src, dst, x, scale, offset):
    a = np.array([x], dtype=np.uint32).view(np.float32) if src == "float32" else np.array([x], dtype=np.dtype(src))
    return int(V.ref_bits(a, scale, offset, dst)[0])


def h(v):
    return int(np.array([v], dtype=np.float16).view(np.uint16)[0])


def b(v):
    return V.fbits(v) >> 16


def test_the_results_the_tables_were_chosen_for():
    inf = float("inf")
    for src in V.SRC[:6]:
        # -0 keeps its sign
        assert one(src, "float32", 0, -1.0, -0.0) == 0x80000000
        assert one(src, "float16", 0, -1.0, -0.0) == 0x8000
        assert one(src, "bfloat16", 0, -1.0, -0.0) == 0x8000
        # fused
        assert one(src, "float32", 3, 1.0 + 2.0 ** -23, -3.0) == V.fbits(3 * 2.0 ** -23)
        # half subnormals
        assert one(src, "float16", 1, 2.0 ** -24, 0.0) == 1
        assert [one(src, "float16", x, 2.0 ** -25, 0.0) for x in (1, 3, 5, 7)] == [0, 2, 2, 4]
        assert one(src, "float16", 3, 2.0 ** -26, 0.0) == 1
        # the overflow edge
        assert [one(src, "float16", x, 1.0, 65440.0) for x in (64, 79, 80)] == [0x7BFF, 0x7BFF, 0x7C00]
        assert [one(src, "float16", x, -1.0, -65440.0) for x in (64, 79, 80)] == [0xFBFF, 0xFBFF, 0xFC00]
        assert [one(src, "float16", x, 1.0, 2048.0) for x in (1, 3)] == [h(2048.0), h(2052.0)]
        assert one(src, "float16", 1, 2.0 ** -20, 2049.0) == h(2048.0)
        # bfloat16
        assert [one(src, "bfloat16", x, 1.0, 256.0) for x in (1, 3)] == [b(256.0), b(260.0)]
        assert [one(src, "bfloat16", x, 2.0 ** -133, 0.0) for x in (1, 2, 3)] == [1, 2, 3]
        assert [one(src, "bfloat16", x, 2.0 ** -134, 0.0) for x in (1, 3, 5, 7)] == [0, 2, 2, 4]
        assert one(src, "bfloat16", 1, 2.0 ** -20, 257.0) == b(256.0)
        # float32
        assert [one(src, "float32", x, 2.0 ** -149, 0.0) for x in (1, 3, 100)] == [1, 3, 100]
        assert [one(src, "float32", x, 2.0 ** 127, 0.0) for x in (1, 2)] == [V.fbits(2.0 ** 127), V.fbits(inf)]
    for src in ("uint16", "uint32", "int32"):
        assert [one(src, "float16", x, 1.0, 0.0) for x in (65504, 65519, 65520)] == [0x7BFF, 0x7BFF, 0x7C00]
        assert [one(src, "float16", x, -1.0, -0.0) for x in (65504, 65519, 65520)] == [0xFBFF, 0xFBFF, 0xFC00]
    for src in V.SRC[2:6]:
        assert [one(src, "float16", x, 1.0, 0.0) for x in (2049, 2051)] == [h(2048.0), h(2052.0)]
        assert [one(src, "bfloat16", x, 1.0, 0.0) for x in (257, 259)] == [b(256.0), b(260.0)]
        assert one(src, "float32", 4097, 1.0 + 2.0 ** -12, -4098.0) == V.fbits(2.0 ** -12)
    for src in ("uint32", "int32"):
        assert one(src, "float32", (1 << 24) + 1, 0.5, 0.25) == V.fbits(2.0 ** 23)
        assert one(src, "float32", (1 << 24) + 1, 2.0 ** -4, -(2.0 ** 20)) == 0
        assert one(src, "float32", 256, 2.0 ** 120, 0.0) == V.fbits(inf)
    assert one("uint32", "float32", 0xFFFFFF7F, 0.5, 0.25) == V.fbits(2.0 ** 31 - 128)
    assert one("uint32", "float32", 0xFFFFFF80, 0.5, 0.25) == V.fbits(2.0 ** 31)
    assert one("int32", "float32", (1 << 31) - 65, 0.5, 0.25) == V.fbits(2.0 ** 30 - 64)
    assert one("int32", "float32", (1 << 31) - 64, 0.5, 0.25) == V.fbits(2.0 ** 30)
    F = "float32"
    assert one(F, "bfloat16", 0x7F7F8000, 1.0, 0.0) == 0x7F80 and one(F, "bfloat16", 0x7F7F7FFF, 1.0, 0.0) == 0x7F7F
    assert one(F, "float32", 0x80000000, 1.0, 0.0) == 0 and one(F, "float32", 0x80000000, 1.0, -0.0) == 0x80000000
    assert one(F, "float32", 0x7F7FFFFF, 2.0, 0.0) == 0x7F800000
    assert one(F, "float32", 0x00800000, 0.5, 0.0) == 0x00400000
    assert one(F, "float32", 0x00000001, 0.5, 0.0) == 0 and one(F, "float32", 0x00000003, 0.5, 0.0) == 2
    assert one(F, "float32", 0x00000001, 1.0, 0.0) == 1 and one(F, "float32", 0x807FFFFF, 1.0, 0.0) == 0x807FFFFF
    assert one(F, "float16", 0x00000001, 2.0 ** 125, 0.0) == 1
    assert V.is_nan_bits(np.array([one(F, "float32", 0x7F800000, 0.0, 0.0)]), "float32")[0]
    assert one(F, "float32", V.fbits(-3.0), 0.0, 0.0) == 0     # -0 + +0
    assert one(F, "float16", V.fbits(-2.0 ** -25), 1.0, 0.0) == 0x8000


# ------------------------------------------------------------------ coverage
@pytest.mark.parametrize("pair", V.PAIRS, ids=PAIR_IDS)
def test_window_layouts_put_every_value_on_every_path(pair):
    src, dst = pair
    lay = V.layout(src)
    D = V.DSIZE[dst]
    paths = V.all_paths(lay.S, D)
    assert {"single", "head", "unit-aligned", "tail"} <= paths
    assert ("chunk" in paths) == (max(16 // lay.S, 16 // D) * D > 16)
    shifted = {p for p in paths if p.startswith("unit-shifted")}
    assert len(shifted) == (4 if lay.S < 4 else 3)
    have, lanes = set(), set()
    for starts, window, doff in lay.window_calls(D):
        lay.cover_windows(D, [0] * len(starts), starts, window, doff, have)
        lanes.add(window * max(lay.S, D) > 2048)
    assert lanes == {False, True}
    want = V.every_pair(lay, paths)
    assert want <= have, sorted(want - have)[:8]
    # the long windows alone hold every value in head, units, chunks and tail
    long_have = set()
    for starts, window, doff in lay.window_calls(D):
        if window * max(lay.S, D) > 2048:
            lay.cover_windows(D, [0] * len(starts), starts, window, doff, long_have)
    want_long = V.every_pair(lay, paths - {"single"})
    assert want_long <= long_have, sorted(want_long - long_have)[:8]
    # over the set: every value in a verbatim tail, too
    set_have = set()
    for ids, starts, window, doff in lay.set_calls(D):
        lay.cover_windows(D, ids, starts, window, doff, set_have)
    want_tail = V.every_pair(lay, {"vtail"})
    assert want_tail <= set_have, sorted(want_tail - set_have)[:8]


@pytest.mark.parametrize("pair", V.PAIRS, ids=PAIR_IDS)
def test_ragged_and_tile_layouts_hold_the_stated_paths(pair):
    src, dst = pair
    lay = V.layout(src)
    D = V.DSIZE[dst]
    want = V.every_pair(lay, V.SUBSET)
    calls, (t_ids, t_starts, t_counts) = lay.ragged_calls(D)
    seen = set()
    for ids, starts, counts, max_window, pitch, doff in calls:
        have = set()
        lay.cover_ragged(D, ids, starts, counts, pitch, doff, have)
        assert max(counts) <= max_window
        assert want <= V.fold_shifted(have), (max_window, pitch, sorted(want - V.fold_shifted(have))[:8])
        seen.add((max_window * max(lay.S, D) > 2048, pitch > 0))
    assert len(seen) == 4, "packed and pitched under both lane instantiations"
    tails = set()
    lay.cover_ragged(D, t_ids, t_starts, t_counts, 0, 0, tails)
    assert V.every_pair(lay, {"vtail"}) <= tails
    by_lanes = {16: set(), 64: set(), 256: set()}
    for starts, rows, cols, pitch, doff in lay.tile_calls(D):
        lay.cover_tiles(D, [0] * len(starts), starts, rows, cols, pitch, doff, by_lanes[lay.lanes_of_tiles(D, cols)])
    assert want <= V.fold_shifted(set().union(*by_lanes.values()))
    for T, have in by_lanes.items():
        w = V.every_pair(lay, ["unit-aligned", "unit-shifted", "tail"])
        assert w <= V.fold_shifted(have), (T, sorted(w - V.fold_shifted(have))[:8])


# --------------------------------------------------------------- sensitivity
@pytest.mark.parametrize("wrong", V.WRONG)
def test_every_wrong_variant_changes_an_expected_bit(wrong):
    for src, dst in V.PAIRS:
        changed = []
        for x, scale, offset in entries(src, dst):
            right = V.model_bits(src, dst, x, scale, offset)
            if V.is_nan_bits(np.array([right]), dst)[0]:
                continue     # a NaN's bits are not compared
            if V.model_bits(src, dst, x, scale, offset, wrong) != right:
                changed.append((x, scale, offset))
        if V.wrong_applies(wrong, src, dst):
            assert changed, "%s would pass on %s -> %s" % (wrong, src, dst)
        else:
            assert not changed, (wrong, src, dst, changed[:3])
