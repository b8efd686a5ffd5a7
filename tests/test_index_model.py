"""What the decoy streams of tests/index_model.py visit in the block-index
rebuild (csrc/lz4_decode.hip), asserted on the CPU with the model of its phase
1; tests/test_gpu_index_rebuild.py runs the same streams on the device.  Every
stream is also decoded by the oracle and walked by the serial index, which
must tile [0, Cb) with its blocks.
"""
import numpy as np
import pytest

from tests import index_model as M

A, DEAD = M.AMBIGUOUS, M.DEAD

# seeds of the random streams (density 6) that give three and more ambiguous
# chunks each: picked with the model, asserted below
RANDOM_SEEDS = (20, 23, 24)
RANDOM_DENSITY = 6
RANDOM_BLOCKS = 95      # 8 KiB blocks: 6 chunks (larger than the crafted streams, still under 1 MiB)

_CACHE = {}


def built(name, *args):
    key = (name,) + args
    if key not in _CACHE:
        c = getattr(M, name)(*args)
        c.ex = M.exits(c.buf, c.Cb, c.n)
        _CACHE[key] = c
    return _CACHE[key]


def everything():
    """(id, builder name, args) of every crafted stream."""
    out = [("d1-%s" % v, "d1", (v,)) for v in M.D1_VARIANTS]
    out += [("d2%s-%s" % (k, s), "d2", (k, s)) for s in M.D2_SHAPES for k in M.D2_KINDS]
    out += [("d1_8k", "d1_8k", ())]
    out += [("d3-%s" % k, "d3", (k,)) for k in M.D3_KINDS]
    out += [("d4-%s" % k, "d4", (k,)) for k in M.D4_KINDS]
    out += [("random-%d" % s, "random_stream", (s, RANDOM_DENSITY, 1, 8192, RANDOM_BLOCKS)) for s in RANDOM_SEEDS]
    return out


EVERYTHING = everything()


def exit_codes(c):
    return [x.exit for x in c.ex]


def true_exits(c):
    """Per chunk the first true header at or behind its end (Cb: none)."""
    nch = c.g.nchunks(c.Cb)
    st = c.starts.tolist() + [c.Cb]
    return [min(x for x in st if x >= min((s + 1) * c.g.CH, c.Cb)) for s in range(nch)]


# ------------------------------------------------------------------ geometry
def test_geometry_of_the_shapes_used():
    g = M.Geometry(64)
    assert (g.maxlen, g.W, g.CH, g.ny, g.wsub) == (80, 84, 131072, 1, 84)
    g = M.Geometry(8192)
    assert (g.maxlen, g.W, g.CH, g.ny, g.win_lds) == (8240, 8244, 131072, 1, 8336)
    g = M.Geometry(M.D4_BLOCK)
    assert (g.maxlen, g.W, g.CH, g.ny, g.wsub, g.win_lds) == (49360, 49364, 131072, 2, 32640, 32768)
    g = M.Geometry(1 << 20)     # CH doubles until it holds two of the largest records
    assert g.CH == 4 << 20 and g.CH >= 2 * g.W and g.ny == 33
    assert M.layout(50 * 680 + 7, 680) == (50, 7) and M.layout(3 * 64 + 16 + 5, 64) == (4, 5)


def test_the_global_memory_branch_of_phase_1_cannot_be_reached():
    """k_idx_exits reads its candidates from global memory when the slice does
    not fit the LDS window (`use_lds` false).  With the win_lds and wsub the
    host passes it always fits: a slice stages at most 15 + wsub + 3 bytes in
    whole 16-byte granules.  Swept over every maxlen to 2^17 and a spread of
    larger ones (the two regimes meet near 32 KiB)."""
    ns = list(range(8, 1 << 17, 8)) + [(1 << k) + d for k in range(17, 31) for d in (-8, 0, 8, 4088)]
    split = whole = 0
    for n in ns:
        g = M.Geometry(n)
        assert M.slice_lds_bytes(g.wsub) <= g.win_lds, n
        assert g.wsub * g.ny >= g.W > g.wsub * (g.ny - 1)
        if g.ny > 1:
            split += 1
            assert g.win_lds == M.WIN_MAX and g.wsub == M.WIN_MAX - 128
        else:
            whole += 1
            assert g.wsub == g.W and g.win_lds <= M.WIN_MAX
    assert split > 1000 and whole > 1000
    # the last whole window and the first split one
    assert M.Geometry(32520).ny == 1 and M.Geometry(32528).ny == 2


# ------------------------------------------------------- every stream at once
@pytest.mark.parametrize("name,args", [e[1:] for e in EVERYTHING], ids=[e[0] for e in EVERYTHING])
def test_stream_is_valid_and_the_model_rebuilds_its_index(oracle, name, args):
    c = built(name, *args)
    assert len(c.buf) < (1 << 19) or name == "random_stream"
    assert len(c.buf) < (1 << 20)
    nb, tail_elems = M.layout(c.size, c.block)
    assert (nb, tail_elems * c.E) == (c.nb, c.tail) and c.Cb == len(c.buf) - c.tail
    # the serial walk tiles [0, Cb) with nb records
    want = M.serial_index(c.buf, c.Cb, c.nb)
    assert want.tolist() == c.starts.tolist() and len(want) == c.nb
    ends = want + 4 + np.array([int.from_bytes(c.buf[o:o + 4].tobytes(), "big") for o in want])
    assert ends[-1] == c.Cb and (ends[:-1] == want[1:]).all()
    # the oracle decodes it
    dt = np.uint8 if c.E == 1 else np.dtype("V%d" % c.E)
    dec = oracle.decompress_lz4(c.buf, (c.size,), dt, c.block)
    assert dec.nbytes == c.size * c.E
    # the model of phases 1 to 4 lands on the serial index
    got = M.rebuild(c.buf, c.Cb, c.n, c.nb)
    assert got is not None and got.tolist() == want.tolist()
    # the true chain survives every chunk
    for s, (x, t) in enumerate(zip(c.ex, true_exits(c))):
        assert t in x.survivors, s
    # nothing but what was planted is a candidate
    if name != "random_stream":
        extra = set(M.plausible_positions(c.buf, c.Cb, c.n).tolist()) - set(c.starts.tolist()) - set(c.planted)
        assert all(any(a <= p < b for a, b in c.fills) for p in extra)


# ------------------------------------------------------------------------ D1
@pytest.mark.parametrize("variant", M.D1_VARIANTS)
def test_d1_every_interior_chunk_is_ambiguous(variant):
    c = built("d1", variant)
    assert c.nb == 5800 and c.g.nchunks(c.Cb) == 4 and len(c.planted) == c.nb
    assert exit_codes(c) == [true_exits(c)[0], A, A, c.Cb]      # a run of two
    for s in (1, 2):
        x = c.ex[s]
        assert len(x.survivors) == 2 and true_exits(c)[s] in x.survivors
        assert 2 <= x.ncand <= 4
    # in one of them the decoy's exit is the smaller one (an ambiguous chunk
    # given its minimum would misplace the blocks behind it)
    assert any(c.ex[s].survivors[0] != true_exits(c)[s] for s in (1, 2))
    # the last decoy: implausible ("dies", "tail": it ends past Cb) or one more
    # chain that ends at Cb
    last = c.planted[-1]
    ln = int.from_bytes(c.buf[last:last + 4].tobytes(), "big")
    if variant == "dies":
        assert last + 4 + ln > len(c.buf)
    if variant == "exact":
        assert last + 4 + ln == c.Cb
    if variant == "tail":
        assert c.tail == 7 and c.Cb < last + 4 + ln < len(c.buf)
        assert c.buf[c.Cb:].tobytes() == M.words16(7)
    assert c.ex[3].survivors == [c.Cb]


def test_d1_at_8k_blocks():
    c = built("d1_8k")
    assert exit_codes(c) == [true_exits(c)[0], A, A, c.Cb] and c.n == 8192


# ------------------------------------------------------------------------ D2
@pytest.mark.parametrize("shape", list(M.D2_SHAPES))
def test_d2_visits(shape):
    t = None
    for kind in M.D2_KINDS:
        c = built("d2", kind, shape)
        t = true_exits(c)
        assert c.g.nchunks(c.Cb) == 4 and c.g.ny == 1
        want = [t[0], A if kind in ("a", "d") else t[1], t[2], c.Cb]
        assert exit_codes(c) == want, kind
        x = c.ex[1]
        cs = c.g.CH
        assert cs <= c.planted[0] < cs + c.g.W
        if kind == "a":     # exactly one ambiguous chunk; the decoy's exit is the minimum
            assert x.survivors == [2 * cs + 16, t[1]]
        if kind == "b":     # three decoys that reach a true header
            assert len(c.planted) == 3 and x.survivors == [t[1]] and x.ncand >= 2
            ln = int.from_bytes(c.buf[c.planted[-1]:c.planted[-1] + 4].tobytes(), "big")
            assert c.planted[-1] + 4 + ln in c.starts.tolist()
        if kind == "c":     # three decoys, dead inside the chunk
            assert len(c.planted) == 3 and x.survivors == [t[1]] and c.planted[-1] < 2 * cs - c.g.W
        if kind == "d":     # three distinct exits, the true one in the middle
            assert len(x.survivors) == 3 and x.survivors[1] == t[1] and x.survivors[0] == 2 * cs + 16
    assert built("d2", "a", "e12").tail == 7 * 12 and built("d2", "a", "e12").n == 8160


# ------------------------------------------------------------------------ D3
def test_d3_candidate_counts_and_flushes():
    for kind, ncand, flushes in (("below", 511, 0), ("at", 512, 0), ("above", 513, 1)):
        c = built("d3", kind)
        x = c.ex[2]
        assert (x.ncand, x.flushes) == (ncand, [flushes]), kind
        assert x.exit == A and len(x.survivors) == 2
    for kind in ("behind", "thousands", "first"):
        c = built("d3", kind)
        x = c.ex[2]
        t = true_exits(c)
        assert exit_codes(c) == [t[0], t[1], A, c.Cb]
        assert x.survivors == [3 * c.g.CH + 16, t[2]]
        true_hdr = t[1]                     # chunk 2's entry: chunk 1's exit
        decoy = min(c.planted)
        assert 2 * c.g.CH <= decoy and decoy < 2 * c.g.CH + c.g.W
        groups = x.flushed_at[0]
        where = {p: i for i, grp in enumerate(groups) for p in grp}
        assert x.flushes[0] >= 1 and max(len(grp) for grp in groups) <= M.CAND_CAP
        if kind == "first":     # the true header in the first flush, the live decoy in a later one
            assert where[true_hdr] == 0 < where[decoy]
        else:                   # the live decoy in the first flush, the true header in a later one
            assert where[decoy] == 0 < where[true_hdr]
            assert decoy == 2 * c.g.CH          # the window's first candidate
    x = built("d3", "thousands").ex[2]
    assert x.ncand > 2000 and x.flushes[0] >= 3
    # a step holds at most 256 candidates, so the list never overflows
    assert max(max(st) for c in (built("d3", k) for k in M.D3_KINDS) for st in c.ex[2].steps) <= M.STEP


# ------------------------------------------------------------------------ D4
def test_d4_per_slice_extremes():
    g = M.Geometry(M.D4_BLOCK)
    for kind in M.D4_KINDS:
        c = built("d4", kind)
        s = c.note["chunk"]
        t = true_exits(c)
        assert len(c.buf) < (1 << 19) and c.g.nchunks(c.Cb) == 4 and c.nb == 9
        want = [t[0], t[1], t[2], c.Cb]
        want[s] = A
        assert exit_codes(c) == want, kind
        decoy, true = (s + 1) * g.CH + 16, t[s]
        assert decoy < true
        head = c.planted[0] - s * g.CH
        sl = c.ex[s].slices
        if kind == "s0":
            assert head < g.wsub and sl == [(decoy, true), None]
        if kind == "s1":
            assert head >= g.wsub and sl == [None, (decoy, true)]
        if kind == "straddle":
            assert head == g.wsub - 2 and sl == [(decoy, true), None]
        if kind == "join_s1":   # each slice agrees with itself, the two differ
            assert head >= g.wsub and sl == [(true, true), (decoy, decoy)]
        if kind == "join_s0":
            assert head < g.wsub and sl == [(decoy, decoy), (true, true)]
        # the other interior chunk sees the true chain alone, in one slice
        o = 3 - s
        assert sorted(x for x in c.ex[o].slices if x) == [(t[o], t[o])]


# -------------------------------------------------------------------- random
@pytest.mark.parametrize("seed", RANDOM_SEEDS)
def test_random_streams_have_three_ambiguous_chunks(seed):
    c = built("random_stream", seed, RANDOM_DENSITY, 1, 8192, RANDOM_BLOCKS)
    assert exit_codes(c).count(A) >= 3
    assert len(c.planted) > 50


# --------------------------------------------------- the model on broken chains
def test_model_rejects_broken_chains():
    c = built("d2", "a", "e1")
    k = int(np.searchsorted(c.starts, 2 * c.g.CH))      # the true header behind the ambiguous chunk
    bad = c.buf.copy()
    bad[c.starts[k]:c.starts[k] + 4] = 0xFF
    assert M.rebuild(bad, c.Cb, c.n, c.nb) is None
    with pytest.raises(ValueError):
        M.serial_index(bad, c.Cb, c.nb)
    d = built("d1", "dies")
    cut = d.planted[-1]                                  # the decoy chain ends exactly here
    assert M.rebuild(d.buf[:cut], cut, d.n, d.nb - 1) is None
    assert M.exits(d.buf[:cut], cut, d.n)[3].survivors == [cut]
