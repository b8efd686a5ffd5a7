"""CPU tests of the crafted fast-parse blocks (tests/fast_craft.py, DESIGN.md
§4.1g): a scalar restatement of the rule of §6.6 equals the numpy model on
every crafted block and on a seeded fuzz; every case's declared parse is the
model's parse and its claimed events are in its census; every payload decodes;
and the census of the crafted set holds every (shape, event) cell except the
listed ones that cannot exist.  `pytest -s` prints both census tables."""
import collections
import fnmatch

import numpy as np
import pytest

import oracle as oracle_mod
from tests import dispatch_model, fast_cases, fast_craft, fast_model


# ---- the rule, restated in plain loops from the text of DESIGN.md §6.6 --------
def scalar_parse(block, E):
    s = bytes(block)
    L = len(s)
    if L < 13:                                   # short blocks: one literal-only sequence
        return [(0, L, 0, 0)]
    P = L // (8 * E)
    D = []
    for d in (1, 2, 3, 4, 8, P, 2 * P):          # sorted distinct values that are < L
        if 0 < d < L and d not in D:
            D.append(d)
    D.sort()
    seqs = []
    anchor, ip = 0, 1
    while True:
        found = None
        p = ip
        while p <= L - 12:                       # the smallest p >= ip with p <= L - 12 ...
            longest, offset = 0, 0
            for d in D:
                if p < d or s[p] != s[p - d]:    # (run_d(p) = 0)
                    continue
                q = p
                while q < L and s[q] == s[q - d]:  # consecutive q >= p, q < L, q >= d
                    q += 1
                run = min(q - p, L - 5 - p)      # the capped run
                if run > longest:                # ties to the smaller offset (D ascends)
                    longest, offset = run, d
            if longest >= 4:                     # ... whose largest capped run is >= 4
                found = (p, offset, longest)
                break
            p += 1
        if found is None:
            break
        p, offset, length = found
        seqs.append((anchor, p - anchor, offset, length))
        anchor = ip = p + length
    seqs.append((anchor, L - anchor, 0, 0))      # last sequence: literals [anchor, L)
    return seqs


@pytest.fixture(scope="module")
def families():
    """{shape name: (E, block elements, [Case])} of the main and the tiny shapes."""
    return {name: (E, m, fast_craft.shape_cases(name, E, m)) for name, E, m in fast_craft.SHAPES + fast_craft.TINY}


@pytest.fixture(scope="module")
def partials():
    return {name: (E, m, m_last) + fast_craft.partial_cases(name, E, m, m_last)
            for name, E, m, m_last in fast_craft.PARTIAL}


@pytest.fixture(scope="module")
def reference():
    return oracle_mod.Reference() if oracle_mod.reference_available() else None


def _all_cases(families, partials):
    for E, m, cases in families.values():
        yield from cases
    for E, m, m_last, full, last in partials.values():
        yield last


def test_scalar_rule_equals_model_on_every_crafted_block(families, partials):
    for c in _all_cases(families, partials):
        assert scalar_parse(c.s, c.E) == fast_model.parse(c.s, c.E), c.id


def test_scalar_rule_equals_model_on_a_fuzz_of_structured_blocks():
    """Small blocks over alphabets of 1..4 symbols with imposed periodic
    stretches (periods from the block's own offset set and their neighbours)."""
    rng = np.random.default_rng(20260)
    nmatch = 0
    for it in range(2000):
        E = int(rng.choice([1, 2, 3, 4, 5, 8, 12]))
        L = E * int(rng.integers(1, 40)) * 8
        s = rng.integers(0, int(rng.integers(1, 5)), L, dtype=np.uint8)
        P = L // (8 * E)
        for _ in range(int(rng.integers(0, 4))):
            d = int(rng.choice([1, 2, 3, 4, 5, 7, 8, 9, P, P + 1, 2 * P, max(2 * P - 1, 1)]))
            a = int(rng.integers(0, L))
            b = min(L, a + int(rng.integers(1, 3 * d + 40)))
            for q in range(max(a, d), b):
                s[q] = s[q - d]
        want = fast_model.parse(s, E)
        nmatch += len(want) - 1
        assert scalar_parse(s, E) == want, (it, E, L, s.tobytes().hex())
    assert nmatch > 2000


def test_declared_parse_is_the_models_and_claims_are_in_the_census(families, partials):
    """The hand-derived sequences of every case are the model's whole parse, at
    their positions (so the filler between them is inert), and the events a
    case is there for are in its census."""
    for c in _all_cases(families, partials):
        got = fast_model.parse(c.s, c.E)
        assert [(ll, d, n) for _, ll, d, n in got[:-1]] == c.parse, c.id
        pos = 0
        for (a, ll, d, n), (ll2, d2, n2) in zip(got, c.parse):
            assert a == pos and (ll, d, n) == (ll2, d2, n2), c.id
            pos = a + ll + n
        assert got[-1] == (pos, c.s.size - pos, 0, 0), c.id
        ev = fast_craft.census(c.s, c.E, "sreg" in fast_craft.instance(c.E, c.m))
        assert c.claims <= set(ev), (c.id, sorted(c.claims - set(ev)))


def test_streams_round_trip_and_payloads_decode(oracle, reference, families, partials):
    """bitshuffle(stream) is the crafted bytes; each payload decodes (oracle and,
    when built, the reference's LZ4_decompress_safe) to its block within the
    record bound; the framed stream decodes to the input."""
    todo = [(E, m, cases, None) for E, m, cases in families.values()]
    todo += [(E, m, full, last) for E, m, m_last, full, last in partials.values()]
    for E, m, cases, last in todo:
        raw = fast_craft.stream(oracle, cases, m, last)
        arr = fast_cases.view_e(raw, E)
        blocks = [c.s for c in cases] + ([last.s] if last else [])
        assert oracle.bitshuffle(arr, m).view(np.uint8).tobytes() == b"".join(b.tobytes() for b in blocks)
        stream = fast_model.compress_lz4(oracle, arr, m)
        assert stream.size <= oracle.compress_lz4_bound(arr.size, E, m)
        assert oracle.decompress_lz4(stream, arr.shape, arr.dtype, m).tobytes() == raw.tobytes()
        recs = fast_model.block_records(stream, oracle, arr, m)
        assert len(recs) == len(blocks)
        for (L, payload), b, c in zip(recs, blocks, cases + [last]):
            assert L == b.size and 4 + payload.size <= 4 + L + L // 255 + 16, c.id
            assert oracle.lz4_decompress_block(payload, L).tobytes() == b.tobytes(), c.id
            if reference is not None:
                assert reference.lz4_decompress_block(payload, L).tobytes() == b.tobytes(), c.id
            assert fast_craft.sequences(payload)[:-1] == c.parse, c.id


def test_partial_block_streams_reach_their_branches(partials):
    """The SREG stream's partial block (P % 4 != 0) is transposed straight from
    HBM; the 8-slot stream's partial block has another P than the full blocks;
    both hold a match at exactly their own P."""
    E, m, m_last, full, last = partials["E2_bs4096_last304"]
    paths = dispatch_model.encode(E, m, len(full) * m + m_last, 0, fast=True)
    assert paths == ("fast:ek/sreg/reg", "fast:ek/sreg/direct") and (m_last // 8) % 4
    E, m, m_last, full, last = partials["E3_bs2728_last344"]
    paths = dispatch_model.encode(E, m, len(full) * m + m_last, 0, fast=True)
    assert paths == ("fast:ek0/slots/words", "fast:ek0/slots/words") and m_last // 8 != m // 8
    for E, m, m_last, full, last in partials.values():
        assert (m_last // 8, m_last // 8, 6) in last.parse and 2 * (m_last // 8) in [d for _, d, _ in last.parse]


# ---- census -------------------------------------------------------------------
# (shape pattern, event pattern, why the cell cannot exist); every other cell
# of shapes x fast_craft.EVENTS must be hit, and none of these may be
NO_REGS = ["E3_bs2728", "E1_bs8200", "E8_bs1024", "E2_bs16384"]
EXCLUDED = [
    ("*", "mea:win:1>smaller", "no offset is smaller than 1"),
    ("*", "mea:win:2P>larger", "no offset is larger than 2P"),
    ("*", "mea:win:2>smaller", "only offset 1 is smaller: its run of k >= 1 bytes makes s[p-1 .. p+k) constant, so "
                               "s[p+k] differs from s[p+k-2] as well and the 2-run is no longer"),
    ("*", "mea:win:3>smaller", "against 1 as for 2; a 2-run of k >= 4 under a longer 3-run makes s[p-2 .. p+k) "
                               "constant (periods 2 and 3 over >= 4 bytes), which ends the 3-run at p+k too"),
    ("*", "mea:win:4>smaller", "1 and 2 divide 4, so their run of k >= 3 bytes carries the 4-run no further than "
                               "itself; 3 and 4 over >= 6 bytes make the bytes constant, as for 3"),
    ("E*", "set:*", "offset-set merging: P is 1..8 or 16 only in the tiny blocks"),
    ("E[1348]_*", "ll=163*", "more than 64 length bytes need a 32 KiB block"),
    ("E2_bs4096", "ll=163*", "more than 64 length bytes need a 32 KiB block"),
    ("E[1348]_*", "ml=163*", "more than 64 length bytes need a 32 KiB block"),
    ("E2_bs4096", "ml=163*", "more than 64 length bytes need a 32 KiB block"),
    ("E[1348]_*", "last>=16335", "more than 64 length bytes need a 32 KiB block"),
    ("E2_bs4096", "last>=16335", "more than 64 length bytes need a 32 KiB block"),
    ("tiny", "ll=163*", "blocks of at most 512 bytes"), ("tiny", "ml=163*", "blocks of at most 512 bytes"),
    ("tiny", "last>=16335", "blocks of at most 512 bytes"), ("tiny", "last=525", "blocks of at most 512 bytes"),
    ("tiny", "sel:gap=6?w", "at most 16 words"), ("tiny", "sel:gap>=*", "at most 16 words"),
    ("tiny", "sel:reg+?", "at most 16 words: one start register"), ("tiny", "mea:round3", "at most 16 words"),
    ("E1_bs384", "sel:gap=6?w", "12 words"), ("E1_bs384", "sel:gap>=*", "12 words"),
    ("E1_bs384", "sel:reg+?", "12 words: one start register"), ("E1_bs384", "mea:round3", "12 words"),
    ("E1_bs384", "last=525", "384 bytes"),
    ("E4_bs544", "sel:gap>=128w", "68 words"), ("E4_bs544", "sel:reg+2", "68 words: two start registers"),
    ("E1_bs8200", "sel:last-word", "L % 32 = 8: the last word's positions are all past L - 12"),
] + [(s, "sel:reg+?", "the 8-slot layout keeps the starts in LDS, not in registers") for s in NO_REGS] + [
    (s, "mea:far-unaligned-P", "P % 4 = 0 in this shape") for s in
    ("E2_bs4096", "E4_bs544", "E1_bs384", "E8_bs1024", "E2_bs16384")]


def _excluded(shape, event):
    return any(fnmatch.fnmatchcase(shape, s) and fnmatch.fnmatchcase(event, e) for s, e, _ in EXCLUDED)


def _crafted_census(families):
    rows = collections.OrderedDict()
    for name, (E, m, cases) in families.items():
        col = "tiny" if name.startswith("tiny") else name
        row = rows.setdefault(col, collections.Counter())
        for c in cases:
            row.update(fast_craft.census(c.s, E, "sreg" in fast_craft.instance(E, m)))
    return rows


def test_census_every_cell_that_can_exist_is_hit(families):
    rows = _crafted_census(families)
    print("\ncrafted blocks, events per shape (" + ", ".join(
        "%s: %s" % (n, fast_craft.instance(E, m)) for n, E, m in fast_craft.SHAPES) + ")")
    print(fast_craft.census_table(rows))
    missing = [(s, e) for s in rows for e in fast_craft.EVENTS if not rows[s][e] and not _excluded(s, e)]
    surplus = [(s, e) for s in rows for e in fast_craft.EVENTS if rows[s][e] and _excluded(s, e)]
    assert not missing, missing
    assert not surplus, surplus
    for s, e, why in EXCLUDED:  # every entry of the list names at least one cell
        assert why and any(fnmatch.fnmatchcase(r, s) for r in rows)
        assert any(fnmatch.fnmatchcase(x, e) for x in fast_craft.EVENTS)
    # every instance the issue names is reached, and the tiny blocks cover both layouts
    assert {fast_craft.instance(E, m) for _, E, m in fast_craft.SHAPES} == {
        "ek2/sreg", "ek4/sreg", "ek1/sreg", "ek0/slot8", "ek1/slot8", "ek8/slot8", "ek2/slot8"}
    assert {fast_craft.instance(E, m).split("/")[1] for _, E, m in fast_craft.TINY} == {"sreg", "slot8"}


def test_census_of_the_incidental_inputs(oracle):
    """The same census over tests/fast_cases.py's inputs (G1/G2, zeros, random,
    period 3), per kernel instance: printed for DESIGN.md §4.1g, and a guard
    that the crafted set is needed -- these events are in none of them."""
    rows = collections.OrderedDict()
    seen = set()
    for name, raw, E, bsz in fast_cases.cases(oracle) + [fast_cases.segmented_case(oracle)]:
        arr = fast_cases.view_e(raw, E)
        bs = bsz or oracle.default_block_size(E)
        if not arr.size or bs * E > fast_model.FAST_MAX_BLOCK_BYTES:
            continue
        inst = fast_craft.instance(E, bs)
        shuf = oracle.bitshuffle(arr, bs).view(np.uint8).reshape(-1)
        for off, m in fast_model.blocks(oracle, arr, bsz)[0]:
            s = shuf[off * E:(off + m) * E]
            key = (E, inst, s.tobytes())
            if key not in seen:
                seen.add(key)
                rows.setdefault(inst, collections.Counter()).update(fast_craft.census(s, E, "sreg" in inst))
    print("\ntests/fast_cases.py, events per kernel instance")
    print(fast_craft.census_table(rows))
    total = sum(rows.values(), collections.Counter())
    for e in ("sel:p=L-12:len4", "sel:p=L-12:len7", "ll=269", "ll=270", "ll=271", "ll=319", "ll=320", "ml=273",
              "ml=274", "ml=275", "last=270", "last=525", "last>=16335"):
        assert not total[e], e
    assert "ek1/slot8" not in rows
