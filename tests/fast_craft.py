"""TEST INFRASTRUCTURE ONLY -- crafted blocks for every rule of "fast parse v1"
(DESIGN.md §6.6, §4.1g), shared by tests/test_fast_craft.py (CPU) and
tests/test_gpu_fast_craft.py (GPU).

A block is crafted in the bit-transposed domain: the byte string `s` the parse
sees.  The codec's input is oracle.bitunshuffle(s viewed as E-byte elements).

A recipe names the match starts of one block as features (p, {d: n}): offset
d runs exactly n bytes from p (s[q] == s[q-d] for p <= q < p+n, the byte at
p+n chosen to break it and, unless p continues a match, the byte at p-1 too).
`craft` merges the equalities of all features (union-find), gives every class
of positions one seeded random byte -- positions no feature touches are the
inert filler -- and derives the parse the rule must give from the features
alone: (literal length, offset, match length) per match.  It never trusts the
filler: the declared runs and the declared parse are compared with
fast_model, under another seed when a random byte happens to extend a run.
Recipes that do not fit a shape (positions past the block, offsets above p)
or contradict themselves (an inequality inside one class) raise Infeasible
and are left out of that shape; tests/test_fast_craft.py's census then shows
what every shape holds and asserts that only what cannot exist is absent.
"""
import collections
import zlib

import numpy as np

from tests import dispatch_model, fast_cases, fast_model

W = 32  # positions per bitmap word


class Infeasible(Exception):
    pass


Case = collections.namedtuple("Case", "id s E m parse claims")
# id; s: the bit-transposed block; E; m: block elements; parse: the declared
# [(literal length, offset, match length)] of every match of the block;
# claims: the census events the case is there for

# (name, E, block elements): the smallest shapes at which each mechanism exists
SHAPES = [("E2_bs4096", 2, 4096), ("E4_bs544", 4, 544), ("E1_bs384", 1, 384), ("E3_bs2728", 3, 2728),
          ("E1_bs8200", 1, 8200), ("E8_bs1024", 8, 1024), ("E2_bs16384", 2, 16384)]
TINY_BS = (8, 16, 24, 32, 40, 48, 56, 64, 128)  # P = 1 .. 8, 16
TINY = [("tiny_E%d_bs%d" % (E, b), E, b) for E in (2, 4) for b in TINY_BS]
# (name, E, block elements, elements of the partial last block)
PARTIAL = [("E2_bs4096_last304", 2, 4096, 304),   # SREG, P = 38: transposed straight from HBM
           ("E3_bs2728_last344", 3, 2728, 344)]   # 8 slots, P = 43 against the full blocks' 341

LL_EVENTS = (0, 1, 14, 15, 16, 63, 64, 65, 269, 270, 271, 319, 320, 321, 16334, 16335, 16336)
ML_EVENTS = (4, 18, 19, 20, 273, 274, 275, 16338, 16339, 16340)
LAST_EVENTS = (5, 270, 525)
SLOTS = ("1", "2", "3", "4", "8", "P", "2P")
TIES = (("1", "2"), ("2", "4"), ("4", "8"), ("8", "P"), ("P", "2P"), ("3", "P"))
SET_P = (1, 2, 3, 4, 5, 6, 7, 8, 16)

EVENTS = (["sel:p=1", "sel:p=L-12:len4", "sel:p=L-12:len7", "sel:L-11-only", "sel:to-end", "sel:run3-none",
           "sel:carry29", "sel:carry30", "sel:carry31", "sel:p%32=0", "sel:p%32=31", "sel:stale",
           "sel:ll0-other-offset", "sel:gap=7w", "sel:gap=8w", "sel:gap=63w", "sel:gap=64w", "sel:gap>=64w",
           "sel:gap>=128w", "sel:reg+1", "sel:reg+2", "sel:last-word",
           "mea:end-in-start-word", "mea:end%32=0", "mea:round2", "mea:round3", "mea:two-rounds",
           "mea:far-unaligned-P"]
          + ["mea:win:%s>smaller" % x for x in SLOTS] + ["mea:win:%s>larger" % x for x in SLOTS]
          + ["mea:tie:%s=%s" % t for t in TIES] + ["mea:only:%s" % x for x in ("8", "P", "2P")]
          + ["ll=%d" % v for v in LL_EVENTS] + ["ml=%d" % v for v in ML_EVENTS]
          + ["last=%d" % v for v in LAST_EVENTS] + ["last=L", "last>=16335"]
          + ["set:P=%d:d=%s" % (k, x) for k in SET_P for x in ("P", "2P")])


def far_offsets(L, E):
    """(P, the offset of slot P, of slot 2P); 0 where it merges into 1, 2, 3, 4, 8."""
    P = L // (8 * E)
    return P, (0 if P <= 4 or P == 8 else P), (0 if P in (1, 2, 4) else 2 * P)


def slot_name(L, E, d):
    P, dP, d2P = far_offsets(L, E)
    return "P" if d == dP else "2P" if d == d2P else str(d)


def instance(E, m):
    """The kernel instance the full blocks of a stream reach (16-aligned data)."""
    ek = dispatch_model.pick_ek(E, True)
    return "ek%d/%s" % (ek, "sreg" if dispatch_model.fast_sreg(ek, m * E) else "slot8")


# ---- the builder --------------------------------------------------------------
def _find(par, i):
    while par[i] != i:
        par[i] = par[par[i]]
        i = par[i]
    return i


def craft(L, E, feats, seed=0):
    """(s, declared parse) of a block of L bytes holding the features
    [(p, {d: n})] or [(p, {d: n}, False)] (equalities that must NOT make a
    match: too short, or too late in the block)."""
    D = fast_model.offsets(L, E)
    par = list(range(L))
    neq, declared, checks = [], [], []
    ip = 1
    for f in sorted(feats, key=lambda f: f[0]):
        p, runs, is_match = f[0], f[1], (f[2] if len(f) > 2 else True)
        if p < ip or p >= L:
            raise Infeasible("feature at %d starts before %d or past the block" % (p, ip))
        for d, n in runs.items():
            if d not in D or p < d or p + n > L or n < 1:
                raise Infeasible("offset %d, run %d at %d in a block of %d" % (d, n, p, L))
            if L - 5 < p + n < L:
                # a run ends on a chosen byte in front of the cap or goes on to
                # the block's end; one that the cap would cut is a misfit
                raise Infeasible("run %d at %d ends inside the last 5 bytes" % (n, p))
            for q in range(p, p + n):
                a, b = _find(par, q), _find(par, q - d)
                if a != b:
                    par[a] = b
            if p + n < L:
                neq.append((p + n, p + n - d))
            if p - 1 >= ip and p - 1 >= d:
                neq.append((p - 1, p - 1 - d))
        cap = L - 5 - p
        capped = {d: max(min(n, cap), 0) for d, n in runs.items()}
        checks.append((p, capped))
        if is_match:
            best = max(capped.values())
            if best < 4 or p > L - 12:
                raise Infeasible("no match of >= 4 at %d" % p)
            d = min(d for d in capped if capped[d] == best)
            declared.append((p, d, best))
            ip = p + best
        elif p <= L - 12 and max(capped.values()) >= 4:
            raise Infeasible("the no-match feature at %d is a match" % p)
    root = np.array([_find(par, i) for i in range(L)])
    for a, b in neq:
        if root[a] == root[b]:
            raise Infeasible("bytes %d and %d must both differ and be equal" % (a, b))
    want, anchor = [], 0
    for p, d, n in declared:
        want.append((anchor, p - anchor, d, n))
        anchor = p + n
    want.append((anchor, L - anchor, 0, 0))
    for attempt in range(64):
        vals = np.random.default_rng([seed, attempt]).integers(0, 256, L, dtype=np.uint8)
        s = vals[root]
        if any(s[a] == s[b] for a, b in neq) or fast_model.parse(s, E) != want:
            continue
        runs = {d: fast_model._capped_runs(s, d) for d in D}
        if all(runs[d][p] == capped[d] if d in capped else runs[d][p] < 4 for p, capped in checks for d in D):
            return s, [(ll, d, n) for _, ll, d, n in want[:-1]]
    raise Infeasible("no seed gives the declared parse: %r" % (feats,))


# ---- recipes ----------------------------------------------------------------
def recipes(L, E):
    """[(name, features, claimed events)] for a block of L bytes; positions are
    chosen per shape, and what does not fit fails in craft()."""
    P, dP, d2P = far_offsets(L, E)
    nw = (L + 31) // 32
    R = []

    def add(name, feats, *claims):
        R.append((name, feats, set(claims)))

    # -- selection
    add("p1", [(1, {1: 6})], "sel:p=1", "ll=1")
    add("pL12_len4", [(L - 12, {1: 4})], "sel:p=L-12:len4")
    add("pL12_len7", [(L - 12, {1: 12})], "sel:p=L-12:len7", "sel:to-end", "last=5")
    add("L11_only", [(L - 11, {1: 6}, False)], "sel:L-11-only", "last=L")
    add("L11_only_far", [(L - 11, {dP or 8: 11}, False)], "sel:L-11-only", "last=L")
    add("to_end", [(L - 40, {2: 40})], "sel:to-end", "last=5")
    add("run3", [(40, {1: 3}, False), (60, {3: 3}, False), (80, {8: 3}, False),
                 (max(dP, 92) + 8, {dP or 4: 3}, False)], "sel:run3-none", "last=L")
    add("carry", [(2 * W + 29, {1: 4}), (4 * W + 30, {3: 4}), (6 * W + 31, {8: 4})],
        "sel:carry29", "sel:carry30", "sel:carry31", "sel:p%32=31", "ml=4")
    add("pmod32", [(3 * W, {2: 5}), (5 * W + 31, {3: 6})], "sel:p%32=0", "sel:p%32=31")
    add("stale", [(4 * W + 2, {1: 12}), (4 * W + 20, {2: 5})], "sel:stale")
    add("stale_far", [(max(dP, 3 * W) + W + 3, {dP or 3: 20}), (max(dP, 3 * W) + W + 27, {1: 4})], "sel:stale")
    add("back_to_back", [(100, {3: 8}), (108, {1: 6})], "sel:ll0-other-offset", "ll=0")
    add("gap7", [(W + 1, {1: 5}), (8 * W + 3, {2: 6})], "sel:gap=7w")
    add("gap8", [(W + 1, {1: 5}), (9 * W + 3, {2: 6})], "sel:gap=8w")
    add("gap63", [(63 * W + 5, {2: 6})], "sel:gap=63w")
    add("gap64", [(64 * W + 5, {2: 6})], "sel:gap=64w", "sel:gap>=64w")
    add("gap64_ip1", [(W + 1, {1: 5}), (66 * W + 3, {2: 6})], "sel:gap>=64w")
    add("gap128_ip1", [(W + 1, {1: 5}), (131 * W + 3, {3: 6})], "sel:gap>=128w")
    add("gap_reg2_to_3", [(130 * W, {1: 40}), (200 * W + 7, {8: 5})], "sel:gap>=64w")
    add("last_word", [((nw - 1) * W + 1, {1: 4})], "sel:last-word")
    # -- measure
    add("end_in_start_word", [(3 * W + 4, {1: 10})], "mea:end-in-start-word")
    if L > 4 * W:  # (at 128 bytes the run would be the one to the block's end)
        add("end_mod32", [(3 * W + 10, {1: 22})], "mea:end%32=0")
    add("round2", [(40, {1: 9 * W})], "mea:round2")
    add("round3", [(40, {1: 17 * W})], "mea:round3")
    if dP:
        # (equal bytes at p that also equal those at p - P: a short match there)
        add("two_rounds", [(9, {1: 9}), (dP + 8, {1: 10, dP: 300})], "mea:two-rounds")
        add("two_rounds_far_first", [(9, {1: 9}), (dP + 8, {1: 300, dP: 10})], "mea:two-rounds")
    base = 2 * P + 40

    def sl(d):
        return slot_name(L, E, d)

    def win(w, l, nl=4, pre=()):
        """offset w runs 9 bytes, offset l runs nl (>= 4, shorter) from the same p"""
        p = base + P if pre else base
        add("win%s_over_%s" % (sl(w), sl(l)), list(pre) + [(p, {w: 9, l: nl})],
            "mea:win:%s>%s" % (sl(w), "smaller" if l < w else "larger"))

    def tie(a, b, pre=(), p=base, tag=""):
        lo, hi = min(a, b), max(a, b)
        claims = ["mea:tie:%s=%s" % (sl(lo), sl(hi))] if (sl(lo), sl(hi)) in TIES else []
        add("tie_%s_%s%s" % (sl(a), sl(b), tag), list(pre) + [(p, {a: 10, b: 10})], *claims)

    for x in (1, 2, 3):
        win(x, 8)
    for x in (dP, d2P):  # (4 over 8: the 8 run would make the 4 run start earlier)
        if x > 4:
            win(4, x)
    win(8, 1)
    add("only8", [(8, {8: 6})], "mea:only:8")
    if dP:
        win(8, dP)
        win(dP, 1)
        win(dP, 8, 5)
        tie(8, dP)
        # (the 3 run's bytes repeat at p - P: a match of 7 there)
        tie(3, dP, pre=[(base - P + 3, {3: 7})])
        add("onlyP", [(dP, {dP: 6})], "mea:only:P")
    if d2P:
        win(d2P, 1)
        win(8, d2P)
        if dP:  # P a multiple of 8: the tie exists only behind a match
            tie(8, dP, pre=[(base, {d2P: 9})], p=base + 9, tag="_ll0")
        add("only2P", [(d2P, {d2P: 6})], "mea:only:2P")
    if dP and d2P:
        # a P run beside a 2P run repeats at p - P: one more match there
        win(dP, d2P, pre=[(base, {dP: 4})])
        win(d2P, dP, pre=[(base, {dP: 4})])
        q = base + P + 20
        add("tie_P_2P", [(q - P, {dP: 6}), (q - 9, {1: 9}), (q, {dP: 6, d2P: 6})], "mea:tie:P=2P")
    # ties of offsets that divide one another exist only where p continues a
    # match: the shorter offset's run would otherwise start the match earlier
    prev = dP or 3
    for a, b, n in ((1, 2, 9), (2, 4, 9), (4, 8, 5)):
        tie(a, b, pre=[(base, {prev: n})], p=base + n)
    # -- emit
    pairs = [(1, 273), (14, 274), (15, 275), (16, 4), (63, 18), (64, 19), (65, 20), (269, 4), (270, 18),
             (271, 19), (319, 20), (320, 4), (321, 18), (16334, 4), (16335, 5), (16336, 6), (2, 16338),
             (3, 16339), (4, 16340)]
    for ll, ml in pairs:
        claims = ["ll=%d" % ll] if ll in LL_EVENTS else []
        claims += ["ml=%d" % ml] if ml in ML_EVENTS else []
        add("ll%d_ml%d" % (ll, ml), [(ll, {1 if ll < 3 else 3: ml})], *claims)
    add("last270", [(L - 280, {1: 10})], "last=270")
    add("last525", [(L - 535, {2: 10})], "last=525")
    return R


def periodic(L, E, d, seed):
    """A block of period d with d distinct bytes: one match at p = d, the
    smallest offset of the set that is a multiple of d, to the cap."""
    pat = np.random.default_rng(seed).permutation(256)[:d].astype(np.uint8)
    return np.resize(pat, L).astype(np.uint8)


def shape_cases(name, E, m):
    """Every recipe that fits a block of m elements, as Cases."""
    L = m * E
    out = []
    for rname, feats, claims in recipes(L, E):
        try:
            s, parse = craft(L, E, feats, zlib.crc32(("%s/%s" % (name, rname)).encode()))
        except Infeasible:
            continue
        out.append(Case("%s/%s" % (name, rname), s, E, m, parse, claims))
    P = m // 8
    if P in SET_P:
        for x, d in (("P", P), ("2P", 2 * P)):
            if d <= L - 12 - 4:
                out.append(Case("%s/period_%s" % (name, x), periodic(L, E, d, 100 * P + E), E, m,
                                [(d, d, L - 5 - d)], {"set:P=%d:d=%s" % (P, x), "sel:to-end", "last=5"}))
    rnd = np.random.default_rng(zlib.crc32(name.encode())).integers(0, 256, L, dtype=np.uint8)
    out.append(Case("%s/random" % name, rnd, E, m, [], {"last=L"}))
    return out


def partial_cases(name, E, m, m_last):
    """(cases of the full blocks, the partial last block's case): a stream
    whose last block has its own P and a match at exactly that offset."""
    full = [c for c in shape_cases(name, E, m) if c.id.rsplit("/", 1)[1] in ("onlyP", "tie_3_P", "random")]
    L = m_last * E
    P, dP, d2P = far_offsets(L, E)
    feats = [(dP, {dP: 6}), (P + 43, {3: 7}), (2 * P + 40, {3: 10, dP: 10}), (2 * P + 160, {d2P: 9, 1: 4})]
    s, parse = craft(L, E, feats, zlib.crc32(name.encode()))
    return full, Case("%s/partial" % name, s, E, m_last, parse,
                      {"mea:only:P", "mea:tie:3=P", "mea:win:2P>smaller", "mea:far-unaligned-P"})


def stream(oracle, cases, m, last=None):
    """The codec's input (raw bytes) whose bit-transposed blocks are the
    cases' blocks, in order, then `last`'s shorter block."""
    E = cases[0].E
    s = np.concatenate([c.s for c in cases] + ([last.s] if last is not None else []))
    return oracle.bitunshuffle(fast_cases.view_e(s, E), m).view(np.uint8).reshape(-1).copy()


# ---- census -------------------------------------------------------------------
def census(s, E, sreg=False):
    """Counter of the events (EVENTS) the parse of block s holds; `sreg`: the
    block is parsed by a register-layout instance (the reg+N events)."""
    s = np.ascontiguousarray(s, dtype=np.uint8).reshape(-1)
    L = s.size
    ev = collections.Counter()
    if L < 13:
        return ev
    seqs = fast_model.parse(s, E)
    P, dP, d2P = far_offsets(L, E)
    D = fast_model.offsets(L, E)
    runs = {d: fast_model._capped_runs(s, d) for d in D}
    best = np.max(np.stack([runs[d] for d in D]), axis=0)
    startbit = best >= 4
    startbit[0] = False
    startbit[L - 11:] = False
    nw = (L + 31) // 32
    ip, prev_d, prev_len = 1, 0, 0
    for i, (a, ll, d, ml) in enumerate(seqs):
        if d == 0:
            if ll in LAST_EVENTS:
                ev["last=%d" % ll] += 1
            if ll == L:
                ev["last=L"] += 1
                if int(best[1:L - 11].max()) == 3:
                    ev["sel:run3-none"] += 1
            if ll >= 16335:
                ev["last>=16335"] += 1
            if a <= L - 11 and best[L - 11] >= 4:
                ev["sel:L-11-only"] += 1
            break
        p = a + ll
        e = p + ml
        wip, wp, we = ip >> 5, p >> 5, e >> 5
        if ll in LL_EVENTS:
            ev["ll=%d" % ll] += 1
        if ml in ML_EVENTS:
            ev["ml=%d" % ml] += 1
        # selection
        if p == 1:
            ev["sel:p=1"] += 1
        if p == L - 12 and ml in (4, 7):
            ev["sel:p=L-12:len%d" % ml] += 1
        if e == L - 5 and np.array_equal(s[e:], s[e - d:L - d]):
            ev["sel:to-end"] += 1
        if ml == 4 and p % 32 >= 29:
            ev["sel:carry%d" % (p % 32)] += 1
        if p % 32 in (0, 31):
            ev["sel:p%%32=%d" % (p % 32)] += 1
        if i and prev_len >= 8 and ip % 32 and wp == wip and p > ip and startbit[32 * wip:ip].any():
            ev["sel:stale"] += 1
        if i and ll == 0 and d != prev_d:
            ev["sel:ll0-other-offset"] += 1
        gap = wp - wip
        if gap in (7, 8, 63, 64):
            ev["sel:gap=%dw" % gap] += 1
        if gap >= 128:
            ev["sel:gap>=128w"] += 1
        elif gap >= 64:
            ev["sel:gap>=64w"] += 1
        if sreg and (wp >> 6) - (wip >> 6) in (1, 2):
            ev["sel:reg+%d" % ((wp >> 6) - (wip >> 6))] += 1
        if wp == nw - 1:
            ev["sel:last-word"] += 1
        # measure: rounds of 8 words from ip's word (the speculative window) when
        # p lies within 8 words of it, else from p's word
        wb = wip if wp < wip + 8 else wp
        rnd = (we - wb) // 8
        if we == wp:
            ev["mea:end-in-start-word"] += 1
        if e % 32 == 0:
            ev["mea:end%32=0"] += 1
        if rnd == 1:
            ev["mea:round2"] += 1
        elif rnd >= 2:
            ev["mea:round3"] += 1
        me = slot_name(L, E, d)
        others = {x: int(runs[x][p]) for x in D if x != d and runs[x][p] >= 4}
        for x, n in others.items():
            if n < ml:
                ev["mea:win:%s>%s" % (me, "smaller" if x < d else "larger")] += 1
                if (((p + n) >> 5) - wb) // 8 != rnd:  # the loser's run ends in an earlier round
                    ev["mea:two-rounds"] += 1
            elif n == ml and (me, slot_name(L, E, x)) in TIES:
                ev["mea:tie:%s=%s" % (me, slot_name(L, E, x))] += 1
        if p == d and not others and me in ("8", "P", "2P"):
            ev["mea:only:%s" % me] += 1
        if me in ("P", "2P") and P % 4:
            ev["mea:far-unaligned-P"] += 1
        if P in SET_P and d in (P, 2 * P):
            ev["set:P=%d:d=%s" % (P, "P" if d == P else "2P")] += 1
        ip, prev_d, prev_len = e, d, ml
    return ev


def census_table(rows):
    """Markdown table of {column: Counter}: one line per event of EVENTS that any column holds."""
    cols = list(rows)
    out = ["| event | " + " | ".join(cols) + " |", "|---|" + "---|" * len(cols)]
    for e in EVENTS:
        if any(rows[c][e] for c in cols):
            out.append("| `%s` | " % e + " | ".join(str(rows[c][e] or "–") for c in cols) + " |")
    return "\n".join(out)


# ---- a kernel's payload, for the GPU test's reports ---------------------------
def sequences(payload):
    """[(literal length, offset, match length)] of an LZ4 block payload (the
    last with offset 0); stops quietly at a malformed end."""
    b = bytes(payload)
    i, out = 0, []
    while i < len(b):
        tok = b[i]
        i += 1
        ll = tok >> 4
        if ll == 15:
            while i < len(b) and b[i] == 255:
                ll += 255
                i += 1
            ll += b[i] if i < len(b) else 0
            i += 1
        i += ll
        if i >= len(b):
            out.append((ll, 0, 0))
            break
        d = b[i] | (b[i + 1] << 8) if i + 1 < len(b) else -1
        i += 2
        ml = (tok & 15) + 4
        if tok & 15 == 15:
            while i < len(b) and b[i] == 255:
                ml += 255
                i += 1
            ml += b[i] if i < len(b) else 0
            i += 1
        out.append((ll, d, ml))
    return out
