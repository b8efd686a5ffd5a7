"""Shuffled blocks that hold chosen events of the LZ4 encoder's SEARCH: where a
match is found, how far it is caught up, which table entry a lane sees
(tests/test_search_cases.py, test_gpu_search_cases.py).  Test infrastructure
only; the companion of tests/emit_cases.py for the parse's input side.

A block is built in the SHUFFLED domain from random bytes (which the parse
walks with its skip schedule, finding nothing) and planted copies, and the
codec's input comes from the oracle's bitunshuffle.  Where a probe lands is
never taken on trust: a builder proposes a layout from the probe schedule
(parse_census.probe_offset), the instrumented serial parse
(tests/parse_census.py) says what it holds, and the builder moves the copy or
draws other bytes until the census shows the event (`tune`).  The CPU test
then asserts every family's census again, and that the serial parse is the
oracle's.

Three building blocks:
  * a DICTIONARY at the block start: the first search inserts positions 0..65
    one by one, so any 4 bytes of it are a live table entry;
  * a RESET: a 6-byte copy of a dictionary piece (found at any step <= 3), or
    a run of one byte value (found at any step below its length / 2): behind
    the match the next search starts over at step 1, so the bytes behind a
    reset are probed one by one, probe k at offset k;
  * same-hash quads: 4-byte values with equal hash4 and different bytes, found
    by drawing random values.

Families (the source lines each reaches: DESIGN.md 4.1c):
  A  catch-up lengths          B  probe schedule and the block end
  C  table traffic in a window D  count-window edges
  E  wide blocks: the 65,535 distance rule, the byU16 / byU32 boundary
"""
import functools

import numpy as np

from tests.parse_census import MAX_DISTANCE, census, hash4, parse, probe_offset

A_BACKS = [1, 2, 3, 62, 63, 64, 65, 66, 127, 128, 129]
D_COUNTS = list(range(250, 263)) + list(range(506, 519))
E_DISTANCES = [65534, 65535, 65536, 65537, 70000]


def events(block, traffic=False):
    return parse(block, traffic)[2]


def searches(ev):
    return [e for e in ev if e["kind"] == "search"]


def block_bytes(oracle, E, want=None):
    """The default block's byte size, or the largest multiple of 8 elements <= want."""
    if want is None:
        return oracle.default_block_size(E) * E
    return want // (8 * E) * 8 * E


def same_hash_sets(rng, size, count):
    """`count` disjoint sets of `size` 4-byte values with equal hash4."""
    buckets, out, used = {}, [], set()
    while len(out) < count:
        q = rng.integers(0, 256, 4, dtype=np.uint8)
        h = hash4(q.tobytes(), 0)
        g = buckets.setdefault(h, [])
        if h in used or any(q.tobytes() == x.tobytes() for x in g):
            continue
        g.append(q)
        if len(g) == size:
            out.append(g)
            used.add(h)         # one set per hash value
    return out


def tune(build, ok, tries=40):
    """build(t) for t = 0, 1, ... until ok(events) holds; -> the block."""
    for t in range(tries):
        blk = build(t)
        if blk is None:
            continue
        if ok(events(blk, traffic=True)):
            return blk
    raise AssertionError("no layout holds the event")


# --------------------------------------------------------------------------
# A. catch-up length
# --------------------------------------------------------------------------
def _probed(n):
    """Positions a search from the block start probes while it finds nothing."""
    out, k = set(), 0
    while 1 + probe_offset(k) < n:
        out.add(1 + probe_offset(k))
        k += 1
    return out


def _copy_block(base, s, d, L):
    b = base.copy()
    b[d:d + L] = b[s:s + L]
    if s > 0:
        b[d - 1] = b[s - 1] ^ 0x5A
    b[d + L] = b[s + L] ^ 0x5A
    return b


def _first_back(ev, d, L):
    for e in searches(ev):
        if d <= e["mpos"] < d + L:
            return e
    return None


@functools.lru_cache(maxsize=None)
def catchup_cases(n, seed=11):
    """A random n-byte block per catch-up length of A_BACKS and one >= 192,
    each with a 600-byte copy of an earlier slice that the search finds `back`
    bytes into the copy (the catch-up ends on a mismatch); the copies are long,
    so back >= 64 comes with a count >= 256.  -> [(block, back)]."""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, n, dtype=np.uint8)
    P, L = _probed(n), 600
    want = {t: None for t in A_BACKS + [192]}
    for s in [s0 + i for s0 in (1800, 600, 3000) for i in range(13)]:
        xs = [x for x in range(L - 8) if s + x in P]
        for d in range(s + L + 40, n - L - 40):
            x = next((x for x in xs if d + x in P), None)   # proposal: first probe that sees an insert
            if x is None:
                continue
            t = x if x in want else 192 if x >= 192 else None
            if t is None or want[t] is not None:
                continue
            blk = _copy_block(base, s, d, L)
            e = _first_back(events(blk), d, L)
            if e and e["stop"] == "mismatch" and (e["back"] == t or (t == 192 and e["back"] >= 192)):
                want[t] = (blk, e["back"])
        if all(v is not None for v in want.values()):
            break
    missing = [t for t, v in want.items() if v is None]
    assert not missing, missing
    return [want[t] for t in sorted(want)]


@functools.lru_cache(maxsize=None)
def block_start_case(n, seed=12):
    """A copy of the block's first bytes: the catch-up stops at position 0
    (match == 0).  The block start is inserted position by position, so the
    catch-up is shorter than the step in force at the copy: the longest the
    layout gives is taken.  -> (block, back)."""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, n, dtype=np.uint8)
    P, L, best = _probed(n), 200, None
    for d in range(n - L - 40, n // 2, -1):
        x = next(x for x in range(64) if d + x in P)
        if best is None or x > best[0]:
            best = (x, d)
    blk = _copy_block(base, 0, best[1], L)
    e = _first_back(events(blk), best[1], L)
    assert e and e["stop"] == "zero", e
    return blk, e["back"]


@functools.lru_cache(maxsize=None)
def anchor_cases(n, seed=13):
    """Catch-ups that end at the anchor: the search match gives a sequence
    without literals.  A 16-byte run of one value at 700 is a reset; the copy
    starts where the run's match ends.  Its source lies at 400.., where the
    first search inserted every fourth position: when the source's first quad
    is no table entry the re-test misses, and the search's first hit comes at
    the first inserted position, `back` <= 3 probes later.

    A catch-up of 63, 64 or 65 bytes to the anchor needs that many positions
    in a row without a live entry in front of a live one, which the steps of an
    8 KiB block (15 at the most) do not leave by themselves.  So the source's
    inserted positions in front of the live one are overwritten: for each of
    them a quad of the same hash4 and other bytes stands at a later position
    that the first search probes.  -> [(block, back)] for 1, 2, 3, 63, 64, 65."""
    out = []
    for back in (1, 2, 3):
        def build(t, back=back):
            rng = np.random.default_rng(seed + back)
            b = rng.integers(0, 256, n, dtype=np.uint8)
            b[700:716] = 0xE7
            b[699] = b[716] = 0x11
            s = 400 + t
            b[716:716 + 40] = b[s:s + 40]
            b[756] = b[s + 40] ^ 0x5A
            return b

        blk = tune(build, lambda ev, back=back: (back, "anchor") in census(ev)["back_stop"])
        out.append((blk, back))
    P = sorted(_probed(n))
    for back in (63, 64, 65):
        def build(t, back=back):
            rng = np.random.default_rng(seed + back + 1000 * t)
            b = rng.integers(0, 256, n, dtype=np.uint8)
            e = next(p for p in P if p >= 1800 + back and p - back not in P)
            s = e - back
            live = [p for p in P if s < p < e]
            Z = [p for p in P if p >= e + 200]
            for i, p in enumerate(live):
                h = hash4(b.tobytes(), p)
                while True:
                    q = rng.integers(0, 256, 4, dtype=np.uint8)
                    if hash4(q.tobytes(), 0) == h and q.tobytes() != b[p:p + 4].tobytes():
                        break
                b[Z[2 * i]:Z[2 * i] + 4] = q
            r = Z[2 * len(live)] + 40
            b[r:r + 40] = 0xE7
            b[r - 1] = 0x11
            if b[s] == 0xE7:
                return None
            b[r + 40:r + 60 + back] = b[s:s + 20 + back]
            b[r + 60 + back] = b[s + 20 + back] ^ 0x5A
            return b

        blk = tune(build, lambda ev, back=back: (back, "anchor") in census(ev)["back_stop"], tries=8)
        out.append((blk, back))
    return out


# --------------------------------------------------------------------------
# B. probe schedule and the block end
# --------------------------------------------------------------------------
B_PROBES = [4 * 64 + 62, 0, 1, 62, 63, 64, 65, 126, 127, 128, 129, 190, 191, 256, 257, 319]


@functools.lru_cache(maxsize=None)
def probe_cases(n, seed=21):
    """One block whose searches hit at the probes of B_PROBES: lanes 0, 1, 62,
    63 of windows 0, 1, 2 and 4.  Every hit is a 6-byte copy of a dictionary
    piece; behind it the next search starts over."""
    def build(t):
        rng = np.random.default_rng(seed + t)
        b = rng.integers(0, 256, n, dtype=np.uint8)
        p0 = 1
        for i, k in enumerate(B_PROBES):
            pos = p0 + probe_offset(k)
            src = 4 * (i % 15) + 1
            if pos + 8 >= n - 16:
                return None
            b[pos:pos + 6] = b[src:src + 6]
            b[pos - 1] = b[src - 1] ^ 0x5A
            b[pos + 6] = b[src + 6] ^ 0x5A
            p0 = pos + 7
        return b

    return tune(build, lambda ev: set(B_PROBES) <= census(ev)["probes"])


def _filled(rng, n, a):
    """64 random bytes, repeated with period 64 up to position a: one match
    from 64 to a, behind which the search starts over at a + 1."""
    b = rng.integers(0, 256, n, dtype=np.uint8)
    for i in range(64, a):
        b[i] = b[i - 64]
    b[a] = b[a - 64] ^ 0x5A
    return b


@functools.lru_cache(maxsize=None)
def block_end_cases(n, seed=22):
    """name -> block, for the events at the block end (limit = n - 11,
    mlimit = n - 5)."""
    limit, mlimit = n - 11, n - 5
    out = {}

    def runout(valid, window):
        def build(t):
            k = 64 * window + valid            # the first probe past the limit
            return _filled(np.random.default_rng(seed + t), n, limit - probe_offset(k) - 1)
        return tune(build, lambda ev: any(e["kind"] == "runout" and e["valid"] == valid and
                                          e["window"] == window for e in ev))

    out["runout_1"] = runout(1, 1)
    out["runout_1_w0"] = runout(1, 0)
    out["runout_63"] = runout(63, 0)

    def hit_at_limit(t):
        b = _filled(np.random.default_rng(seed + 50 + t), n, limit - 11)
        b[limit - 1:limit + 3] = b[8:12]
        b[limit - 2] = b[7] ^ 0x5A
        b[limit + 3] = b[12] ^ 0x5A
        return b
    out["hit_at_limit"] = tune(hit_at_limit, lambda ev: any(
        e["at_limit"] and e["last_valid"] and e["valid"] == 10 for e in searches(ev)))

    def last_lane_w1(t):
        # the partial window is window 1 (step 2): its last valid probe
        b = _filled(np.random.default_rng(seed + 60 + t), n, limit - probe_offset(64 + 20) - 1)
        pos = limit - probe_offset(64 + 20) + probe_offset(64 + 19)
        b[pos:pos + 4] = b[8:12]
        b[pos - 1] = b[7] ^ 0x5A
        return b
    out["last_lane_w1"] = tune(last_lane_w1, lambda ev: any(
        e["last_valid"] and e["window"] == 1 for e in searches(ev)))

    def to_mlimit(short):
        def build(t):
            b = _filled(np.random.default_rng(seed + 70 + t), n, limit - 30)
            pos = limit - 24
            b[pos:] = b[8:8 + n - pos]
            b[pos - 1] = b[7] ^ 0x5A
            if short:
                b[mlimit - 1] ^= 0x5A
            return b
        return tune(build, lambda ev: any(e["ip"] + e["ml"] == mlimit - short for e in searches(ev)))

    out["ends_at_mlimit"] = to_mlimit(0)
    out["ends_at_mlimit_1"] = to_mlimit(1)

    def retest_at_limit(hit):
        def build(t):
            b = _filled(np.random.default_rng(seed + 80 + t), n, limit - 1)
            if hit:
                j = 20 if b[20] != b[(limit - 1) % 64] else 24
                b[limit - 1:limit + 5] = b[j:j + 6]
            return b
        return tune(build, lambda ev: any(e["kind"] == "retest_try" and e["ip"] == limit - 1 and
                                          e["hit"] == hit for e in ev))

    out["retest_at_limit_miss"] = retest_at_limit(False)
    out["retest_at_limit_hit"] = retest_at_limit(True)
    return out


@functools.lru_cache(maxsize=None)
def tiny_cases(n, seed=23):
    """An n-byte block (16..40) whose only 4-byte repeat sits at limit - 1, the
    last position a search probes, and one whose repeat sits at limit, which no
    probe sees.  -> (seen, unseen)."""
    limit = n - 11

    def build(at):
        def f(t):
            b = np.random.default_rng(seed + n + t).integers(0, 256, n, dtype=np.uint8)
            s = at - 4
            b[at:at + 4] = b[s:s + 4]
            b[at + 4] = b[s + 4] ^ 0x5A
            return b
        return f

    seen = tune(build(limit - 1), lambda ev: any(e["at_limit"] for e in searches(ev)))
    unseen = tune(build(limit), lambda ev: not searches(ev))
    return seen, unseen


# --------------------------------------------------------------------------
# C. table traffic inside the hit's window
# --------------------------------------------------------------------------
class Chain:
    """A block written front to back: a 64-byte dictionary, then segments.
    Each segment starts behind a match, so its bytes are probed one by one:
    `gap(j)` writes the byte the re-test misses on and j random bytes, after
    which the next byte is lane j of the new search's first window."""

    def __init__(self, rng, n, head=None):
        self.rng, self.n = rng, n
        self.b = rng.integers(0, 256, n, dtype=np.uint8)
        if head is not None:
            self.b[:head.size] = head
        self.at = 66
        self.piece = 0
        self.reset()

    def put(self, data, stop=None):
        data = np.asarray(data, dtype=np.uint8)
        assert self.at + data.size + 32 < self.n
        self.b[self.at:self.at + data.size] = data
        self.at += data.size
        if stop is not None:                 # the byte behind must differ from `stop`
            self.b[self.at] = int(stop) ^ 0x5A

    def gap(self, j):
        self.at += 1 + j

    def reset(self):
        """A 6-byte copy of a dictionary piece (pieces at 36, 40, .. 56)."""
        s = 36 + 4 * (self.piece % 6)
        self.piece += 1
        # the byte in front differs from the piece's and from every earlier copy's
        self.b[self.at - 1] = (int(self.b[s - 1]) + 1 + 7 * (self.piece // 6)) & 0xFF
        self.put(self.b[s:s + 6].copy(), stop=self.b[s + 6])

    def hit(self, j):
        """A dictionary hit at lane j of a new search."""
        self.gap(j)
        self.reset()


def _head(rng, quads):
    """Dictionary: 6 random bytes, then the quads 4 random bytes apart."""
    h = rng.integers(0, 256, 64, dtype=np.uint8)
    for i, q in enumerate(quads):
        h[6 + 8 * i:10 + 8 * i] = q
    return h


@functools.lru_cache(maxsize=None)
def window_cases(n, seed=31):
    """Two blocks.  The first holds in-window sources at distances 1, 2, 3, 4
    and 63, one across the window boundary, and the deciding restores of an
    old entry and of an in-window entry; the second holds the same-slot groups:
    two and three lanes before, around and behind js, and later lanes that
    share a restored slot in its deciding form."""
    def first(t):
        rng = np.random.default_rng(seed + t)
        c = Chain(rng, n)
        for dist, j in ((1, 5), (2, 5), (3, 5), (4, 5), (63, 0), (1, 63)):
            c.gap(j)
            u = rng.integers(0, 256, dist, dtype=np.uint8)
            if dist > 1:
                while u[0] == u[-1]:
                    u = rng.integers(0, 256, dist, dtype=np.uint8)
            rep = np.resize(u, dist + 4)
            c.b[c.at - 1] = int(rep[dist - 1]) ^ 0x5A
            c.put(rep, stop=rep[4 % dist] if dist <= 4 else rep[4])
        # an OLD entry restored and then read: a copy of dictionary bytes 8..27
        # at lane 3, then a copy of bytes 13..20 behind the match
        c.gap(3)
        c.b[c.at - 1] = c.b[7] ^ 0x5A
        c.put(c.b[8:28].copy(), stop=c.b[28])
        c.gap(2)
        c.b[c.at - 1] = c.b[12] ^ 0x5A
        c.put(c.b[13:21].copy(), stop=c.b[21])
        # an IN-WINDOW entry restored and then read: 12 fresh bytes twice, then
        # bytes 5..12 of them behind the match
        c.gap(3)
        u = rng.integers(0, 256, 12, dtype=np.uint8)
        q = c.at
        c.put(np.concatenate([u, u]), stop=u[0])
        c.gap(2)
        c.b[c.at - 1] = c.b[q + 4] ^ 0x5A
        c.put(c.b[q + 5:q + 13].copy(), stop=c.b[q + 13])
        return c.b

    def ok_first(ev):
        c = census(ev)
        s = searches(ev)
        dist = {e["off"] for e in s if e["window"] == 0 and e["off"] <= e["lane"]}
        cross = any(e["k"] == 64 and e["off"] == 1 for e in s)
        return ({1, 2, 3, 4, 63} <= dist and cross and
                any(x[0] == "old" and x[2] and x[3] for x in c["restores"]) and
                any(x[0] == "inwin" and x[2] and x[3] for x in c["restores"]))

    def second(t):
        rng = np.random.default_rng(seed + 500 + t)
        sets = same_hash_sets(rng, 3, 8)
        c = Chain(rng, n, _head(rng, sets[0]))
        # later lanes share a restored slot (deciding): a copy of dictionary
        # bytes 4..31 (three same-hash quads), then the last quad again
        c.gap(3)
        c.b[c.at - 1] = c.b[3] ^ 0x5A
        c.put(c.b[4:32].copy(), stop=c.b[32])
        c.gap(2)
        c.b[c.at - 1] = c.b[21] ^ 0x5A
        c.put(c.b[22:30].copy(), stop=c.b[30])
        k = 1
        for size in (2, 3):
            # all before js
            q = sets[k]; k += 1
            c.gap(2)
            for x in q[:size]:
                c.put(x)
                c.at += 2
            c.reset()
            # around js
            q = sets[k]; k += 1
            c.gap(2)
            for x in q[:size - 1]:
                c.put(x)
                c.at += 2
            c.reset()
            c.at += 3
            c.put(q[size - 1])
            c.at += 8
            c.reset()
            # all behind js
            q = sets[k]; k += 1
            c.hit(3)
            c.at += 4
            for x in q[:size]:
                c.put(x)
                c.at += 2
            c.at += 8
            c.reset()
        return c.b

    def ok_second(ev):
        c = census(ev)
        r, g = c["restores"], c["same_slot"]
        return (("old", 3, True, True) in r and ("old", 2, True, False) in r and
                ("old", 3, True, False) in r and {(1, 1, True), (2, 1, True)} <= c["spanning"] and
                (2, False, True) in g and (3, False, True) in g)

    return [tune(first, ok_first), tune(second, ok_second)]


# --------------------------------------------------------------------------
# D. count-window edges
# --------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def count_cases(n, seed=41):
    """Blocks whose search matches and re-test hits count every value of
    D_COUNTS and 4 from their origin.  R = the block's first 600 bytes; a copy
    of R[0:c] three random bytes behind a match is a search hit at its first
    byte (catch-up 0), one straight behind a match is a re-test hit; the
    candidate is the copy before, so the counts go down."""
    groups = [list(range(262, 249, -1)) + [4], list(range(518, 512, -1)), list(range(512, 508, -1)),
              list(range(508, 505, -1))]

    def build(cs):
        def f(t):
            rng = np.random.default_rng(seed + cs[0] + t)
            b = rng.integers(0, 256, n, dtype=np.uint8)
            R = b[:600].copy()
            R[1:][R[1:] == R[0]] ^= 0x5A      # R[0] occurs once: a copy of R[0:c] ends where the next begins
            b[:600] = R
            at = 603
            for gap in (3, 0):
                for c in [cs[0] + 9] + cs:
                    at += gap
                    if gap:
                        b[at - 1] = rng.integers(0, 256)
                        while b[at - 1] in (R[0], R[599]):
                            b[at - 1] ^= 0x33
                    b[at:at + c] = R[:c]
                    at += c
                    b[at] = R[c] ^ 0x5A
                at += 5
            assert at < n - 32, at
            return b
        return f

    out = []
    for cs in groups:
        want = set(cs)
        out.append(tune(build(cs), lambda ev, want=want: want <= census(ev)["search_counts"] and
                        want <= census(ev)["retest_counts"]))
    return out


# --------------------------------------------------------------------------
# E. wide blocks
# --------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def far_case(n, seed=51):
    """A wide block (n >= 96 KiB) with, per distance of E_DISTANCES, a 24-byte
    slice and its copy at that distance, once found by the search and once
    straight behind a match's end (the re-test finds it), each followed by a
    third copy that reads the entry the first copy's probe left.  Every slice
    and copy stands behind a reset (a 200-byte run of one byte value), so it is
    inserted and probed position by position."""
    def build(t):
        rng = np.random.default_rng(seed + t)
        b = rng.integers(0, 256, n, dtype=np.uint8)
        val = 0
        for i, dist in enumerate(E_DISTANCES * 2):
            retest = i >= len(E_DISTANCES)
            s = 1500 + 300 * i
            d = s + dist
            third = d + 9000 + 300 * i
            assert third + 64 < n
            for at, glued in ((s, False), (d, retest), (third, False)):
                val = val % 250 + 1
                g = 0 if glued else 3
                b[at - g - 200:at - g] = val
                b[at - g - 201] = val ^ 0x5A
                if g:
                    b[at - g:at] = rng.integers(0, 256, g)
                    b[at - g] = val ^ 0x5A
            b[d:d + 24] = b[s:s + 24]
            b[third:third + 24] = b[s:s + 24]
            for at in (s, d, third):
                if b[at] == b[at - 1] and (at != d or retest):
                    return None
            b[d + 24] = b[s + 24] ^ 0x5A
            b[third + 24] = b[s + 24] ^ 0xA5
        return b

    def ok(ev):
        c = census(ev)
        return ({("search", True), ("retest", True)} <= c["far"] and
                {"search", "retest"} <= c["far65535"] and
                {65534, 65535} <= c["offsets"])

    return tune(build, ok, tries=6)


@functools.lru_cache(maxsize=None)
def small_far_case(n, dist, retest, seed=53):
    """The smallest wide blocks (65,552 bytes; 65,568 for 3-byte elements)
    hold one far copy each: the search probes up to n - 12, so a copy at
    distance 65,534..65,537 has its source in the block's first bytes (position
    2 here, inserted by the first search's second probe) and stands in the
    block's last 20.  Distance 70,000 and a third copy behind the second do
    not fit in such a block.  The copy stands three random bytes behind a
    200-byte run of one value (the search finds it) or straight behind the run
    (the re-test does)."""
    def build(t):
        rng = np.random.default_rng(seed + dist + 7 * t)
        b = rng.integers(0, 256, n, dtype=np.uint8)
        s, d = 2, 2 + dist
        g = 0 if retest else 3
        b[d - g - 200:d - g] = 0xE7
        b[d - g - 201] = 0x11
        if g:
            b[d - g] = 0x12
        b[d:d + 8] = b[s:s + 8]
        if b[d] == 0xE7 or b[d - 1] == b[s - 1]:
            return None
        b[d + 8] = b[s + 8] ^ 0x5A
        return b

    where = "retest" if retest else "search"

    def ok(ev):
        if dist <= MAX_DISTANCE:
            return any(e["kind"] == where and e["off"] == dist and e["ip"] == 2 + dist for e in ev)
        return any(e["kind"] == "far" and e["where"] == where and e["equal"] and e["cand"] == 2 and
                   e["pos"] == 2 + dist for e in ev)

    return tune(build, ok, tries=8)


@functools.lru_cache(maxsize=None)
def boundary_case(n, seed=52):
    """n = 65,536 .. 65,568: a match whose source lies beyond position 65,000
    and one with an offset above 60,000 (byU16 up to 65,546 bytes: the 16-bit
    entries hold them; wide from 65,547), plus a family-A copy."""
    def build(t):
        rng = np.random.default_rng(seed + t)
        b = rng.integers(0, 256, n, dtype=np.uint8)
        b[5000:5600] = b[1800:2400]
        b[4999] = b[1799] ^ 0x5A
        b[5600] = b[2400] ^ 0x5A
        b[64000:64200] = 9
        b[64203:64227] = b[3200:3224]                 # offset 61,003
        b[64227] = b[3224] ^ 0x5A
        b[65005:65205] = 11
        b[65250:65450] = 13
        b[65453:65473] = b[65208:65228]               # source beyond 65,000
        b[65473] = b[65228] ^ 0x5A
        return b

    def ok(ev):
        s = [e for e in ev if e["kind"] in ("search", "retest")]
        return (any(e["off"] > 60000 for e in s) and any(e["ip"] - e["off"] > 65000 for e in s) and
                any(e["back"] >= 64 for e in searches(ev)))

    return tune(build, ok, tries=6)
