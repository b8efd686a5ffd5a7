"""An instrumented serial restatement of LZ4's greedy parse
(LZ4_compress_default: acceleration 1, no dictionary) for one block, for the
tests of the encoder's SEARCH side (tests/search_cases.py,
test_search_cases.py, test_gpu_search_cases.py).  Test infrastructure only.

Below 65,547 bytes the table is byU16 / hash4; from 65,547 bytes it is byU32 /
hash5 with the 65,535 distance check (lz4/lz4.c:710, 777-795).  `parse`
returns the sequences [(ip, offset, literals, match length)] -- the form of
tests.emit_model.parse_record, against which every user checks them -- and one
event record per search match, per re-test hit, per search that ran out and
per candidate rejected for its distance.  The events name what the kernel
(csrc/lz4_encode.hip) does differently for them:

search match (kind "search")
  p0, k, window = k // 64, lane = k % 64: the search's start and the probe
      index of the hit; the kernel resolves 64 probes per window, so `lane` is
      js, the lane whose insert is the last one that counts.
  step: the stride from probe k to probe k + 1 (1 up to probe 64, 2 from
      probe 65 on, ...).
  valid: the valid lanes of the hit's window (64: a full window, the asm
      search_chain; less: the partial window, kPcPartial); last_valid: the hit
      is that window's last valid lane; at_limit: mpos == limit - 1.
  back, stop: the catch-up and what ended it ("mismatch", "anchor", "zero":
      match == 0).  back >= 64 is search_entry's back = -1 (the continuation
      loop behind it, catch_and_count's twin of it, parse_chain's kPcEntry).
  count: equal bytes from the probe position mpos (>= 4); count >= 256 is the
      other way into kPcEntry and the `while (c0 == kWinBytes)` loop.
re-test hit (kind "retest")
  count: equal bytes from ip; count >= 256 is kPcLong / kRtLong.
  at_limit: ip == limit - 1.
both
  ml, lit, off, at_mlimit (the match ended at mlimit), end_limit (ip >= limit
  after the sequence: kPcLimit), and
  slow: the NEXT re-test takes kPcSlow / kRtSlow.  retest_chain
  (BSHUF_RETEST_ASM) and parse_chain decide it the same way:

        "s_sub_u32 %[t0], %[ip], %[tb]\n\t"
        "s_sub_u32 %[t1], %[t0], 2\n\t"
        "s_cmp_gt_u32 %[t1], 249\n\t"
        "s_cbranch_scc1 L_slow%=\n\t"
  and   "s_sub_u32 %[t1], %[mc], 2\n\t"        (mc = ip - tb there)
        "s_cmp_gt_u32 %[t1], 249\n\t"
        "s_cbranch_scc1 L_slow%=\n\t"

  ip is the position behind the sequence and tb the base of the LAST 256-byte
  count window, whose a-side dwords the wave still holds: the re-test reads
  ip - 2 .. ip + 3 from them, which needs 2 <= ip - tb <= 251.  The predicate
  is `slow_pred(tb, ip)`: (ip - tb - 2) mod 2^32 > 249.  The count windows
  start at the count's origin o (mpos for a search match counted by
  search_entry, ip for a re-test) and a window that is equal throughout hands
  on to the next, so tb = o + 256 * ((ip_after - o) // 256): `slow` holds for
  counts of 252..257, 508..513, ... from o.  (catch_and_count, which finishes
  kPcEntry and kPcPartial matches, counts from mpos + 4; `slow_cc` is the
  predicate with that origin.)
"far" events (wide blocks only)
  a candidate rejected by `cand + 65535 < pos`, in the search or in the
  re-test, with `equal`: its 4 bytes match, the only case in which the check
  decides.  Search matches and re-test hits carry far65535: the distance is
  exactly 65,535.
"runout"
  a search that ran past limit: k, window, and valid = k % 64, the valid
  lanes of the window it ended in.

With traffic=True a search match also carries what the kernel's undo of the
window's later inserts must get right (`if (lane > js && cand <= mpos)
T.put(h, cand)`).  For every valid lane behind js: the entry V the slot must
hold when the window is done -- an entry older than the window ("old") or the
position of a lane <= js of the same window ("inwin") -- how many later
lanes hold the slot (`lanes`), and, after the parse, whether the entry is
OBSERVED: read by a later get before the serial parse's next put to
that slot, and DECIDING: that read finds equal bytes (within the distance),
so a wrong restore changes a sequence.  Lanes <= js that share a slot are
reported as same-slot groups with equal or different bytes, and a slot held
by lanes on both sides of js as a spanning group: (lanes <= js, lanes > js,
all bytes different).
"""
from bisect import bisect_right

K4 = 2654435761
K5 = 889523592379
MINMATCH, MFLIMIT, LASTLITERALS, MIN_LENGTH = 4, 12, 5, 13
WIDE_LIMIT = 65536 + MFLIMIT - 1      # LZ4_64Klimit: 65,547
MAX_DISTANCE = 65535
WAVE, WIN_BYTES = 64, 256


def probe_offset(k):
    """Offset of probe k from the search's start (the skip schedule of
    lz4/lz4.c:1042-1101 at acceleration 1)."""
    if k < 2:
        return k
    t = 62 + k
    q, r = t >> 6, t & 63
    return 1 + 32 * q * (q - 1) + q * (r + 1)


def slow_pred(tb, ip):
    return ((ip - tb - 2) & 0xFFFFFFFF) > 249


def hash4(b, p):
    return ((int.from_bytes(b[p:p + 4], "little") * K4) & 0xFFFFFFFF) >> 19


def hash5(b, p):
    return (((int.from_bytes(b[p:p + 8], "little") << 24) * K5) & 0xFFFFFFFFFFFFFFFF) >> 52


def parse(block, traffic=False):
    """-> (seqs, last-literals anchor, events)."""
    b = bytes(block)
    n = len(b)
    wide = n >= WIDE_LIMIT
    hp = hash5 if wide else hash4
    tab = {}
    log = []            # (op, slot, position): every table access, in order
    seqs, ev, pending = [], [], []
    anchor = 0
    if n < MIN_LENGTH:
        return seqs, anchor, ev
    limit, mlimit = n - MFLIMIT + 1, n - LASTLITERALS

    def close(e, origin, ip0, match, a):
        ml = a - ip0
        e.update(ip=ip0, off=ip0 - match, ml=ml, count=a - origin, at_mlimit=a == mlimit,
                 end_limit=a >= limit, far65535=ip0 - match == MAX_DISTANCE)
        e["tb"] = origin + WIN_BYTES * ((a - origin) // WIN_BYTES)
        e["slow"] = not e["end_limit"] and slow_pred(e["tb"], a)
        if e["kind"] == "search":
            o = origin + MINMATCH
            e["slow_cc"] = not e["end_limit"] and slow_pred(o + WIN_BYTES * ((a - o) // WIN_BYTES), a)
        ev.append(e)

    tab[hp(b, 0)] = 0
    log.append(("p", hp(b, 0), 0))
    ip = 1
    while True:
        p0, k = ip, 0
        fwd, step, nbm = ip, 1, 64
        while True:
            cur = fwd
            h = hp(b, cur)
            cand = tab.get(h, 0)
            log.append(("g", h, cur))
            ip = fwd
            fwd += step
            step = nbm >> 6
            nbm += 1
            if fwd > limit:
                ev.append(dict(kind="runout", p0=p0, k=k, window=k // WAVE, valid=k % WAVE))
                return seqs, anchor, ev + _resolve(b, wide, log, pending)
            tab[h] = cur
            log.append(("p", h, cur))
            eq = b[cand:cand + 4] == b[cur:cur + 4]
            if wide and cand + MAX_DISTANCE < cur:
                ev.append(dict(kind="far", where="search", pos=cur, cand=cand, equal=eq))
            elif eq:
                match = cand
                break
            k += 1
        mpos, mref = ip, match
        e = dict(kind="search", p0=p0, k=k, window=k // WAVE, lane=k % WAVE, step=step, mpos=mpos,
                 mref=mref, at_limit=mpos == limit - 1)
        # the valid lanes of the hit's window
        k0 = k - k % WAVE
        nv = 0
        while nv < WAVE and p0 + probe_offset(k0 + nv + 1) <= limit:
            nv += 1
        e["valid"] = nv
        e["last_valid"] = nv < WAVE and k % WAVE == nv - 1
        if traffic:
            pending.append(_window_traffic(b, hp, tab, e, p0, k0, k % WAVE, nv, len(log)))
        while ip > anchor and match > 0 and b[ip - 1] == b[match - 1]:
            ip -= 1
            match -= 1
        e["back"] = mpos - ip
        e["stop"] = "anchor" if ip == anchor else "zero" if match == 0 else "mismatch"
        origin = mpos
        while True:
            a, c = ip + 4, match + 4
            while a < mlimit and b[a] == b[c]:
                a += 1
                c += 1
            e["lit"] = ip - anchor
            seqs.append((ip, ip - match, ip - anchor, a - ip))
            close(e, origin, ip, match, a)
            slow = e["slow"]
            ip = anchor = a
            if ip >= limit:
                return seqs, anchor, ev + _resolve(b, wide, log, pending)
            h = hp(b, ip - 2)
            tab[h] = ip - 2
            log.append(("p", h, ip - 2))
            h = hp(b, ip)
            cand = tab.get(h, 0)
            log.append(("g", h, ip))
            tab[h] = ip
            log.append(("p", h, ip))
            eq = b[cand:cand + 4] == b[ip:ip + 4]
            if wide and cand + MAX_DISTANCE < ip:
                ev.append(dict(kind="far", where="retest", pos=ip, cand=cand, equal=eq))
                eq = False
            ev.append(dict(kind="retest_try", ip=ip, hit=eq, slow=slow))
            if not eq:
                break
            match, origin = cand, ip
            e = dict(kind="retest", at_limit=ip == limit - 1, was_slow=slow)
        ip += 1


def _window_traffic(b, hp, tab, e, p0, k0, js, nv, at):
    """The table entries the undo of lanes js + 1 .. nv - 1 must leave, and the
    same-slot groups among lanes 0 .. js."""
    win_lo = p0 + probe_offset(k0)
    later = []
    for lane in range(js + 1, nv):
        pos = p0 + probe_offset(k0 + lane)
        h = hp(b, pos)
        later.append((lane, h, tab.get(h, 0)))
    slots = [h for _, h, _ in later]
    groups = {}
    for lane in range(js + 1):
        pos = p0 + probe_offset(k0 + lane)
        groups.setdefault(hp(b, pos), []).append(pos)
    same = []
    for h, ps in groups.items():
        if len(ps) > 1:
            same.append(dict(slot=h, lanes=len(ps), equal=len({b[p:p + 4] for p in ps}) < len(ps),
                             different=len({b[p:p + 4] for p in ps}) > 1))
    e["same_slot"] = same
    # groups with lanes on both sides of js: (lanes <= js, lanes > js, bytes differ)
    span = {}
    for _, h, _ in later:
        if h in groups:
            span[h] = span.get(h, 0) + 1
    e["spanning"] = [dict(slot=h, before=len(groups[h]), after=k,
                          different=len({b[p:p + 4] for p in groups[h]} |
                                        {b[p0 + probe_offset(k0 + l):p0 + probe_offset(k0 + l) + 4]
                                         for l, hh, _ in later if hh == h}) == len(groups[h]) + k)
                     for h, k in span.items()]
    e["restores"] = []
    return e, at, win_lo, [(lane, h, v, slots.count(h)) for lane, h, v in later]


def _resolve(b, wide, log, pending):
    """Fill in which restored entries are observed / deciding."""
    if not pending:
        return []
    by_slot = {}
    for i, (op, h, pos) in enumerate(log):
        by_slot.setdefault(h, []).append(i)
    for e, at, win_lo, later in pending:
        seen = set()
        for lane, h, v, shared in later:
            if h in seen:       # one entry per slot: its first later lane restores it
                continue
            seen.add(h)
            idx = by_slot.get(h, [])
            j = bisect_right(idx, at - 1)
            observed = deciding = False
            if j < len(idx) and log[idx[j]][0] == "g":
                observed = True
                r = log[idx[j]][2]
                deciding = b[v:v + 4] == b[r:r + 4] and not (wide and v + MAX_DISTANCE < r)
            e["restores"].append(dict(lane=lane, value=v, origin="inwin" if v >= win_lo else "old",
                                      lanes=shared, observed=observed, deciding=deciding))
    return []


def census(events):
    """A summary of a list of events: the sets and counts the tests ask for."""
    s = [e for e in events if e["kind"] == "search"]
    r = [e for e in events if e["kind"] == "retest"]
    out = dict(
        backs={e["back"] for e in s},
        back_stop={(e["back"], e["stop"]) for e in s},
        hits={(e["window"], e["lane"]) for e in s},
        probes={e["k"] for e in s},
        search_counts={e["count"] for e in s},
        retest_counts={e["count"] for e in r},
        runout_valid={e["valid"] for e in events if e["kind"] == "runout"},
        far={(e["where"], e["equal"]) for e in events if e["kind"] == "far"},
        n_far=sum(e["kind"] == "far" for e in events),
        far65535={e["kind"] for e in s + r if e["far65535"]},
        offsets={e["off"] for e in s + r},
        slow_retests=sum(e["kind"] == "retest_try" and e["slow"] for e in events),
        slow_retest_hits=sum(e["was_slow"] for e in r),
        restores={(x["origin"], x["lanes"], x["observed"], x["deciding"])
                  for e in s for x in e.get("restores", ())},
        same_slot={(g["lanes"], g["equal"], g["different"]) for e in s for g in e.get("same_slot", ())},
        spanning={(g["before"], g["after"], g["different"]) for e in s for g in e.get("spanning", ())},
    )
    return out


def shuffled_blocks(oracle, arr, block=0):
    """The shuffled blocks the codec parses for `arr` (the last may be shorter;
    the elements behind the last multiple of 8 are stored raw)."""
    import numpy as np
    E = arr.dtype.itemsize
    be = block or oracle.default_block_size(E)
    n = arr.size - arr.size % 8
    sh = oracle.bitshuffle(arr, block).view(np.uint8).reshape(-1)
    return [sh[i * E:min(i + be, n) * E] for i in range(0, n, be)]


def summary(events):
    """The figures of the pull request's table, from a list of events."""
    c = census(events)
    s = [e for e in events if e["kind"] == "search"]
    r = [e for e in events if e["kind"] == "retest"]
    return dict(
        matches=len(s), retest_hits=len(r), longest_back=max(c["backs"] or {0}),
        back_ge_64=sum(e["back"] >= 64 for e in s),
        back_to_anchor=sum(e["stop"] == "anchor" and e["back"] > 0 for e in s),
        back_to_zero=sum(e["stop"] == "zero" for e in s),
        hit_windows=sorted({e["window"] for e in s})[-3:],
        partial_window_hits=sum(e["valid"] < WAVE for e in s),
        search_count_ge_256=sum(e["count"] >= WIN_BYTES for e in s),
        retest_count_ge_256=sum(e["count"] >= WIN_BYTES for e in r),
        slow_retests=c["slow_retests"],
        far_equal_search=sum(e["kind"] == "far" and e["where"] == "search" and e["equal"] for e in events),
        far_equal_retest=sum(e["kind"] == "far" and e["where"] == "retest" and e["equal"] for e in events),
        far_65535=sum(e["far65535"] for e in s + r),
        deciding_restores=sum(x["deciding"] for e in s for x in e.get("restores", ())),
        deciding_restores_inwin=sum(x["deciding"] and x["origin"] == "inwin" for e in s for x in e.get("restores", ())),
        deciding_restores_shared=sum(x["deciding"] and x["lanes"] > 1 for e in s for x in e.get("restores", ())),
    )


if __name__ == "__main__":
    # the census of the generic inputs of tests/test_gpu_parity.py (the matrix of
    # test_lz4_matches_oracle with fixed seeds, 40 default blocks of G1 and G2)
    import os
    import sys
    import numpy as np
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from oracle import Oracle
    o = Oracle()
    ev, nblocks = [], 0
    for ki, kind in enumerate(["random", "runs", "periodic", "walk", "zeros"]):
        rng = np.random.default_rng(1000 + ki)
        for E in [1, 2, 4, 8, 3, 12]:
            for n in [1, 8, 13, 64, 200, 1000, 5000, 40000]:
                nbytes = n * E
                d = {"random": lambda: rng.integers(0, 256, nbytes, dtype=np.uint8),
                     "runs": lambda: np.repeat(rng.integers(0, 4, nbytes // 7 + 1), 7)[:nbytes].astype(np.uint8),
                     "periodic": lambda: (np.arange(nbytes) % (1 + (n % 13)) * 29).astype(np.uint8),
                     "walk": lambda: (rng.integers(-2, 3, nbytes).cumsum() % 256).astype(np.uint8),
                     "zeros": lambda: np.zeros(nbytes, dtype=np.uint8)}[kind]()
                arr = d.view({1: np.uint8, 2: np.int16, 4: np.int32, 8: np.int64}[E]) if E in (1, 2, 4, 8) \
                    else d.view(np.dtype("V%d" % E))
                for block in [0, 64, 8]:
                    for b in shuffled_blocks(o, arr, block):
                        ev += parse(b, traffic=True)[2]
                        nblocks += 1
    for gen in (o.gen_g1, o.gen_g2):
        a = gen(40 * o.default_block_size(gen(8).dtype.itemsize))
        for b in shuffled_blocks(o, a):
            ev += parse(b, traffic=True)[2]
            nblocks += 1
    print(nblocks, "blocks")
    for k, v in summary(ev).items():
        print("%-28s %s" % (k, v))
