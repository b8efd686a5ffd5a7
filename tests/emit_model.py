"""numpy restatement of the LZ4 encoder's wave-parallel emission
(csrc/lz4_encode.hip, emit_sequences_flat): the addressing of every LDS access
it makes, lane by lane and step by step, so that the owner walk, the dword
composition and the bounds can be checked on the CPU against the oracle's
record.  Test infrastructure only.

The kernel's stages, per batch of 64 sequences (lane = sequence):
  1. prefix sum of the sequences' sizes -> op, the literal run's place lp;
  2. token + the first four literal-length bytes, and offset + the first three
     match-length bytes, as two masked dword writes each; the rest of a longer
     length run (a few lanes per block) by the wave, one run per step;
  3. every literal run's head and tail destination dword as masked writes of
     v_alignbyte(source dword t + 1, source dword t);
  4. interior dwords: runs up to the per-lane size by their own lanes, longer
     ones by the wave, run after run -- up to 64 dwords one per lane, longer
     runs in 16-byte chunks of the destination (two aligned 16-byte source
     reads per chunk, the same dword offset q in every lane) with the <= 3
     dwords in front and behind in a step of their own.  Source reads are
     unmasked (over-read into the LDS behind the block), writes are masked by
     the run's end.
"""
import numpy as np

WAVE = 64
MIN_MATCH = 4
LANE_RUN = 32        # kFlatLaneRun
LANE_RUN_MIN = 4     # kLaneRunMin
PAD = 16 + 2048      # readable LDS behind the block: kDataPad + the descriptors
TABLE = 16384        # kTableBytes: the record's staging area


def parse_record(rec, n):
    """An LZ4 block -> [(ip, off, lit, ml)] and the anchor of the last literals."""
    seqs, p, ip = [], 0, 0
    while True:
        tok = int(rec[p]); p += 1
        lit = tok >> 4
        if lit == 15:
            while True:
                b = int(rec[p]); p += 1
                lit += b
                if b != 255:
                    break
        p += lit
        ip += lit
        if p >= len(rec):
            assert ip == n, (ip, n)
            return seqs, ip - lit
        off = int(rec[p]) | int(rec[p + 1]) << 8
        p += 2
        ml = (tok & 15) + MIN_MATCH
        if (tok & 15) == 15:
            while True:
                b = int(rec[p]); p += 1
                ml += b
                if b != 255:
                    break
        seqs.append((ip, off, lit, ml))
        ip += ml


def ext_bytes(v):
    return (v - 15) // 255 + 1 if v >= 15 else 0


class Lds:
    """Byte array with dword helpers and access bookkeeping."""

    def __init__(self, size):
        self.b = np.zeros(size, dtype=np.uint8)
        self.hi = -1

    def rd32(self, a):
        assert a % 4 == 0 and a >= -4, a
        self.hi = max(self.hi, a + 3)
        if a < 0:          # the dword in front of the block: masked off by the caller
            return 0xDEADBEEF
        assert a + 4 <= self.b.size, (a, self.b.size)
        return int(self.b[a:a + 4].view("<u4")[0])

    def wr32(self, a, v, mask=0xFFFFFFFF):
        assert a % 4 == 0 and 0 <= a and a + 4 <= self.b.size, a
        old = int(self.b[a:a + 4].view("<u4")[0])
        self.b[a:a + 4].view("<u4")[0] = (old & ~mask & 0xFFFFFFFF) | (v & mask)
        self.hi = max(self.hi, a + 3)

    def wr8(self, a, v):
        assert 0 <= a < self.b.size, a
        self.b[a] = v
        self.hi = max(self.hi, a)


def alignbyte(hi, lo, sh):
    return ((hi << 32 | lo) >> (8 * sh)) & 0xFFFFFFFF


def len_run_head(J, cnt, last):
    """The first J bytes of a length run as a little-endian value."""
    if cnt > J:
        return (1 << 8 * J) - 1
    if cnt <= 0:
        return 0
    sh = 8 * (cnt - 1)
    return ((1 << sh) - 1) | last << sh


def put5(S, p, v, nbytes):
    """Up to 5 bytes at p as two masked dword writes."""
    assert 0 <= nbytes <= 5
    sh = 8 * (p & 3)
    m = ((1 << 8 * nbytes) - 1) << sh
    d = (v << sh) & m
    assert m < 1 << 64
    a = p & ~3
    S.wr32(a, d & 0xFFFFFFFF, m & 0xFFFFFFFF)
    S.wr32(a + 4, d >> 32, m >> 32)


def len_rest(S, J, lanes):
    """lanes: [(p, cnt, last)].  Bytes J.. of the runs longer than J, by the wave."""
    for p, cnt, last in lanes:
        if cnt > J:
            for i0 in range(J, cnt, WAVE):
                for lane in range(WAVE):
                    i = i0 + lane
                    if i < cnt:
                        S.wr8(p + i, 255 if i + 1 < cnt else last)


def emit(block, seqs, la, stats=None):
    """The record payload the kernel's emission builds for one parsed block."""
    n = len(block)
    D = Lds(n + PAD)
    D.b[:n] = block
    D.b[n:] = 0xA5        # pad and descriptors: read, never used
    S = Lds(TABLE)
    S.b[:] = 0x5A
    ns = len(seqs)
    opb = 4
    written = np.zeros(TABLE, dtype=np.int32)   # plain interior dword writes per byte
    steps = 0
    for b0 in range(0, ns + 1, WAVE):
        L = []
        for lane in range(WAVE):
            s = b0 + lane
            m, act = s < ns, s <= ns
            ip, off, lit, mc = n, 0, (n - la if act else 0), 0
            if m:
                ip, off, lit, ml = seqs[s]
                mc = ml - MIN_MATCH
            le = ext_bytes(lit)
            me = ext_bytes(mc) if m else 0
            ln = 1 + le + lit + (2 + me if m else 0) if act else 0
            L.append(dict(m=m, act=act, ip=ip, off=off, lit=lit, mc=mc, le=le, me=me, len=ln))
        op = opb
        for r in L:
            r["op"] = op
            op += r["len"]
            r["lp"] = r["op"] + 1 + r["le"]
            r["lsrc"] = r["ip"] - r["lit"]
        opb = op
        lane_max = LANE_RUN if sum(r["lit"] > 16 for r in L) >= LANE_RUN_MIN else 16
        for r in L:
            ll, ml = (r["lit"] - 15) % 255, (r["mc"] - 15) % 255
            tok = min(r["lit"], 15) << 4 | (min(r["mc"], 15) if r["m"] else 0)
            put5(S, r["op"], tok | len_run_head(4, r["le"], ll) << 8, 1 + min(r["le"], 4) if r["act"] else 0)
            put5(S, r["lp"] + r["lit"], r["off"] | len_run_head(3, r["me"], ml) << 16,
                 2 + min(r["me"], 3) if r["m"] else 0)
        len_rest(S, 4, [(r["op"] + 1, r["le"], (r["lit"] - 15) % 255) for r in L])
        len_rest(S, 3, [(r["lp"] + r["lit"] + 2, r["me"], (r["mc"] - 15) % 255) for r in L])
        # the destination-dword frame of every literal run
        for r in L:
            k = r["lp"] & 3
            b = r["lsrc"] - k
            r["sh"], r["W"], r["O"] = b & 3, b & ~3, r["lp"] & ~3
            r["nd"] = ((r["lp"] + r["lit"] + 3) >> 2) - (r["lp"] >> 2)
            if r["lit"] <= 0:
                continue
            nd, W, O, sh = r["nd"], r["W"], r["O"], r["sh"]
            e = r["lp"] + r["lit"] - 4 * ((r["lp"] + r["lit"] - 1) >> 2)
            mt = 0xFFFFFFFF if e >= 4 else (1 << 8 * e) - 1
            mh = (0xFFFFFFFF << 8 * k) & 0xFFFFFFFF
            if nd == 1:
                mh &= mt
            S.wr32(O, alignbyte(D.rd32(W + 4), D.rd32(W), sh) & mh, mh)
            if nd > 1:
                S.wr32(O + 4 * (nd - 1), alignbyte(D.rd32(W + 4 * nd), D.rd32(W + 4 * (nd - 1)), sh) & mt, mt)

        def put(r, t):
            a = r["O"] + 4 * t
            S.wr32(a, alignbyte(D.rd32(r["W"] + 4 * t + 4), D.rd32(r["W"] + 4 * t), r["sh"]))
            written[a:a + 4] += 1

        # interior dwords 1 .. nd - 2: short runs by their own lanes ...
        for r in L:
            if 0 < r["lit"] <= lane_max:
                for t in range(1, r["nd"] - 1):
                    put(r, t)
        # ... long runs by the wave, run after run
        for r in L:
            if r["lit"] <= lane_max:
                continue
            last, W, O, sh = r["nd"] - 2, r["W"], r["O"], r["sh"]
            assert last >= 1
            steps += 1
            if last <= WAVE:            # one dword per lane
                for lane in range(WAVE):
                    t = 1 + lane
                    D.rd32(W + 4 * t), D.rd32(W + 4 * t + 4)   # unmasked
                    if t <= last:
                        put(r, t)
                continue
            # 16-byte chunks of the destination; the dwords around them by lanes 0-3 / 4-7
            a = 1 + (((0 - (O + 4)) & 15) >> 2)
            nc = (last - a + 1) >> 2
            assert 1 <= a <= 4 and nc >= 1 and (O + 4 * a) % 16 == 0
            for lane in range(8):
                te = 1 + lane if lane < 4 else a + 4 * nc + (lane - 4)
                if (te < a) if lane < 4 else (te <= last):
                    put(r, te)
            sa = W + 4 * a
            q = (sa >> 2) & 3
            X = sa & ~15
            assert X >= 0
            for c0 in range(0, nc, WAVE):
                steps += 1
                for lane in range(WAVE):
                    c = c0 + lane
                    z = [D.rd32(X + 16 * c + 4 * i) for i in range(8)]   # two aligned 16-byte reads, unmasked
                    if c < nc:
                        for i in range(4):
                            aadr = O + 4 * (a + 4 * c + i)
                            assert (O + 4 * (a + 4 * c)) % 16 == 0
                            S.wr32(aadr, alignbyte(z[q + i + 1], z[q + i], sh))
                            written[aadr:aadr + 4] += 1
    assert written.max() <= 1, "an interior dword was written twice"
    assert D.hi < n + PAD
    if stats is not None:
        stats["steps"] = stats.get("steps", 0) + steps
        stats["read_hi"] = max(stats.get("read_hi", 0), D.hi - n)
    return S.b[4:opb].copy()
