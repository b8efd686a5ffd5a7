"""Hand-built LZ4 block streams for the decoder tests (tests/test_lz4_craft.py
on the CPU, tests/test_gpu_decode_paths.py on the device).

Nothing here is an encoder: payload() writes the LZ4 block format field by
field from a list of sequences, decode() is a byte-at-a-time decoder of that
format (the tests' high-precision reference next to the oracle), classify()
restates the dispatch of the device executor (lz4_exec_block / wave_match in
bitshuffle_amd/csrc/lz4_decode.hip) so that the tests can assert which of its
paths a stream visits, and batches() restates its batching rules.

The families f1..f7 are deterministic generators of payloads that decode to
exactly n bytes each.  Block-format end rules (lz4_scan.h, scan_block): a
match starts at or before n - 12 and ends at or before n - 5; the last
sequence is literals only.  Block enforces them.
"""
import numpy as np

WAVE = 64
MINMATCH = 4
DEC_PER = 16            # kDecPer: per-lane periodic fills up to this length
IN_PLACE_MARGIN = 704   # kInPlaceMargin


def lz4_bound(n):
    return n + n // 255 + 16


# ---------------------------------------------------------------- the format
def _ext(v):
    out = bytearray()
    while v >= 255:
        out.append(255)
        v -= 255
    out.append(v)
    return out


def payload(seqs, last_literals):
    """seqs: (literal_bytes, offset, match_len) per sequence; then the last,
    literal-only sequence."""
    out = bytearray()
    for lit, off, ml in seqs:
        lit = bytes(lit)
        assert ml >= MINMATCH and 0 <= off <= 0xFFFF, (off, ml)
        out.append((min(len(lit), 15) << 4) | min(ml - MINMATCH, 15))
        if len(lit) >= 15:
            out += _ext(len(lit) - 15)
        out += lit
        out += bytes([off & 255, off >> 8])
        if ml - MINMATCH >= 15:
            out += _ext(ml - MINMATCH - 15)
    last = bytes(last_literals)
    out.append(min(len(last), 15) << 4)
    if len(last) >= 15:
        out += _ext(len(last) - 15)
    out += last
    return bytes(out)


def frame(payloads):
    """bitshuffle's framing: a big-endian 32-bit length in front of every block."""
    out = bytearray()
    for p in payloads:
        out += len(p).to_bytes(4, "big") + p
    return bytes(out)


def stream(payloads, tail=b""):
    return np.frombuffer(frame(payloads) + bytes(tail), dtype=np.uint8)


def parse(pay):
    """[(tp, lit, lsrc, off, ml)] of a well-formed payload; the last has ml 0."""
    out, p, end = [], 0, len(pay)
    while True:
        tp = p
        tok = pay[p]
        p += 1
        lit = tok >> 4
        if lit == 15:
            while True:
                b = pay[p]
                p += 1
                lit += b
                if b != 255:
                    break
        lsrc = p
        p += lit
        if p > end:
            raise ValueError("literals run past the payload")
        if p == end:
            out.append((tp, lit, lsrc, 0, 0))
            return out
        off = pay[p] | (pay[p + 1] << 8)
        p += 2
        ml = tok & 15
        if ml == 15:
            while True:
                b = pay[p]
                p += 1
                ml += b
                if b != 255:
                    break
        out.append((tp, lit, lsrc, off, ml + MINMATCH))


def decode(pay, n):
    """Byte-at-a-time LZ4 block decoder.  Offset 0 writes zeros, as
    LZ4_decompress_safe does (see the comment on wave_match)."""
    out = bytearray()
    for _, lit, lsrc, off, ml in parse(pay):
        out += pay[lsrc:lsrc + lit]
        if ml == 0:
            break
        if off > len(out):
            raise ValueError("offset %d before the block start at %d" % (off, len(out)))
        if off == 0:
            out += bytes(ml)
        else:
            for _ in range(ml):
                out.append(out[-off])
    if len(out) != n:
        raise ValueError("decodes to %d bytes, not %d" % (len(out), n))
    return bytes(out)


def walk(pay):
    """Per sequence: dict(j, tp, lit, lsrc, off, ml, op, mop)."""
    out, op = [], 0
    for j, (tp, lit, lsrc, off, ml) in enumerate(parse(pay)):
        out.append(dict(j=j, tp=tp, lit=lit, lsrc=lsrc, off=off, ml=ml, op=op, mop=op + lit))
        op += lit + ml
    return out


# ------------------------------------------------- the executor's dispatch
MATCH_LABELS = ("lane_copy", "lane_fill124", "wave_copy_le64", "wave_copy_gt64", "wave_zero",
                "wave_overlap_le64", "wave_fill124", "wave_mod")
LIT_LABELS = ("lit_lane", "lit_wave_le64", "lit_wave_gt64")


def classify(lit, off, ml, mop):
    """(literal label or None, match label or None) of one sequence, as
    lz4_exec_block dispatches it:

    literals -- 1..16 bytes by the sequence's own lane (copy16), longer runs by
    the wave (copyw / wave_copy: n <= 64 one byte per lane, else dwords);
    match -- `per` (off < ml <= kDecPer, off in {1, 2, 4}): the lane's periodic
    fill; not coop (ml <= 16 and off >= ml): the lane's 16-byte copy; else
    wave_match: off >= ml -> wave_copy (n <= 64 / > 64), off == 0 -> zeros,
    ml <= 64 -> one byte per lane, q1 <= q0 (cannot happen above 64 bytes),
    off in {1, 2, 4} -> rotated pattern dword, else small_mod."""
    ll = None
    if lit > 0:
        ll = "lit_lane" if lit <= 16 else ("lit_wave_le64" if lit <= WAVE else "lit_wave_gt64")
    if ml == 0:
        return ll, None
    if off < ml and ml <= DEC_PER and off in (1, 2, 4):
        return ll, "lane_fill124"
    if not (ml > 16 or off < ml):
        return ll, "lane_copy"
    if off >= ml:
        return ll, "wave_copy_le64" if ml <= WAVE else "wave_copy_gt64"
    if off == 0:
        return ll, "wave_zero"
    if ml <= WAVE:
        return ll, "wave_overlap_le64"
    q0, q1 = (mop + 3) & ~3, (mop + ml) & ~3
    assert q1 > q0, "ml > 64 always holds an aligned dword"
    return ll, "wave_fill124" if off in (1, 2, 4) else "wave_mod"


def is_coop(off, ml):
    return classify(0, off, ml, 0)[1].startswith("wave_")


def batches(seqs, rule="lds"):
    """Match batches per 64-sequence chunk: [[[j, ...] per batch] per chunk].
    rule "lds": lz4_exec_block (a later match breaks the batch when
    rend = mop - off + min(ml, off) > opf); rule "big": k_lz4_exec_big and
    tests/exec_model.py (off < ml or mop - off + ml > opf)."""
    out = []
    for c0 in range(0, len(seqs), WAVE):
        lanes = seqs[c0:c0 + WAVE]
        todo = [s for s in lanes if s["ml"] > 0]
        chunk = []
        while todo:
            opf = todo[0]["mop"]
            g = None
            for s in todo[1:]:
                if rule == "lds":
                    brk = s["mop"] - s["off"] + min(s["ml"], s["off"]) > opf
                else:
                    brk = s["off"] < s["ml"] or s["mop"] - s["off"] + s["ml"] > opf
                if brk:
                    g = s["j"]
                    break
            batch = [s["j"] for s in todo if g is None or s["j"] < g]
            chunk.append(batch)
            todo = [s for s in todo if s["j"] not in batch]
        out.append(chunk)
    return out


def survey(payloads, base=0):
    """Walks framed payloads (first header at stream byte `base`).  Returns
    (match cells, literal cells, record starts): cells are (label, destination
    & 3, source & 3); a literal run's source is its position in the stream,
    which is what its address in LDS or in global memory is congruent to."""
    mc, lc, starts = set(), set(), []
    o0 = base
    for pay in payloads:
        starts.append(o0)
        for s in walk(pay):
            ll, ml_ = classify(s["lit"], s["off"], s["ml"], s["mop"])
            if ll:
                lc.add((ll, s["op"] & 3, (o0 + 4 + s["lsrc"]) & 3))
            if ml_:
                mc.add((ml_, s["mop"] & 3, (s["mop"] - s["off"]) & 3))
        o0 += 4 + len(pay)
    return mc, lc, starts


# ------------------------------------------------------------ block builder
class Lits:
    """Literal bytes: any 256 consecutive ones are distinct (167 is odd), and
    the pattern drifts from one group of 256 to the next."""

    def __init__(self, start=0):
        self.c = start

    def take(self, k):
        i = np.arange(self.c, self.c + k, dtype=np.int64)
        self.c += k
        return ((i * 167 + (i >> 8) * 91 + 13) & 255).astype(np.uint8).tobytes()


class Block:
    def __init__(self, n, src, reserve=0):
        self.n, self.src, self.reserve = n, src, reserve
        self.seqs, self.op = [], 0

    def fits(self, lit, ml, reserve=None):
        r = self.reserve if reserve is None else reserve
        mop = self.op + lit
        return mop <= self.n - 12 - r and mop + ml <= self.n - 5 - r

    def add(self, lit, off, ml):
        assert self.fits(lit, ml, 0), (self.n, self.op, lit, ml)
        assert off <= self.op + lit, (self.op, lit, off)
        self.seqs.append((self.src.take(lit), off, ml))
        self.op += lit + ml

    def length(self):
        return len(payload(self.seqs, bytes(self.n - self.op)))

    def close(self, residue=None):
        """The payload; with `residue`, 4-byte matches in place of last
        literals (3 record bytes instead of 4) bring its length to residue
        mod 16."""
        if residue is not None:
            while self.length() % 16 != residue:
                self.add(0, 8, 4)
        pay = payload(self.seqs, self.src.take(self.n - self.op))
        assert len(pay) <= lz4_bound(self.n)
        return pay


def _up4(v):
    return (v + 3) & ~3


# ------------------------------------------------------------------ families
F1_OFFS = (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 12, 15, 16, 17, 31, 32, 33, 63, 64, 65, 66, 100, 255, 256, 257)
F1_FAR = (8193, 32768, 65535)
F1_MLS = tuple(range(4, 22)) + (31, 32, 33) + tuple(range(63, 70)) + tuple(range(127, 134)) + \
    (255, 270, 274, 1000)


def f1(n, offs=F1_OFFS, thin=False):
    """Match grid: one sequence per (off, ml, mop & 3).  Every block opens with
    a prologue of literals longer than its largest offset; every new offset
    opens with fresh literals covering one period, so the pattern a fill
    repeats has distinct bytes and a wrong rotation changes the output.  The
    0..3 literals in front of a match force its destination alignment.  thin:
    the alignment rotates with the cell instead of being crossed (large
    blocks).  Cells that cannot fit a block of n bytes at all are left out
    (n = 1024: ml = 1000)."""
    out = []
    src = Lits(1)
    groups = [[o for o in offs if o <= 257], [o for o in offs if o > 257]]
    for grp in groups:
        if not grp:
            continue
        pro = _up4(max(grp) + 4)
        blk, pend = Block(n, src), pro
        cell = 0
        for off in grp:
            if off <= 257:   # (a far offset reads the prologue)
                pend = max(pend, _up4(max(off, 8)))
            for ml in F1_MLS:
                for a in ([cell % 4] if thin else range(4)):
                    cell += 1
                    k = (a - blk.op) & 3
                    if not blk.fits(pend + k, ml):
                        if blk.seqs:
                            out.append(blk.close())
                        blk, pend = Block(n, src), pro
                        k = a
                        if not blk.fits(pend + k, ml):
                            continue
                    blk.add(pend + k, off, ml)
                    pend = 0
        if blk.seqs:
            out.append(blk.close())
    return out


F2_LITS = (0, 1, 3, 4, 5, 14, 15, 16, 17, 18, 31, 32, 33) + tuple(range(63, 70)) + \
    (127, 128, 129, 269, 270, 271, 524, 525, 3000)
F2_LONG_AT = (0, 1, 62, 63, 64)


def f2(n):
    """Literal grid.  Part 1: every run length behind a pad sequence whose
    literal count (0..3) moves source and destination together and whose
    match length (4..7) moves the destination alone: all 16 alignment pairs.
    Part 2: blocks of 130 sequences with short (S, <= 16) and long (L) runs in
    the rotations of S L S S L L S, long runs forced at sequence indices 0, 1,
    62, 63, 64.  Block i's payload length is i mod 16, so the records start at
    many stream alignments."""
    out = []
    src = Lits(2)

    def opened():
        b = Block(n, src, reserve=80)
        b.add(12, 8, 4)
        return b

    blk = opened()
    for L in F2_LITS:
        if not opened().fits(3 + 7 + L, 4):
            continue
        for mlpad in range(4, 8):
            for padlit in range(4):
                if not blk.fits(padlit + mlpad + L, 4):
                    out.append(blk.close(len(out) % 16))
                    blk = opened()
                blk.add(padlit, 8, mlpad)
                blk.add(L, 8, 4)
    out.append(blk.close(len(out) % 16))
    out += f2_arrangements(n, src, len(out))
    while len(out) < 17:   # every payload-length residue at least once
        blk = opened()
        blk.add(20, 8, 40)
        out.append(blk.close(len(out) % 16))
    return out


def f2_arrangements(n, src=None, first=0):
    """Part 2 of f2: one block per rotation of S L S S L L S."""
    src = src or Lits(2)
    out = []
    for r in range(7):
        pat = ("SLSSLLS" * 2)[r:r + 7]
        blk = Block(n, src, reserve=80)
        for i in range(130):
            long_ = i in F2_LONG_AT or pat[i % 7] == "L"
            lit = 17 + (i * 7) % 60 if long_ else (0 if i % 11 == 5 else 1 + (i * 5) % 16)
            if not blk.fits(lit, 4 + i % 4):
                break
            blk.add(lit, 8, 4 + i % 4)
        out.append(blk.close((first + len(out)) % 16))
    return out


def f3(n, thin=False):
    """Length fields: literal and match lengths of 15 + 255 k (last extension
    byte 0) and 15 + 255 k + 254 (last byte 254), k = 0..9, and up to k = 14
    so that the terminating byte falls on every position of read_ext's 7- and
    8-byte windows; match lengths behind 0..7 literals, which puts the offset
    inside (token + literals <= 6 bytes) and outside the token's 8-byte read."""
    out = []
    src = Lits(3)
    cells = []
    for k in range(15):
        for last in (0, 254):
            cells.append((15 + 255 * k + last, 8, 4))
    idx = 0
    for k in range(15):
        for last in (0, 254):
            for lit in (range(8) if (k < 10 and not thin) else [k % 8 if thin else 0]):
                cells.append((lit, (1, 3, 7, 16)[idx % 4], MINMATCH + 15 + 255 * k + last))
                idx += 1
    blk = None
    for lit, off, ml in cells:
        if blk is None or not blk.fits(lit, ml):
            if blk is not None:
                out.append(blk.close())
            blk = Block(n, src)
            blk.add(20, 8, 4)
            if not blk.fits(lit, ml):
                continue
        blk.add(lit, off, ml)
    out.append(blk.close())
    return out


def f4_named(n):
    """Dependency grid: [(pattern name, payload)].  All patterns sit in the
    first 64-sequence chunk unless they are about the chunk boundary."""
    out = []
    src = Lits(4)
    PRO = 300   # prologue literals: independent matches read from here

    def new():
        return Block(n, src)

    # a later match's source ends at opf - 1, opf, opf + 1 (rend > opf breaks
    # the batch): per-lane (ml 6) and wave (ml 20) followers
    for d in (-1, 0, 1):
        for ml in (6, 20):
            b = new()
            b.add(40, 30, 8)                  # head: opf = 40
            mop = 48 + 2
            b.add(2, mop + ml - (40 + d), ml)  # source [.., 40 + d)
            b.add(0, 24, 4)
            out.append(("rend%+d_ml%d" % (d, ml), b.close()))
    # source inside the previous match's output / the own literals / both /
    # reaching into the own output
    for name, off, ml in (("src_in_prev_match", 16, 8), ("src_in_own_literals", 6, 5),
                          ("src_straddles", 9, 6), ("src_into_own_output", 9, 14)):
        b = new()
        b.add(40, 30, 12)
        b.add(6, off, ml)
        b.add(0, 24, 4)
        out.append((name, b.close()))
    # 64 matches, each reading the last 3 bytes of the one before and its own
    # literal: 64 batches of one
    b = new()
    b.add(40, 4, 4)
    for i in range(63):
        b.add(1, 4, 4 if i % 3 else 5)
    out.append(("chain64", b.close()))
    # 64 independent short matches: one batch
    b = new()
    b.add(PRO, 290, 4)
    for i in range(63):
        b.add(0, 280, 4)
    out.append(("independent64", b.close()))
    # wave and per-lane matches alternating in one batch
    cnt = 63 if n >= 2048 else 30   # (all sources must end before the head's output)
    total = 4 + sum(17 if i % 2 == 0 else 4 for i in range(cnt))
    b = new()
    b.add(total + 12, total + 8, 4)
    for i in range(cnt):
        b.add(0, total, 17 if i % 2 == 0 else 4)
    out.append(("alternating", b.close()))
    # a self-overlapping match at lanes 0, 1, 62, 63 (f = 63: no lanes above)
    for lane in (0, 1, 62, 63):
        b = new()
        for i in range(64):
            lit = PRO if i == 0 else 0
            if i == lane:
                b.add(lit, 3, 20)
            else:
                b.add(lit, 290, 4)
        out.append(("self_overlap_lane%d" % lane, b.close()))
    # sequence 64 reads what sequence 63 wrote
    b = new()
    for i in range(63):
        b.add(PRO if i == 0 else 0, 290, 4)
    b.add(1, 290, 6)    # 63
    b.add(0, 5, 5)      # 64: the 5 bytes before its start end 63's output
    b.add(2, 290, 4)
    out.append(("dep_63_to_64", b.close()))
    # exactly 1, 2, 63, 64, 65, 128, 129 sequences (the last is literal-only)
    for cnt in (1, 2, 63, 64, 65, 128, 129):
        b = new()
        for i in range(cnt - 1):
            b.add(40 if i == 0 else i % 3, 9 + i % 5, 4 + i % 2)
        out.append(("nseq%d" % cnt, b.close()))
    return out


# the patterns kept at the large block size (dependent matches back to back:
# what k_lz4_exec_big's fences order)
F4_BIG = ("rend+1_ml6", "rend+1_ml20", "src_into_own_output", "chain64", "alternating",
          "self_overlap_lane63", "dep_63_to_64", "nseq129")


def f4(n, names=None):
    return [p for name, p in f4_named(n) if names is None or name in names]


F5_OFFS = tuple(range(1, 71)) + (127, 128, 129, 255, 256, 257, 1000, 4095, 4096, 4097)
F5_FAR = (8191, 8192, 8193, 32767, 32768, 65534, 65535)


def f5(n, offs=F5_OFFS):
    """Long periodic fills: `off` literals, then one match to n - 5.  Offsets
    that leave no room for the match in n bytes are left out."""
    out = []
    src = Lits(5)
    for off in offs:
        b = Block(n, src)
        ml = n - 5 - off
        if ml < MINMATCH or not b.fits(off, ml):
            continue
        b.add(off, off, ml)
        out.append(b.close())
    return out


F6_SIZES = (16, 24, 40, 64, 72, 128)


def f6(n):
    """Small blocks (scan_block leaves its fast loop below 64 bytes): literal
    only, the longest match a block allows, short periods, offset 0."""
    src = Lits(6)
    out = []
    b = Block(n, src)
    out.append(b.close())
    for lit, off in ((4, 4), (1, 1), (2, 2), (3, 3), (4, 0), (n - 12, n - 12)):
        b = Block(n, src)
        b.add(lit, off, n - 5 - lit)
        out.append(b.close())
    if n >= 24:
        b = Block(n, src)
        b.add(3, 3, 4)
        b.add(1, 2, 4)
        b.add(0, 1, n - 5 - 12)
        out.append(b.close())
    return out


F7_TAIL = 7   # raw tail elements behind the last block (the most a stream has)


def f7(E, bs=80, last_lits=600):
    """In-place margin sweep: two compressible blocks of bs elements of E
    bytes and a raw tail of F7_TAIL elements.  The last block's span runs to
    the end of the stream, so its record lands tail bytes further down its
    LDS buffer than a record that ends its span; from about 700 tail bytes
    (E = 100) it fails the in-place test and is read from global memory.  The
    last literal run is long enough (several 256-byte steps of the wave's
    copy) that decoding it in place where the test fails would overwrite
    record bytes before they are read.  Returns (stream, payloads, n); the
    stream holds 2 * bs + F7_TAIL elements."""
    n = bs * E
    src = Lits(7 + E)
    pays = []
    for i in range(2):
        b = Block(n, src)
        b.add(24 + i, 5, 2000)
        b.add(300, 16, 1000)
        b.add(3, 1, n - b.op - 3 - last_lits)
        pays.append(b.close())
    return stream(pays, src.take(F7_TAIL * E)), pays, n


F7_ES = tuple(range(88, 112))
F7_LARGE = (128, 512)   # (E, bs): 64 KiB blocks, 896 tail bytes


# ------------------------------------------------- the cases the tests share
# block bytes that are a whole number of 8-element groups: E -> n
E_SIZES = {3: 8064, 12: 8160, (3, "16k"): 16320}
# 27,200 3-byte elements: among the largest blocks decoded in LDS (81,720 bytes),
# where block, in-place record and a staging block no longer fit 160 KiB together
LDS_TOP = 81600
BIG = 98304     # above the LDS budget: k_seq_scan_big + k_lz4_exec_big
# (41 and 61: periods at which the f32 quotient of small_mod falls one short
# within 96 KiB, so its downward correction runs in gbl_match too)
F5_BIG_OFFS = (1, 3, 7, 41, 61, 257, 4097, 32767, 65535)
_CASES = {}


def cases():
    """name -> (n, payloads): every family at every block size the device
    tests use (built once per process)."""
    if not _CASES:
        c = _CASES
        for n in (8192, 1024):
            c["f1_%d" % n] = (n, f1(n))
            c["f4_%d" % n] = (n, f4(n))
        c["f2_8192"] = (8192, f2(8192))
        c["f3_8192"] = (8192, f3(8192))
        c["f5_8192"] = (8192, f5(8192))
        c["f5_65536"] = (65536, f5(65536, F5_OFFS + F5_FAR))
        c["f5_%d" % BIG] = (BIG, f5(BIG, F5_BIG_OFFS))
        c["f1_%d" % BIG] = (BIG, f1(BIG, F1_OFFS + F1_FAR, thin=True))
        c["f3_%d" % BIG] = (BIG, f3(BIG, thin=True))
        c["f4_%d" % BIG] = (BIG, f4(BIG, F4_BIG))
        for n in F6_SIZES:
            c["f6_%d" % n] = (n, f6(n))
        c["f5_%d" % LDS_TOP] = (LDS_TOP, f5(LDS_TOP, F5_BIG_OFFS))
        for n in E_SIZES.values():   # element sizes 3 and 12, and 3 with 16 KiB blocks
            c["f1_%d" % n] = (n, f1(n))
            c["f2_%d" % n] = (n, f2(n))
    return _CASES
