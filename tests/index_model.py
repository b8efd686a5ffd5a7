"""The block-index rebuild of csrc/lz4_decode.hip restated in plain Python, and
builders of framed streams whose literals carry decoy header chains
(tests/test_index_model.py on the CPU, tests/test_gpu_index_rebuild.py on the
device).

The rebuild (k_idx_exits, k_idx_exits_join, chunk_entry, k_idx_walk,
k_idx_check) cuts the framed region [0, Cb) into chunks of CH bytes.  Phase 1
tries every position of a chunk's window [s CH, s CH + W) whose big-endian
32-bit word is a plausible record length, follows each such chain to the first
position >= the chunk end, and keeps the exit only if every surviving chain
agrees; otherwise the chunk is ambiguous and its successor's entry is chased
from the nearest agreed exit.  An encoder-made payload practically never holds
a second chain that survives a whole chunk, so the streams here plant one: a
literal-only block (lz4_craft.payload([], literals)) carries its literals
verbatim, and with them any 4-byte word at any position.

serial_index() is the reference's serial walk and the expected value of
everything; exits() restates phase 1 and reports what a stream visits: per
chunk the exit, the plausible candidates per 256-candidate screening step (the
candidate list holds 512: more makes the kernel chase the list mid-window) and
per slice of `wsub` candidates (windows above the LDS budget are split over
workgroups and joined by k_idx_exits_join) the extremes of the surviving exits.
"""
import bisect

import numpy as np

from tests import lz4_craft as C

AMBIGUOUS = -2          # kAmbiguous
DEAD = -1               # kDead
WIN_MAX = 32768         # kIdxWinMax
CAND_CAP = 512          # kIdxCandCap
STEP = 4 * C.WAVE       # candidates per screening step (4 per lane)


# ---------------------------------------------------------------- geometry
class Geometry:
    """Of streams with blocks of n = block_size * elem_size bytes: launch_index,
    index_chunk_bytes, idx_win_lds and idx_wsub."""

    def __init__(self, n):
        self.n = n
        self.maxlen = C.lz4_bound(n)
        self.W = 4 + self.maxlen
        ch = 128 * 1024
        while ch < 2 * self.W:
            ch *= 2
        self.CH = ch
        w = (self.W + 3 + 16 + 64 + 15) & ~15
        self.win_lds = w if w < WIN_MAX else WIN_MAX
        self.wsub = self.W if self.win_lds < WIN_MAX else WIN_MAX - 128
        self.ny = -(-self.W // self.wsub)

    def nchunks(self, Cb):
        return -(-Cb // self.CH) if Cb > 0 else 0


def slice_lds_bytes(wsub):
    """The most bytes k_idx_exits stages for one slice: a start up to 15 bytes
    past a 16-byte boundary, wsub candidates, 3 more bytes of the last one's
    word, in whole 16-byte granules (`nch * 16`)."""
    return (15 + wsub + 3 + 15) & ~15


def layout(size, block):
    """(blocks, tail elements) of `size` elements in blocks of `block`."""
    nfull, rest = divmod(size, block)
    return nfull + (1 if rest // 8 else 0), rest % 8


# ------------------------------------------------------------- the two walks
def serial_index(buf, Cb, nb):
    """The reference's serial walk: nb header offsets tiling [0, Cb).  Raises
    ValueError(offset) at a header it cannot follow."""
    offs, p = [], 0
    for _ in range(nb):
        if p + 4 > Cb:
            raise ValueError(p)
        ln = int.from_bytes(bytes(buf[p:p + 4]), "big")
        if ln == 0 or p + 4 + ln > Cb:
            raise ValueError(p)
        offs.append(p)
        p += 4 + ln
    if p != Cb:
        raise ValueError(p)
    return np.array(offs, dtype=np.int64)


def _links(buf, Cb, maxlen):
    """nxt[p]: where the word at p points if it is a plausible header, else -1
    (p + 4 <= Cb for every p < len(nxt))."""
    if Cb < 4:
        return []
    b = np.asarray(buf[:Cb], dtype=np.int64)
    v = (b[:-3] << 24) | (b[1:-2] << 16) | (b[2:-1] << 8) | b[3:]
    q = np.arange(Cb - 3, dtype=np.int64) + 4 + v
    return np.where((v != 0) & (v <= maxlen) & (q <= Cb), q, -1).tolist()


def plausible_positions(buf, Cb, n):
    """Every position of [0, Cb) that phase 1 would take for a header."""
    nxt = np.array(_links(buf, Cb, C.lz4_bound(n)), dtype=np.int64)
    return np.nonzero(nxt >= 0)[0]


def _chaser(nxt, Cb, stop):
    """chase() of the kernels towards one `stop`, with a memo per position."""
    memo = {}

    def chase(p):
        path = []
        while p < stop and p != Cb:
            if p in memo:
                p = memo[p]
                break
            path.append(p)
            q = nxt[p] if p < len(nxt) else -1
            if q < 0:
                p = DEAD
                break
            p = q
        for x in path:
            memo[x] = p
        return p
    return chase


class ChunkExits:
    """What phase 1 computes for one chunk.  exit: agreed offset, DEAD or
    AMBIGUOUS; survivors: the distinct exits, sorted; ncand: plausible
    candidates in the window; steps[y]: their number per screening step of
    slice y; flushes[y]: how often the list is chased before the slice's last
    step (`nl + total > kIdxCandCap`); flushed_at[y]: the candidates of slice y
    chased in each flush, the closing one included; slices[y]: (min, max) of
    the slice's surviving exits or None."""

    def __init__(self):
        self.exit, self.survivors, self.ncand = DEAD, [], 0
        self.steps, self.flushes, self.flushed_at, self.slices = [], [], [], []


def exits(buf, Cb, n, nch=None):
    """Phase 1 (k_idx_exits and k_idx_exits_join) per chunk; nch: chunks
    launched (more than the stream has when a capacity sizes them)."""
    g = Geometry(n)
    nxt = _links(buf, Cb, g.maxlen)
    out = []
    for s in range(g.nchunks(Cb) if nch is None else nch):
        ce_ = ChunkExits()
        out.append(ce_)
        cs = s * g.CH
        if s > 0 and cs >= Cb:
            continue
        ce = min(cs + g.CH, Cb)
        chase = _chaser(nxt, Cb, ce)
        cwin = cs + 1 if s == 0 else min(cs + g.W, Cb)
        found = set()
        for y in range(g.ny):
            cb0 = min(cs + y * g.wsub, cwin)
            cend = min(cb0 + g.wsub, cwin)
            steps, groups, nl, cur, mine = [], [], 0, [], set()
            for c0 in range(cb0, cend, STEP):
                cand = [c for c in range(c0, min(c0 + STEP, cend)) if c < len(nxt) and nxt[c] >= 0]
                steps.append(len(cand))
                if not cand:
                    continue
                if nl + len(cand) > CAND_CAP:
                    groups.append(cur)
                    cur, nl = [], 0
                cur += cand
                nl += len(cand)
            groups.append(cur)
            for grp in groups:
                for c in grp:
                    x = chase(nxt[c])
                    if x != DEAD:
                        mine.add(x)
            ce_.steps.append(steps)
            ce_.flushes.append(len(groups) - 1)
            ce_.flushed_at.append(groups)
            ce_.slices.append((min(mine), max(mine)) if mine else None)
            ce_.ncand += sum(steps)
            found |= mine
        ce_.survivors = sorted(found)
        if found:
            ce_.exit = ce_.survivors[0] if len(found) == 1 else AMBIGUOUS
    return out


def rebuild(buf, Cb, n, nb):
    """Phases 1 to 4 and the check: the offsets the device writes, or None
    where it reports an error (a broken link in a chunk's walk, or a header
    count other than nb)."""
    g = Geometry(n)
    nxt = _links(buf, Cb, g.maxlen)
    ex = [c.exit for c in exits(buf, Cb, n)]
    offs = []
    for s in range(len(ex)):
        ce = min((s + 1) * g.CH, Cb)
        if s == 0:
            p = 0
        else:                       # chunk_entry
            t = s - 1
            while t >= 0 and ex[t] < 0:
                t -= 1
            p = 0 if t < 0 else ex[t]
            for u in range(t + 1, s):
                if p != DEAD:
                    p = _chaser(nxt, Cb, min((u + 1) * g.CH, Cb))(p)
        if p == DEAD:
            return None
        while p < ce:               # k_idx_walk
            if p >= len(nxt) or nxt[p] < 0:
                return None
            offs.append(p)
            p = nxt[p]
    return np.array(offs, dtype=np.int64) if len(offs) == nb else None


# ------------------------------------------------------------ stream builder
def base_literals(n, k):
    """Block k's literals before anything is planted: every byte >= 0x80, so no
    word of them is a plausible length, and none next to a planted word of 256
    and more (00 00 hi lo) either."""
    i = np.arange(n, dtype=np.int64) + k * n
    return (0x80 | ((i * 37 + (i >> 7) * 11 + k) & 0x7F)).astype(np.uint8)


def _extb(v):
    return 0 if v < 15 else (v - 15) // 255 + 1


def lead_payload(n, paylen):
    """A compressed block of n bytes whose payload is exactly `paylen` bytes:
    literals, one long match of offset 1, the last literals.  In front of a
    stream of literal-only blocks it moves every later header, and with them
    where a chunk's true header lies in its window."""
    for last in range(5, 40):
        for lit in range(max(paylen - 96, 1), paylen):
            ml = n - lit - last
            if lit < 1 or ml < 12:
                continue
            if 1 + _extb(lit) + lit + 2 + _extb(ml - 4) + 1 + _extb(last) + last == paylen:
                src = base_literals(lit + last, 7).tobytes()
                pay = C.payload([(src[:lit], 1, ml)], src[lit:])
                assert len(pay) == paylen and len(C.decode(pay, n)) == n
                return pay
    raise ValueError("no lead block of %d payload bytes" % paylen)


class Crafted:
    """A built stream: buf (uint8), E, block (elements), size (elements), nb,
    Cb, tail (bytes), g (Geometry), starts (the true headers), planted (every
    planted word's offset), fills ((a, b) spans filled with words), note."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    @property
    def n(self):
        return self.E * self.block

    def chunk_of(self, p):
        return p // self.g.CH


class Planter:
    """nblocks literal-only blocks (behind an optional compressed lead block)
    whose literals take planted words at STREAM offsets."""

    def __init__(self, E, block, nblocks, tail=b"", lead=None, lits=None):
        assert block % 8 == 0 and len(tail) % E == 0 and len(tail) // E < 8
        self.E, self.block, self.nblocks = E, block, nblocks
        n = self.n = E * block
        self.g = Geometry(n)
        self.hdr = len(C.payload([], bytes(n))) - n     # token + length bytes
        self.rec = 4 + self.hdr + n
        self.lead, self.tail = lead, bytes(tail)
        self.lits = [bytearray((lits(k) if lits else base_literals(n, k)).tobytes()) for k in range(nblocks)]
        self.starts, o = [], 0
        for k in range(nblocks):
            self.starts.append(o)
            o += 4 + len(lead) if (k == 0 and lead is not None) else self.rec
        self.Cb = o
        self.planted, self.fills, self.used = [], [], set()

    def span(self, k):
        """Stream offsets [a, b) of block k's literals."""
        if k == 0 and self.lead is not None:
            return 0, 0
        return self.starts[k] + 4 + self.hdr, self.starts[k] + self.rec

    def fits(self, p):
        if p < 0 or p + 4 > self.Cb:
            return False
        a, b = self.span(bisect.bisect_right(self.starts, p) - 1)
        return a <= p and p + 4 <= b and not (self.used & set(range(p, p + 4)))

    def first_fit(self, p):
        while not self.fits(p):
            p += 1
        return p

    def plant(self, p, length, note=True):
        assert self.fits(p), p
        assert 0 < length <= self.g.maxlen, length
        k = bisect.bisect_right(self.starts, p) - 1
        i = p - self.span(k)[0]
        self.lits[k][i:i + 4] = int(length).to_bytes(4, "big")
        self.used |= set(range(p, p + 4))
        if note:
            self.planted.append(p)
        return p + 4 + length

    def chain(self, p, step, until, land=None, hops=None, nudge=64):
        """A decoy chain from p: records of `step` bytes (longer by multiples of
        `nudge` where the next header would not lie in literals), until the
        next position is >= until; `land`: where the hop that crosses `until`
        goes; hops: stop after that many (the next position then holds literals
        and the chain dies there).  Returns (positions, where the last points)."""
        out = []
        while p < until and (hops is None or len(out) < hops):
            L = step
            if land is not None and p + 4 + L >= until:
                L = land - p - 4
            else:
                while not self.fits(p + 4 + L):
                    L += nudge
            out.append(p)
            p = self.plant(p, L)
        return out, p

    def fill(self, a, b, length):
        """Words of `length` back to back over the literals of [a, b)."""
        a = self.first_fit(a)
        p = a
        while p + 4 <= b and self.fits(p):
            self.plant(p, length, note=False)
            p += 4
        self.fills.append((a, p))
        return (p - a) // 4

    def build(self, **note):
        pays = [C.payload([], bytes(l)) for l in self.lits]
        if self.lead is not None:
            pays[0] = self.lead
        buf = C.stream(pays, self.tail)
        assert len(buf) == self.Cb + len(self.tail)
        starts = np.array(self.starts, dtype=np.int64)
        assert serial_index(buf, self.Cb, self.nblocks).tolist() == self.starts
        return Crafted(buf=buf, E=self.E, block=self.block, nb=self.nblocks, Cb=self.Cb,
                       size=self.nblocks * self.block + len(self.tail) // self.E, tail=len(self.tail),
                       g=self.g, starts=starts, planted=sorted(self.planted), fills=list(self.fills),
                       note=note)


# --------------------------------------------------------------- the families
WORD16 = bytes([0, 0, 0, 0x10])


def words16(nbytes):
    """`nbytes` of 00 00 00 10 words (the last one cut)."""
    return (WORD16 * (nbytes // 4 + 1))[:nbytes]


D1_VARIANTS = ("dies", "exact", "tail")


def d1(variant, block=64, nblocks=5800, at=20):
    """D1, a parallel decoy: every block's literals hold, at index `at`, a
    header as long as a whole record less 4, so a second complete chain runs
    beside the true one and every interior chunk is ambiguous.  The last decoy
    "dies" (points past Cb), is cut to end "exact"ly at Cb, or points into a
    raw "tail" of 7 elements that holds 00 00 00 10 words."""
    p = Planter(1, block, nblocks, tail=words16(7) if variant == "tail" else b"")
    for k in range(nblocks):
        q = p.span(k)[0] + at
        L = p.rec - 4
        if k == nblocks - 1 and variant == "exact":
            L = p.Cb - q - 4
        if k == nblocks - 1 and variant == "tail":
            L = p.Cb + 3 - q - 4
        p.plant(q, L)
    return p.build(family="d1", variant=variant)


D2_SHAPES = {"e1": (1, 8192, 0), "e4": (4, 2048, 0), "e12": (12, 680, 7)}
D2_KINDS = ("a", "b", "c", "d")
D2_BLOCKS = 50


def _shape(shape):
    E, block, tail_elems = D2_SHAPES[shape]
    return E, block, base_literals(tail_elems * E, 99).tobytes()


def d2(kind, shape="e1"):
    """D2, blocks of 8 KiB, decoys that start 100 bytes into chunk 1:
    a -- a chain that leaves the chunk 16 bytes behind its end, in front of the
         true exit: one ambiguous chunk between agreed ones;
    b -- three decoys, the last landing on a true header: agreed despite them;
    c -- three decoys, then literals: the chain dies inside its chunk;
    d -- a's chain and a second one that leaves the chunk behind the true exit:
         three distinct exits."""
    E, block, tail = _shape(shape)
    p = Planter(E, block, D2_BLOCKS, tail=tail)
    cs, ce = p.g.CH, 2 * p.g.CH
    at = p.first_fit(cs + 100)
    assert at < cs + p.g.W
    if kind in ("a", "d"):
        p.chain(at, 5000, ce, land=ce + 16)
    if kind == "d":
        true_exit = p.starts[bisect.bisect_left(p.starts, ce)]
        p.chain(p.first_fit(at + 40), 4100, ce, land=p.first_fit(true_exit + 1000))
    if kind == "b":
        pos, q = p.chain(at, 5000, ce, hops=2)
        p.plant(q, p.starts[bisect.bisect_left(p.starts, q + 5)] - q - 4)
    if kind == "c":
        p.chain(at, 5000, ce, hops=3)
    return p.build(family="d2", kind=kind, shape=shape, chunk=1)


def d1_8k():
    """D1's pattern at 8 KiB blocks (the batch's neighbour of D2a)."""
    return d1("dies", block=8192, nblocks=D2_BLOCKS, at=100)


D3_KINDS = ("below", "at", "above", "behind", "thousands", "first")
WORD48 = 0x30       # 00 00 00 30 back to back: one candidate per 4 bytes


def _d3_planter(target):
    """50 blocks of 8 KiB behind a lead block that puts chunk 2's true header
    `target` bytes into its window."""
    probe = Planter(1, 8192, D2_BLOCKS)
    cs = 2 * probe.g.CH
    d0 = probe.starts[bisect.bisect_left(probe.starts, cs)] - cs
    delta = (d0 - target) % probe.rec
    p = Planter(1, 8192, D2_BLOCKS, lead=lead_payload(8192, probe.rec - delta - 4))
    assert p.starts[bisect.bisect_left(p.starts, cs)] - cs == target
    return p, cs


def d3(kind):
    """D3, the candidate list's cap, in chunk 2's window.  A live decoy (a
    chain that leaves the chunk in front of the true exit) makes the chunk
    ambiguous; words of length 48, which die, fill the list.
    below / at / above -- 511, 512, 513 plausible candidates in the window;
    behind -- the live decoy first, 600 words, then the true header, which is
        chased in a later flush than the decoy;
    thousands -- as behind, with 00 00 00 10 words over all the literals in
        front of the true header;
    first -- the true header first, 600 words, the live decoy last."""
    if kind == "first":
        p, cs = _d3_planter(300)
        p.fill(cs + 400, cs + 400 + 4 * 600, WORD48)
        p.chain(p.first_fit(cs + 7000), 5000, cs + p.g.CH, land=cs + p.g.CH + 16)
        return p.build(family="d3", kind=kind, chunk=2)
    p, cs = _d3_planter(4100)
    p.chain(cs, 5000, cs + p.g.CH, land=cs + p.g.CH + 16)
    if kind == "thousands":
        p.fill(cs + 8, cs + 4100 - 8, 0x10)
    elif kind == "behind":
        p.fill(cs + 8, cs + 8 + 4 * 600, WORD48)
    else:
        want = {"below": 511, "at": 512, "above": 513}[kind]
        have = exits(p.build().buf, p.Cb, p.n)[2].ncand
        p.fill(cs + 8, cs + 8 + 4 * (want - have), WORD48)
    return p.build(family="d3", kind=kind, chunk=2)


D4_KINDS = ("s0", "s1", "straddle", "join_s1", "join_s0")
D4_BLOCK = 49152


def d4(kind):
    """D4, windows split over two workgroups (blocks of 48 KiB: W = 49,364,
    slices of 32,640 candidates).  Chunk 1's true header lies in slice 0 of its
    window, chunk 2's in slice 1.  Every decoy leaves its chunk 16 bytes behind
    the end, in front of the true exit.
    s0 -- chunk 1, a decoy in slice 0 beside the true header;
    s1 -- chunk 2, a decoy in slice 1 beside the true header;
    straddle -- chunk 1, a decoy at candidate 32,638: the last two bytes of its
        word are the first two of slice 1;
    join_s1 -- chunk 1, the decoy in slice 1: each slice agrees with itself;
    join_s0 -- chunk 2, the decoy in slice 0: the same, mirrored."""
    p = Planter(1, D4_BLOCK, 9)
    s, off = {"s0": (1, 1000), "s1": (2, 40000), "straddle": (1, p.g.wsub - 2), "join_s1": (1, 40000),
              "join_s0": (2, 1000)}[kind]
    cs = s * p.g.CH
    p.chain(cs + off, 0xBEC8, cs + p.g.CH, land=cs + p.g.CH + 16)
    return p.build(family="d4", kind=kind, chunk=s)


def clean(E=1, block=8192, nblocks=D2_BLOCKS):
    """Literal-only blocks with nothing planted."""
    return Planter(E, block, nblocks).build(family="clean")


# ------------------------------------------------------- the seeded generator
def random_stream(seed, density, E=1, block=8192, nblocks=D2_BLOCKS):
    """Random literals with decoy words sprinkled in: `density` chain heads per
    interior chunk, each somewhere in its chunk's window; a chain hops by random
    plausible lengths for a random number of hops or until it has left its
    chunk, and ends in literals, on a true header or on another chain."""
    rng = np.random.default_rng(seed)
    n = E * block
    p = Planter(E, block, nblocks, lits=lambda k: rng.integers(0, 256, n, dtype=np.uint8))
    g = p.g
    nch = g.nchunks(p.Cb)
    for s in range(1, nch - 1):
        for _ in range(density):
            q = p.first_fit(s * g.CH + int(rng.integers(0, g.W - 8)))
            stop = (s + 1 + int(rng.integers(0, 2))) * g.CH
            hops = int(rng.integers(8, 200))
            while hops and q < min(stop, p.Cb - 2 * g.W):
                hops -= 1
                nxt = None
                if rng.integers(0, 16) == 0:       # onto the next true header
                    t = p.starts[bisect.bisect_left(p.starts, q + 5)]
                    if t - q - 4 <= g.maxlen:
                        nxt = t
                for _try in range(8):
                    if nxt is not None:
                        break
                    c = q + 4 + int(rng.integers(256, g.maxlen + 1))
                    if c in p.planted or p.fits(c):
                        nxt = c
                if nxt is None or not p.fits(q):
                    break
                p.plant(q, nxt - q - 4)
                if not p.fits(nxt):                # a true header or another chain
                    break
                q = nxt
    return p.build(family="random", seed=seed, density=density)
