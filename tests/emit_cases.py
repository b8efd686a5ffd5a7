"""Shuffled blocks with chosen literal-run and match lengths, for the tests of
the LZ4 encoder's emission (tests/test_emit_model.py, test_gpu_emit_shapes.py).
Test infrastructure only.

A block is built in the SHUFFLED domain -- literal runs are random bytes,
matches are runs of one byte value -- and the codec's input comes from the
oracle's bitunshuffle, so the parse sees exactly these bytes.  LZ4's search
skips ahead after 64 misses, so a literal run of L bytes needs L - s random
bytes, s being the search step when it reaches the run behind them: `tune`
finds that count with the oracle, and every case is checked afterwards by
parsing the oracle's record (`coverage`), so a case that does not hold the
lengths it is meant to hold fails on the CPU.
"""
import numpy as np

from tests.emit_model import parse_record

DTYPES = {1: np.uint8, 2: np.int16, 4: np.int32, 8: np.int64}

# literal-run lengths every element size is tested with
LITS = [0, 1, 3, 4, 5, 14, 15, 16, 17, 63, 64, 65, 127, 128, 129, 269, 270, 271, 524, 525]
LONG_LIT = 3072
MATCHES = [4, 18, 19, 273, 274]
LONG_MATCH = 3000


def view(data, E):
    return data.view(DTYPES[E]) if E in DTYPES else data.view(np.dtype("V%d" % E))


def rand_bytes(rng, k, avoid=()):
    """k random bytes whose first and last are none of `avoid` (the run values
    next to them, which they would otherwise lengthen)."""
    b = rng.integers(0, 256, k, dtype=np.uint8)
    for i in ((0, k - 1) if k else ()):
        while int(b[i]) in avoid:
            b[i] = rng.integers(0, 256)
    return b


class Builder:
    def __init__(self, oracle, seed=1):
        self.o = oracle
        self.rng = np.random.default_rng(seed)
        self.x = {}     # literal length -> random bytes in front of the run
        self.val = 0

    def next_val(self):
        self.val = self.val % 251 + 1
        return self.val

    def tune(self, L):
        """Random bytes x so that [match][x random][byte run] parses with a
        literal run of exactly L bytes (L >= 1)."""
        if L in self.x:
            return self.x[L]
        for x in range(L - 1, max(L - 12, -1), -1):
            blk = np.concatenate([np.full(16, 0xF1, np.uint8), rand_bytes(self.rng, x, (0xF1, 0xF2)),
                                  np.full(80, 0xF2, np.uint8), rand_bytes(self.rng, 32, (0xF2,))])
            seqs, _ = parse_record(self.o.lz4_compress_block(blk), blk.size)
            if len(seqs) >= 2 and seqs[1][2] == L:
                self.x[L] = x
                return x
        raise AssertionError("no literal run of %d bytes" % L)

    def block(self, spec, n, tail_lits=None):
        """[(lit, ml)] -> an n-byte shuffled block: the sequences in order, then
        last literals (random) up to n, or a final match up to the block's last
        5 bytes when tail_lits == 0."""
        parts, prev, prev2 = [], None, None  # prev: the last run's byte value
        for lit, ml in spec:
            src = [q for q in parts if q.size >= 10 and q.min() != q.max()]
            if lit == 0 and src and prev is not None:
                # straight behind a match: a copy of bytes the search has
                # inserted (an earlier literal run's), found by the re-test
                q = src[-1]
                parts.append(q[2: 2 + min(ml, q.size - 2)].copy())
                v = None
            else:
                v = self.next_val()
                while v in (prev, prev2):
                    v = self.next_val()
                lit = max(lit, 1)
                x = self.tune(lit)
                parts.append(rand_bytes(self.rng, x, (v, prev if prev is not None else v)))
                parts.append(np.full(ml + lit - x, v, np.uint8))
            prev2, prev = prev, v
        used = sum(p.size for p in parts)
        assert used <= n, (used, n)
        if tail_lits == 0:
            parts.append(np.full(n - used, self.next_val(), np.uint8))
        else:
            parts.append(rand_bytes(self.rng, n - used, (prev,) if prev is not None else ()))
        out = np.concatenate(parts)
        assert out.size == n
        return out


def coverage(oracle, blocks):
    """(literal-run lengths incl. last literals, match lengths, sequence counts)
    of the oracle's parse of each shuffled block; blocks the oracle cannot
    shrink have no parse worth the name and count as 0 sequences."""
    lits, mls, counts = set(), set(), []
    for b in blocks:
        rec = oracle.lz4_compress_block(b)
        seqs, la = parse_record(rec, b.size)
        counts.append(len(seqs))
        lits.update(s[2] for s in seqs)
        lits.add(b.size - la)
        mls.update(s[3] for s in seqs)
    return lits, mls, counts


def unshuffle(oracle, blocks, E, block_elems):
    """Shuffled blocks (each block_elems * E bytes; the last may be a shorter
    multiple of 8 elements, followed by raw tail bytes) -> the codec's input."""
    sh = np.concatenate(blocks)
    return oracle.bitunshuffle(view(sh, E), block_elems)


def length_cases(oracle, E, seed=5):
    """Blocks of the default size for element size E that together hold every
    literal-run length of LITS, LONG_LIT, MATCHES and LONG_MATCH, and every
    destination x source alignment of a literal run."""
    bld = Builder(oracle, seed)
    be = oracle.default_block_size(E)
    n = be * E
    blocks = []
    # 1. the listed lengths, a few per block, each followed by a listed match
    spec, k = [], 0
    for lit in LITS[1:8] + [0] + LITS[8:]:
        spec.append((lit, MATCHES[k % len(MATCHES)]))
        k += 1
    blocks.append(bld.block(spec[:12], n))
    blocks.append(bld.block(spec[12:], n))
    # 2. G1's shape: one long run, a long match, short runs around them
    blocks.append(bld.block([(5, 40), (LONG_LIT, LONG_MATCH), (17, 30), (40, 9)], n))
    # 3. literal runs that end at the block end, and a block that ends in a match
    blocks.append(bld.block([(3, 600), (100, 700)], n, tail_lits=None))
    blocks.append(bld.block([(30, 100), (524, 100)], n, tail_lits=0))
    # 4. alignments: runs of 21..24 and 130..133 bytes (all four lengths mod 4)
    # behind matches of 5..11, so that source and destination drift apart
    al = [(21 + (i % 4), 5 + (3 * i + i // 4) % 7) for i in range(64)]
    blocks.append(bld.block(al, n))
    al = [(130 + (i % 4), 6 + (5 * i + i // 4) % 7) for i in range(50)]
    blocks.append(bld.block(al, n))
    # ... and runs of 300..303 bytes: the wave's 16-byte chunks at every
    # destination alignment, source granule offset and byte shift
    al = [(300 + (i % 4), 6 + (5 * i + i // 4) % 7) for i in range(24)]
    blocks.append(bld.block(al, n))
    return blocks, be


def count_cases(oracle, E, seed=9):
    """Blocks with 0, 1, 63, 64, 65, 255, 256 and 257 sequences."""
    bld = Builder(oracle, seed)
    be = oracle.default_block_size(E)
    n = be * E
    blocks = [bld.rng.integers(0, 256, n, dtype=np.uint8)]   # incompressible: 0 sequences
    for ns in (1, 63, 64, 65, 255, 256, 257):
        blocks.append(bld.block([(2 + i % 3, 8 + i % 5) for i in range(ns)], n))
    return blocks, be, [0, 1, 63, 64, 65, 255, 256, 257]
