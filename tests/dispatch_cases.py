"""TEST INFRASTRUCTURE ONLY -- the cells of the dispatch sweep
(tests/test_gpu_dispatch.py), built from the thresholds of
tests/dispatch_model.py: element size x block-byte class x pointer offsets.

A class is a block size in bytes, rounded to whole 8-element groups of E (so
"the last size at most T" is T rounded down to a multiple of 8 E, "the first
above" the next multiple).  Classes that land on one size for an element size
are merged into one cell, named after all of them.
"""
import functools

import numpy as np

from tests import dispatch_model as M

ELEM_SIZES = (1, 2, 3, 4, 5, 8, 12, 16)
# (data, output) offsets into 16-aligned allocations
OFFSETS = ((0, 0), (8, 8), (4, 4), (1, 1), (0, 8), (8, 0), (0, 1), (1, 0))
# pointer residues of the three streams of a batch
BATCH_RESIDUES = ((0, 8, 1), (0, 8, 8), (0, 0, 0))
TAIL_ELEMS = 5
CANARY = 64
FILL = 0xA5


def at_most(T, E):
    """Bytes of the largest block of at most T bytes (at least one group)."""
    return max(T // (8 * E), 1) * 8 * E


def above(T, E):
    return at_most(T, E) + 8 * E


def _last_true(pred, E, hi):
    """Largest multiple n of 8 E, n <= hi, with pred(n); pred is monotone
    (true below a threshold)."""
    lo, hi = 1, hi // (8 * E)
    assert pred(lo * 8 * E) and not pred((hi + 1) * 8 * E)
    while lo < hi:
        mid = (lo + hi + 1) // 2
        if pred(mid * 8 * E):
            lo = mid
        else:
            hi = mid - 1
    return lo * 8 * E


def _stage_lds_fits(n):
    # the decoder's staging of an 8-aligned, not 16-aligned output (E != 1)
    return M.dec_launch(3, n, (8,))["stage_off"] != 0


@functools.lru_cache(maxsize=None)
def class_sizes(E):
    """[(class name, block bytes)]: the sizes on both sides of every threshold
    at which a launcher or a kernel takes another path."""
    P8k = M.STAGE_REG_BYTES // (8 * E)
    while P8k % 4 == 0:
        P8k -= 1
    desc_last = _last_true(M.enc_desc, E, M.U16_TABLE_LIMIT)
    stage_last = _last_true(_stage_lds_fits, E, M.max_lds_decode_bytes() + 8 * E)
    out = [
        ("p1", 8 * E),
        ("p3", 24 * E),
        ("default", M.default_block_size(E) * E),
        ("le8k_p_not4", P8k * 8 * E),
        ("gt8k", above(M.STAGE_REG_BYTES, E)),
        ("desc_last", desc_last),
        ("desc_first_not", desc_last + 8 * E),
        ("48k", at_most(48 * 1024, E)),
        ("stage_lds_last", stage_last),
        ("stage_lds_first_not", stage_last + 8 * E),
        ("fast_max", at_most(M.FAST_MAX_BLOCK_BYTES, E)),
        ("fast_max_next", above(M.FAST_MAX_BLOCK_BYTES, E)),
        ("u16_last", at_most(M.U16_TABLE_LIMIT - 1, E)),
        ("u16_first", above(M.U16_TABLE_LIMIT - 1, E)),
        ("dec_lds_max", at_most(M.max_lds_decode_bytes(), E)),
        ("dec_lds_next", above(M.max_lds_decode_bytes(), E)),
        ("dev_max", at_most(M.max_device_block_bytes(), E)),
        ("dev_next", above(M.max_device_block_bytes(), E)),
        # the first large block whose group count is a multiple of 16: the
        # 16-byte rows of the large path's transposes over more than one tile
        ("large_p16", -(-(M.max_device_block_bytes() // (8 * E) + 1) // 16) * 16 * 8 * E),
    ]
    return out


def classes(E):
    """[(merged class name, block bytes)]: one entry per distinct size."""
    by_size = {}
    for name, n in class_sizes(E):
        by_size.setdefault(n, []).append(name)
    return [("+".join(names), n) for n, names in sorted(by_size.items())]


def class_bytes(E, name):
    return dict(classes(E))[name]


def cells():
    """[(E, class name, block bytes)] of the whole sweep."""
    return [(E, name, n) for E in ELEM_SIZES for name, n in classes(E)]


def fast_cells():
    """The fast encoder's: block classes up to kFastMaxBlockBytes and the one
    size above it."""
    out = []
    for E in ELEM_SIZES:
        nxt = above(M.FAST_MAX_BLOCK_BYTES, E)
        out += [(E, name, n) for name, n in classes(E) if n <= nxt]
    return out


def partial_groups(P):
    """Groups of the partial block: the largest count below P that is not a
    multiple of 4 (0: the block has no room for one)."""
    g = P - 1
    while g > 0 and g % 4 == 0:
        g -= 1
    return g


def stream_elems(E, block_bytes, nfull=3, small_partial=False):
    """Elements of a cell's stream: nfull full blocks, a partial block whose
    group count is not a multiple of 4, a raw tail of 5 elements.
    small_partial: a partial block of 7 groups at the most (for blocks that
    need the byU32 table: one that needs byU16)."""
    bs = block_bytes // E
    g = partial_groups(bs // 8)
    if small_partial:
        g = min(g, 7)
    return nfull * bs + 8 * g + TAIL_ELEMS


def streams(E, block_bytes, three=False):
    """[(name, elements)] of a cell's streams (three: at least three, for the
    batch calls -- the test gives every stream bytes of its own).  Blocks above
    8 KiB, whose partial block can take another in-kernel path than the full
    ones, add one with a
    partial block of 7 groups (register prefetch one group per lane, or raw
    staging; for blocks that need the byU32 table the byU16 partial block of a
    second launch) and one of 16 groups (four groups per lane; 16-byte rows in
    the large path's transposes)."""
    bs = block_bytes // E
    out = [("main", stream_elems(E, block_bytes))]
    if block_bytes > M.RAW_BYTES:
        out.append(("small_partial", stream_elems(E, block_bytes, small_partial=True)))
        out.append(("partial16", 3 * bs + 8 * 16 + TAIL_ELEMS))
    elif three:
        out += [("second", out[0][1]), ("third", out[0][1])]
    return out


def stream_bytes(E, block_bytes, seed, nelem):
    """The raw bytes of a stream: blocks alternate between a slow byte walk,
    random bytes and zeros, so the encoder's deferred copy-out meets an
    incompressible record beside staged raw bytes and the reverse."""
    rng = np.random.default_rng(seed)
    total = nelem * E
    out = np.empty(total, dtype=np.uint8)
    at, k = 0, 0
    while at < total:
        n = min(block_bytes, total - at)
        kind = k % 3
        if kind == 0:
            out[at:at + n] = (rng.integers(-2, 3, n).cumsum() % 7).astype(np.uint8)
        elif kind == 1:
            out[at:at + n] = rng.integers(0, 256, n, dtype=np.uint8)
        else:
            out[at:at + n] = 0
        at += n
        k += 1
    return out


def view_e(raw, E):
    """The byte array as E-byte elements."""
    if E == 1:
        return raw
    if E in (2, 4, 8):
        return raw.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[E])
    return raw.view(np.dtype("V%d" % E))


def header_walk(stream, nblocks):
    """Byte offset of every block's header in a framed stream."""
    offs, pos = [], 0
    for _ in range(nblocks):
        offs.append(pos)
        pos += 4 + int.from_bytes(stream[pos:pos + 4].tobytes(), "big")
    return offs


# ---- transposes -----------------------------------------------------------------
def transpose_extra_blocks():
    """Block sizes (elements) of more than 256 groups, so that a tile boundary
    falls inside a block: one with P % 16 == 0, one with P % 16 != 0."""
    return [("tile_p16", (M.TILE_GROUPS + 16) * 8), ("tile_p_odd", (M.TILE_GROUPS + 13) * 8)]


# ---- ranges ------------------------------------------------------------------------
RANGE_ELEM_SIZES = (1, 2, 3, 4, 8)
RANGE_OUT_SHIFTS = (0, 8, 3)
RANGE_BLOCK = 128  # elements


def range_lists(E, bs=RANGE_BLOCK, nblocks=12):
    """{name: [(start, count)]} over a stream of nblocks blocks of bs elements
    plus a partial block and a tail.  A range that starts on a block boundary
    and covers whole blocks is one direct (interior) piece at the output offset
    where the range lands; the ranges in front of it set that offset.

    residues: direct pieces at output residues 0, 8, 4 and odd (by leading
              ranges of 16 / E-free byte counts);
    al8:      every direct piece not 16-aligned is 8-aligned, so the second
              group takes the staged path (E = 2, 4, 8 as EK = 0) or, for
              E = 1, byte stores."""
    def lead(nbytes):
        # a range of `nbytes` bytes (whole elements) inside block 0, clear of
        # its boundaries: an edge piece
        assert nbytes % E == 0
        return (1, nbytes // E)

    def pad_to(res, at):
        """Leading ranges that move the output offset `at` to residue res mod 16."""
        for k in range(E):
            need = (res - at) % 16 + 16 * k
            if need % E == 0:
                return need  # whole elements
        return None  # E does not reach this residue from here

    lists = {}
    # residues 0, 8, 4, odd (as far as E divides them: 3-byte elements reach
    # every residue, 8-byte ones 0 and 8)
    seq, at = [], 0
    blk = 1
    for res in (0, 8, 4, 1):
        need = pad_to(res, at)
        if need is None:
            continue
        if need:
            seq.append(lead(need))
            at += need
        seq.append((blk * bs, 2 * bs))
        at += 2 * bs * E
        blk += 2
    lists["residues"] = seq
    seq, at, blk = [], 0, 1
    for res in (8, 0, 8):
        need = pad_to(res, at)
        assert need is not None
        if need:
            seq.append(lead(need))
            at += need
        seq.append((blk * bs, 2 * bs))
        at += 2 * bs * E
        blk += 2
    lists["al8"] = seq
    return lists


def direct_residues(E, ranges, shift, bs=RANGE_BLOCK):
    """Output residues (mod 16) of the direct pieces of `ranges` with `out`
    `shift` bytes into a 16-aligned allocation."""
    res, at = [], shift
    for start, count in ranges:
        first = -(-start // bs) * bs
        end = (start + count) // bs * bs
        if end > first:
            res.append((at + (first - start) * E) % 16)
        at += count * E
    return res
