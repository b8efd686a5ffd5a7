"""TEST INFRASTRUCTURE ONLY -- the kernel path every device entry point takes,
restated from bitshuffle_amd/csrc/dispatch.h and the kernels' in-kernel
branches.

A call's path depends on the element size E, the block's bytes and the low
four bits of the data and output pointers.  The launch-level decisions
(`enc_launch`, `dec_launch`, `transpose_tiles`) are compared with the host
build of dispatch.h by tests/test_dispatch_model.py; the functions below them
name, for the full blocks and for the partial block of one stream, the branch
the kernel then takes.  tests/dispatch_cases.py builds the GPU sweep's cells
from the thresholds here, never from literal sizes.

Path names carry no element size, so that the set of element sizes a path is
reached at can be counted.
"""
import functools

# ---- constants (dispatch.h; tests/test_dispatch_model.py compares them) ----
TABLE_BYTES = 16384
RAW_BYTES = 8192
STAGE_REG_BYTES = 8192
FAST_MAX_BLOCK_BYTES = 65536
U16_TABLE_LIMIT = 65536 + 12 - 1
DATA_PAD = 16
DESC_BYTES = 8 * 256
LDS_BYTES = 160 * 1024
TILE_GROUPS = 256
SREG_WORDS = 256
INPLACE_MARGIN = 704
CONST_ORDER = ("TABLE_BYTES", "RAW_BYTES", "STAGE_REG_BYTES", "FAST_MAX_BLOCK_BYTES", "U16_TABLE_LIMIT",
               "max_device_block_bytes", "max_lds_encode_bytes", "max_lds_decode_bytes", "DATA_PAD",
               "DESC_BYTES", "LDS_BYTES", "TILE_GROUPS", "SREG_WORDS", "INPLACE_MARGIN")


def lz4_bound(n):
    return n + n // 255 + 16


def max_device_block_bytes():
    return LDS_BYTES - TABLE_BYTES - 64


def max_lds_encode_bytes():
    return max_device_block_bytes()


def _dec_rec_bytes(maxlen):
    return (maxlen + 4 + 32 + 15) & ~15


@functools.lru_cache(maxsize=None)
def max_lds_decode_bytes():
    n = LDS_BYTES
    while n > 0:
        if ((n + 15) & ~15) + 16 + _dec_rec_bytes(lz4_bound(n)) <= LDS_BYTES:
            break
        n -= 8
    return n


def default_block_size(E):
    bs = 8192 // E // 8 * 8
    return max(bs, 128)


def ek_size(E):
    return E in (1, 2, 4, 8)


def align(residues):
    """(every pointer 16-aligned, every pointer 8-aligned)."""
    return all(r % 16 == 0 for r in residues), all(r % 8 == 0 for r in residues)


def align_state(residues):
    a16, a8 = align(residues)
    return "both" if a16 else "al8" if a8 else "neither"


def pick_ek(E, a16):
    return E if a16 and ek_size(E) else 0


def reg_groups(ek):
    return (8192 // (64 * 8 * ek)) * 64 if ek else 64


def reg_groups4(ek):
    it = 8192 // (64 * 32 * ek) if ek else 1
    return max(it, 1) * 64 * 4


def layout(nelem, bs):
    """(full blocks, elements of the partial block, tail elements)."""
    return nelem // bs, nelem % bs // 8 * 8, nelem % 8


# ---- launch-level decisions -------------------------------------------------
def enc_wide(block_bytes):
    return block_bytes >= U16_TABLE_LIMIT


def enc_desc(nmax):
    return not enc_wide(nmax) and 4 + lz4_bound(nmax) + 15 <= TABLE_BYTES


def fast_applies(block_bytes):
    return block_bytes <= FAST_MAX_BLOCK_BYTES


def fast_sreg(ek, nmax):
    nw = (nmax + 31) >> 5
    return ek not in (0, 8) and nmax % 32 == 0 and nw % 4 == 0 and nw <= SREG_WORDS


def enc_launch(E, block_bytes, last_bytes, residues):
    """What launch_encode (one residue) / launch_encode_batch decide."""
    a16, a8 = align(residues)
    ek = pick_ek(E, a16)
    desc = enc_desc(block_bytes)
    desc_off = ((block_bytes + 15) & ~15) + DATA_PAD
    return dict(ek=ek, raw8=a8 and E != 1, desc=desc, wide=enc_wide(block_bytes),
                wide_last=bool(last_bytes) and enc_wide(last_bytes),
                large=block_bytes > max_lds_encode_bytes(),
                lds=TABLE_BYTES + desc_off + (DESC_BYTES if desc else 0), desc_off=desc_off,
                fast=fast_applies(block_bytes), sreg=fast_sreg(ek, block_bytes))


def inplace_end(cap):
    return (cap + INPLACE_MARGIN + 15) & ~15


def dec_launch(E, block_bytes, residues, inplace=True, grec=False):
    """What launch_decode (one residue) / launch_decode_batch and decode_impl
    decide.  stage_off: 0 byte stores, -1 staged through registers, else the
    LDS offset of the staging block."""
    a16, a8 = align(residues)
    ek = pick_ek(E, a16)
    cap = (block_bytes + 15) & ~15
    if inplace:
        lds = inplace_end(cap) + 32
    else:
        lds = cap + 16 + (0 if grec else _dec_rec_bytes(lz4_bound(block_bytes)))
    stage = 0
    if ek == 0 and a8 and E != 1:
        if block_bytes <= STAGE_REG_BYTES:
            stage = -1
        elif lds + cap <= LDS_BYTES:
            stage = lds
            lds += cap
    return dict(large=block_bytes > max_lds_decode_bytes(), ek=ek, stage_off=stage, lds=lds, cap=cap)


def transpose_fast(E, in_res, out_res):
    return align((in_res, out_res))[0] and ek_size(E)


def rows16(P, ng):
    return P % 16 == 0 and ng % 16 == 0


# ---- paths of one block -----------------------------------------------------
def transpose_block(E, m, in_res, out_res, what):
    """bshuf_bitshuffle_dev / bshuf_bitunshuffle_dev (what: "shuf" /
    "unshuf") of a block of m elements."""
    P = m // 8
    tiles = "ntiles" if P > TILE_GROUPS else "1tile"
    if not transpose_fast(E, in_res, out_res):
        return "%s:generic/%s" % (what, tiles)
    # (P % 16 == 0 makes every tile's group count a multiple of 16)
    last_ng = P - (P - 1) // TILE_GROUPS * TILE_GROUPS
    return "%s:tiles/%s/%s" % (what, "rows16" if rows16(P, last_ng) else "rowsbytes", tiles)


def _enc_block(E, m, d, wide, note=""):
    n, P = m * E, m // 8
    ek = d["ek"]
    if ek:
        if P % 4 == 0 and P <= reg_groups4(ek):
            sub = "ek/fits4"
        elif P <= reg_groups(ek):
            sub = "ek/fits"
        else:
            sub = "ek/chunks"
    elif d["raw8"] and n <= RAW_BYTES:
        sub = "ek0/staged"
    elif E == 1 and d["a8"]:
        sub = "ek0/bytes/E1-rule"
    else:
        sub = "ek0/bytes"
    return "enc:%s/%s/%s%s" % (sub, "desc" if d["desc"] else "nodesc", "u32" if wide else "u16", note)


def _fast_block(E, m, d, res):
    P = m // 8
    ek = d["ek"]
    lay = "sreg" if d["sreg"] else "slots"
    if ek and P % 4 == 0 and P <= reg_groups4(ek):
        sub = "reg"
    elif d["sreg"]:
        sub = "direct"
    else:
        sub = ("words" if res % 8 == 0 else "bytes") + ("/E1" if E == 1 else "")
    return "fast:%s/%s/%s" % ("ek" if ek else "ek0", lay, sub)


def _dec_block(E, m, d):
    P = m // 8
    if d["ek"]:
        return "dec:ek/" + ("x4" if d["ek"] <= 4 and P % 4 == 0 else "groups")
    if d["stage_off"] < 0:
        return "dec:ek0/stage-regs"
    if d["stage_off"] > 0:
        return "dec:ek0/stage-lds"
    return "dec:ek0/bytes/E1-rule" if E == 1 and d["a8"] else "dec:ek0/bytes"


def _stream(full, last, nfull, m_last):
    return (full if nfull else None, last if m_last else None)


def _encode_stream(E, bs, nelem, res, d, fast):
    """One stream's (full, partial) paths under launch decisions d."""
    nfull, m_last, _ = layout(nelem, bs)
    if fast and d["fast"]:
        return _stream(_fast_block(E, bs, d, res), _fast_block(E, m_last, d, res), nfull, m_last)
    pre = "fast>exact " if fast else ""
    if d["large"]:
        # transposed into the workspace (16-aligned), parsed from there
        return _stream(pre + "enc:large/" + transpose_block(E, bs, res, 0, "shuf"),
                       pre + "enc:large/" + transpose_block(E, m_last, res, 0, "shuf"), nfull, m_last)
    wl = enc_wide(m_last * E)
    note = "/second-launch" if m_last and nfull and wl != d["wide"] else ""
    return _stream(pre + _enc_block(E, bs, d, d["wide"]), pre + _enc_block(E, m_last, d, wl, note), nfull, m_last)


# ---- entry points -------------------------------------------------------------
def encode(E, bs, nelem, in_res, out_res=0, fast=False):
    """bshuf_compress_lz4_dev / _fast_dev: (full blocks' path, partial block's
    path); None where the stream has no such block.  The output pointer picks
    no path (the compaction stores at any alignment)."""
    m_last = layout(nelem, bs)[1]
    d = enc_launch(E, bs * E, m_last * E, (in_res,))
    d["a8"] = in_res % 8 == 0
    return _encode_stream(E, bs, nelem, in_res, d, fast)


def encode_batch(E, bs, nelems, in_residues, fast=False):
    """bshuf_compress_lz4_batch_dev: (state, [(full, partial) per stream]).
    state: "both" / "al8" / "neither" for one launch over all streams with the
    alignment flags ANDed, or "per-stream" when the batch is split into single
    calls (large blocks, or a partial block of another table type)."""
    wide = enc_wide(bs * E)
    mixed = bs * E > max_lds_encode_bytes()
    for n in nelems:
        m_last = layout(n, bs)[1]
        mixed = mixed or (m_last and enc_wide(m_last * E) != wide)
    if mixed:
        return "per-stream", [encode(E, bs, n, r, 0, fast) for n, r in zip(nelems, in_residues)]
    d = enc_launch(E, bs * E, 0, in_residues)
    d["a8"] = align(in_residues)[1]
    return align_state(in_residues), [_encode_stream(E, bs, n, r, d, fast) for n, r in zip(nelems, in_residues)]


def _decode_stream(E, bs, nelem, res, d):
    nfull, m_last, _ = layout(nelem, bs)
    if d["large"]:
        # executed in global memory into the workspace, transposed from there
        return _stream("dec:large/" + transpose_block(E, bs, 0, res, "unshuf"),
                       "dec:large/" + transpose_block(E, m_last, 0, res, "unshuf"), nfull, m_last)
    return _stream(_dec_block(E, bs, d), _dec_block(E, m_last, d), nfull, m_last)


def decode(E, bs, nelem, in_res, out_res):
    """bshuf_decompress_lz4_dev: in_res is the stream's pointer (picks no path:
    records are read at any alignment), out_res the decoded data's."""
    d = dec_launch(E, bs * E, (out_res,))
    d["a8"] = out_res % 8 == 0
    return _decode_stream(E, bs, nelem, out_res, d)


def decode_batch(E, bs, nelems, out_residues):
    if bs * E > max_lds_decode_bytes():
        return "per-stream", [decode(E, bs, n, 0, r) for n, r in zip(nelems, out_residues)]
    d = dec_launch(E, bs * E, out_residues)
    d["a8"] = align(out_residues)[1]
    return align_state(out_residues), [_decode_stream(E, bs, n, r, d) for n, r in zip(nelems, out_residues)]


def transpose(E, bs, nelem, in_res, out_res, what):
    nfull, m_last, _ = layout(nelem, bs)
    return _stream(transpose_block(E, bs, in_res, out_res, what),
                   transpose_block(E, m_last, in_res, out_res, what), nfull, m_last)


def range_groups(E, bs, direct_residues, edges=True):
    """bshuf_decompress_lz4_ranges_dev: the decode pieces whose destination is
    16-byte aligned (every edge block's staging area is) go through one batch
    decode, the others through a second.  direct_residues: the output residues
    of the interior pieces.  ((state, path) of group one or None, of group two
    or None); pieces are whole blocks."""
    one = [r for r in direct_residues if r % 16 == 0] + ([0] if edges else [])
    two = [r for r in direct_residues if r % 16 != 0]

    def group(rs):
        if not rs:
            return None
        d = dec_launch(E, bs * E, rs)
        d["a8"] = align(rs)[1]
        return align_state(rs), _dec_block(E, bs, d)
    return group(one), group(two)


def window_path(E, bs):
    """The window decodes: every staging area is 16-byte aligned."""
    d = dec_launch(E, bs * E, (0,))
    d["a8"] = True
    return _dec_block(E, bs, d)
