"""TEST INFRASTRUCTURE ONLY -- numpy restatement of "fast parse v1"
(DESIGN.md §6.6), the rule behind mode="fast" / bshuf_compress_lz4_fast*.

For one bit-transposed block s of L bytes of E-byte elements, P = L / (8 E):

* offsets D = sorted distinct values of {1, 2, 3, 4, 8, P, 2P} that are < L;
* run_d(p) = number of consecutive q >= p with q < L, q >= d, s[q] == s[q-d];
  the capped run is min(run_d(p), L - 5 - p);
* L < 13: one literal-only sequence;
* else anchor = 0, ip = 1, and repeatedly: p = the smallest position >= ip with
  p <= L - 12 whose largest capped run over D is >= 4 (none: stop); the match
  takes the offset of the largest capped run, ties to the smaller offset, and
  that run as its length; literals [anchor, p) + the match are emitted;
  anchor = ip = p + length;
* the last sequence is literals [anchor, L);
* token, length bytes and little-endian offset as in the LZ4 block format.

Framing, block splitting, the partial last block and the verbatim tail are the
exact encoder's.  Blocks above 65536 bytes are not covered by the rule (the
fast entry points take the exact parse for them).
"""
import numpy as np

FAST_PARSE_VERSION = 1
FAST_MAX_BLOCK_BYTES = 65536
SMALL_OFFSETS = (1, 2, 3, 4, 8)


def offsets(L, E):
    P = L // (8 * E)
    return sorted(d for d in set(SMALL_OFFSETS + (P, 2 * P)) if 0 < d < L)


def _capped_runs(s, d):
    """Capped run of offset d at every position (int32 array of len(s))."""
    L = s.size
    ok = np.zeros(L, dtype=bool)
    ok[d:] = s[d:] == s[:-d]
    ok[max(L - 5, 0):] = False  # the cap: a run never reaches into the last 5 bytes
    idx = np.arange(L, dtype=np.int64)
    # first position >= p where ok is False
    stop = np.where(ok, L, idx)
    stop = np.minimum.accumulate(stop[::-1])[::-1]
    return stop - idx


def _len_bytes(v):
    return [255] * (v // 255) + [v % 255]


def parse(s, E):
    """[(literal start, literal length, offset, match length)] of the block,
    the last entry with offset 0 and match length 0."""
    s = np.ascontiguousarray(s, dtype=np.uint8).reshape(-1)
    L = s.size
    if L < 13:
        return [(0, L, 0, 0)]
    D = offsets(L, E)
    runs = np.stack([_capped_runs(s, d) for d in D])
    which = np.argmax(runs, axis=0)  # first maximum = smallest offset
    best = runs[which, np.arange(L)]
    start = best >= 4
    start[0] = False
    start[L - 12 + 1:] = False
    idx = np.arange(L, dtype=np.int64)
    nxt = np.where(start, idx, L)
    nxt = np.minimum.accumulate(nxt[::-1])[::-1]  # next match start at or after p
    seqs = []
    anchor, ip = 0, 1
    while ip < L:
        p = int(nxt[ip])
        if p >= L:
            break
        n = int(best[p])
        seqs.append((anchor, p - anchor, int(D[which[p]]), n))
        anchor = ip = p + n
    seqs.append((anchor, L - anchor, 0, 0))
    return seqs


def encode_block(s, E):
    """The LZ4 payload (uint8 array) of one bit-transposed block."""
    s = np.ascontiguousarray(s, dtype=np.uint8).reshape(-1)
    out = bytearray()
    for a, ll, d, ml in parse(s, E):
        m = ml - 4 if d else 0
        out.append((min(ll, 15) << 4) | min(m, 15))
        if ll >= 15:
            out += bytes(_len_bytes(ll - 15))
        out += s[a:a + ll].tobytes()
        if d:
            out += bytes((d & 255, d >> 8))
            if m >= 15:
                out += bytes(_len_bytes(m - 15))
    return np.frombuffer(bytes(out), dtype=np.uint8)


def blocks(oracle, arr, block_size=0):
    """(element offset, element count) of every block of the framed stream,
    and the count of leftover elements copied verbatim behind them."""
    n, E = arr.size, arr.dtype.itemsize
    bs = block_size or oracle.default_block_size(E)
    if bs % 8:
        raise ValueError("block size must be a multiple of 8")
    out = [(i * bs, bs) for i in range(n // bs)]
    last = (n % bs) // 8 * 8
    if last:
        out.append((n // bs * bs, last))
    return out, n % 8


def compress_lz4(oracle, arr, block_size=0, cache=None):
    """The framed fast stream of `arr` (uint8 array); `oracle` supplies the bit
    transpose and the default block size.  `cache` (a dict) remembers payloads
    by block content, for inputs made of many repeated blocks."""
    arr = np.ascontiguousarray(arr).reshape(-1)
    E = arr.dtype.itemsize
    bs = block_size or oracle.default_block_size(E)
    if bs * E > FAST_MAX_BLOCK_BYTES:
        return oracle.compress_lz4(arr, block_size)
    blks, left = blocks(oracle, arr, block_size)
    shuf = oracle.bitshuffle(arr, bs).view(np.uint8).reshape(-1) if arr.size else arr.view(np.uint8)
    out = bytearray()
    for off, m in blks:
        s = shuf[off * E:(off + m) * E]
        key = s.tobytes()
        rec = cache.get(key) if cache is not None else None
        if rec is None:
            payload = encode_block(s, E)
            rec = int(payload.size).to_bytes(4, "big") + payload.tobytes()
            if cache is not None:
                cache[key] = rec
        out += rec
    if left:
        out += arr[arr.size - left:].view(np.uint8).tobytes()
    return np.frombuffer(bytes(out), dtype=np.uint8)


def block_records(stream, oracle, arr, block_size=0):
    """[(block bytes L, payload)] of a framed stream of `arr`."""
    arr = np.ascontiguousarray(arr).reshape(-1)
    E = arr.dtype.itemsize
    blks, _ = blocks(oracle, arr, block_size)
    pos, out = 0, []
    for _, m in blks:
        c = int.from_bytes(stream[pos:pos + 4].tobytes(), "big")
        out.append((m * E, stream[pos + 4:pos + 4 + c]))
        pos += 4 + c
    return out
