// range_plan.h -- one element range of a framed stream as pieces (host only,
// no HIP: the CPU suite builds it into libbshuf_hostcheck.so).
//
// The stream of `size` elements in blocks of `bs` (plan.h, make_plan): nfull =
// size / bs full blocks, one partial block of last = size % bs - size % 8
// elements when that is not 0, then size % 8 verbatim tail elements.  The
// blocks cover elements [0, nfull * bs + last).  A range [start, start + count)
// goes to `dst0` (a byte offset of the dense output) as, in element order:
//   head edge  the block the range enters part-way (its clip [lo, hi) in
//              elements of the block), decoded whole into a staging block;
//   interior   whole blocks [b0, b1) decoded straight to their place (the
//              partial block counts as whole when the range covers all of it);
//   tail edge  the block the range leaves part-way;
//   tail span  the range's part of the verbatim tail, copied from the stream.
// A range inside one block has one edge: the head edge when it starts inside
// the block, else the tail edge.  Absent pieces have n == 0 (b1 == b0).
#pragma once

#include <stdint.h>

namespace bshuf {

struct RangeEdge {
    int64_t blk;     // block of the stream
    int64_t lo, hi;  // clip, elements of the block
    int64_t dst;     // byte offset of element lo's copy in the output
};

struct RangePieces {
    RangeEdge head, tail;     // present when hi > lo
    int64_t b0, b1, int_dst;  // interior blocks and the byte offset of block b0's copy
    int64_t tail_lo, tail_n;  // tail span: elements [tail_lo, tail_lo + tail_n) of the verbatim tail
    int64_t tail_dst;
};

// start + count <= size (checked by the caller)
inline void range_pieces(int64_t size, int64_t bs, int64_t E, int64_t start, int64_t count,
                         int64_t dst0, RangePieces& r) {
    const int64_t nfull = size / bs;
    const int64_t last = size % bs - size % 8;
    const int64_t covered = nfull * bs + last;  // the blocks' elements
    const int64_t nb = nfull + (last ? 1 : 0);
    const int64_t end = start + count;
    const int64_t s = start < covered ? start : covered, e = end < covered ? end : covered;
    auto dst_of = [&](int64_t elem) { return dst0 + (elem - start) * E; };
    r = RangePieces{};
    if (s < e) {
        const int64_t kb = s / bs;  // the block of the first element
        const bool ends_block = e == covered || e % bs == 0;
        r.b0 = (s + bs - 1) / bs;
        r.b1 = e == covered ? nb : e / bs;
        if (r.b1 < r.b0) r.b1 = r.b0;  // inside one block
        r.int_dst = dst_of(r.b0 * bs);
        if (s % bs) {
            const int64_t bend = (kb + 1) * bs < covered ? (kb + 1) * bs : covered;
            r.head = RangeEdge{kb, s - kb * bs, (e < bend ? e : bend) - kb * bs, dst_of(s)};
        }
        const int64_t ke = e / bs;  // the block holding element e
        if (!ends_block && !(ke == kb && s % bs)) {
            const int64_t from = s > ke * bs ? s : ke * bs;
            r.tail = RangeEdge{ke, from - ke * bs, e - ke * bs, dst_of(from)};
        }
    }
    if (end > covered && count > 0) {
        const int64_t from = start > covered ? start : covered;
        r.tail_lo = from - covered;
        r.tail_n = end - from;
        r.tail_dst = dst_of(from);
    }
}

}  // namespace bshuf
