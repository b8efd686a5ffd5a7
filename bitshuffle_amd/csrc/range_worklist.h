// range_worklist.h -- the work list of one decode piece, shared by the range
// and window decodes of one stream (k_range_worklist, lz4_range.hip) and the
// window decode over a set of streams (k_window_set_worklist, lz4_window.hip),
// whose pieces each name a stream of their own; and where a stream's verbatim
// tail starts, for the kernels that copy from it.
#pragma once

#include "launch.h"

namespace bshuf {

constexpr uint64_t kNoOffset = ~0ull;  // clamp_span's sentinel: -1001 without a read

__device__ __forceinline__ uint32_t be32_at(const uint8_t* p) {
    const gbl8c* q = (const gbl8c*)p;
    return ((uint32_t)q[0] << 24) | ((uint32_t)q[1] << 16) | ((uint32_t)q[2] << 8) | q[3];
}

// Where the verbatim tail of st starts: where the last block's header says its
// record ends (at 0 in a stream without blocks).  False when the header or the
// tail is not inside the stream (-91, as in the whole decode).
__device__ __forceinline__ bool tail_start(const RangeStream& st, uint64_t& ts) {
    const uint64_t N = (uint64_t)st.in_nbytes;
    ts = 0;
    if (st.nb > 0) {
        const uint64_t h = st.offs[st.nb - 1];
        if (h > N || N - h < 4) return false;
        ts = h + 4 + be32_at(st.in + h);
    }
    return ts <= N && N - ts >= (uint64_t)st.tail;
}

// Workgroups (blockIdx.y = 0 .. gridDim.y) share decode piece pc's blocks (a
// range of many blocks is one piece), work blocks [first, first + pc.nblk) of
// wl.  The piece's records lie in [B, end): B its first block's offset, end the
// offset of the block behind it -- or, for the stream's last block, where its
// header says its record ends.  Both come from an index the caller may have
// supplied, so both are forced into the stream and `end` to within nblk largest
// records of B; a block offset outside [B, end] becomes the sentinel.  With
// that, every token position the scan stores for the piece lies in its own area
// of nblk * (4 + maxlen) / 3 + 80 words (seq0 + o0 / 3 + i with o0 in [B, end]),
// and no byte outside [B, end) is read for it.
__device__ __forceinline__ void range_worklist_piece(const RangeStream& st, Seg* seg, const RangePiece& pc,
                                                     int64_t first, uint64_t* __restrict__ wl) {
    const uint64_t N = (uint64_t)st.in_nbytes;
    uint64_t B = st.offs[pc.b0];
    if (B > N) B = N;
    const uint64_t cap = (uint64_t)pc.nblk * (4 + (uint64_t)st.maxlen);
    const uint64_t lim = N - B < cap ? N : B + cap;
    const int64_t b1 = pc.b0 + pc.nblk;
    uint64_t end = lim;
    if (b1 < st.nb) {
        end = st.offs[b1];
    } else {
        const uint64_t h = st.offs[st.nb - 1];
        if (h >= B && h <= lim && lim - h >= 4) end = h + 4 + be32_at(st.in + h);
    }
    if (end < B || end > lim) end = lim;
    const int64_t stride = (int64_t)blockDim.x * gridDim.y;
    for (int64_t j = (int64_t)blockIdx.y * blockDim.x + threadIdx.x; j < pc.nblk; j += stride) {
        const uint64_t v = st.offs[pc.b0 + j];
        wl[first + j] = (v >= B && v <= end) ? v : kNoOffset;
    }
    if (threadIdx.x == 0 && blockIdx.y == 0) {
        seg->in_nbytes = (int64_t)end;
        seg->seq0 = pc.seq_base < 0 ? 0 : pc.seq_base - (int64_t)(B / 3);
    }
}

}  // namespace bshuf
