// lz4_range.hip -- the kernels around the block decode of a range decode
// (bshuf_decompress_lz4_ranges_dev; launch.h, "range decode").  The blocks
// themselves are decoded by the batch decoder's k_seq_scan + k_lz4_decode
// (lz4_decode.hip), unchanged: here are only the work list it reads, the copy
// of the partly covered blocks' clips and of the verbatim tail, and the result.
#include "launch.h"
#include "range_worklist.h"

namespace bshuf {

namespace {

// Piece blockIdx.x of the ONE stream st (range_worklist.h).
__global__ __launch_bounds__(256) void k_range_worklist(RangeStream st, Seg* __restrict__ segs,
                                                        const RangePiece* __restrict__ pcs, int na,
                                                        int64_t nblk_a, uint64_t* __restrict__ wl) {
    const int p = blockIdx.x;
    range_worklist_piece(st, segs + p, pcs[p], segs[p].first + (p >= na ? nblk_a : 0), wl);
}

// n bytes src -> dst by the workgroup: 16-byte loads and stores when the two
// are congruent mod 16 (the bytes up to dst's first 16-byte boundary and
// behind its last one singly), else byte by byte.  Nothing outside [0, n) of
// either is touched.
__device__ __forceinline__ void wg_copy(const uint8_t* src, uint8_t* dst, int64_t n) {
    const gbl8c* s8 = (const gbl8c*)src;
    gbl8* d8 = (gbl8*)dst;
    const int64_t t = threadIdx.x, T = blockDim.x;
    if ((((uintptr_t)src ^ (uintptr_t)dst) & 15) != 0 || n < 32) {
        for (int64_t i = t; i < n; i += T) d8[i] = s8[i];
        return;
    }
    const int64_t head = (int64_t)((16 - ((uintptr_t)dst & 15)) & 15);
    const int64_t nv = (n - head) >> 4;
    if (t < head) d8[t] = s8[t];
    const gbl128c* s16 = (const gbl128c*)(src + head);
    gbl128* d16 = (gbl128*)(dst + head);
    for (int64_t i = t; i < nv; i += T) d16[i] = s16[i];
    for (int64_t i = head + 16 * nv + t; i < n; i += T) d8[i] = s8[i];
}

// One workgroup per piece.  Edge: the clip of the staging block, when the
// block decoded.  Tail span: from the stream's verbatim tail (tail_start,
// range_worklist.h); a tail that is not inside the stream is -91 and nothing
// is copied.
__global__ __launch_bounds__(256) void k_range_edges(RangeStream st, const RangePiece* __restrict__ pcs,
                                                     int64_t* __restrict__ res) {
    const int p = blockIdx.x;
    const RangePiece pc = pcs[p];
    if (pc.kind == kPieceInterior) return;
    const uint8_t* src = pc.src;
    if (pc.kind == kPieceEdge) {
        if (res[p] < 0) return;
    } else {
        uint64_t ts;
        const bool ok = tail_start(st, ts);
        if (threadIdx.x == 0) res[p] = ok ? pc.n : -91;
        if (!ok) return;
        src = st.in + ts + pc.lo;
    }
    wg_copy(src, pc.dst, pc.n);
}

__global__ __launch_bounds__(256) void k_range_reduce(const int64_t* __restrict__ res, int np,
                                                      const int64_t* idx_err, int64_t total,
                                                      int64_t* result) {
    __shared__ int bad;
    if (threadIdx.x == 0) bad = -1;
    __syncthreads();
    int m = -1;
    for (int p = threadIdx.x; p < np; p += blockDim.x)
        if (res[p] < 0) m = p;
    if (m >= 0) atomicMax(&bad, m);
    __syncthreads();
    if (threadIdx.x == 0) *result = (idx_err && *idx_err != 0) ? -91 : (bad >= 0 ? res[bad] : total);
}

}  // namespace

hipError_t launch_range_worklist(const RangeStream& st, Seg* segs, const RangePiece* pcs, int nd, int na,
                                 int64_t nblk_a, int64_t max_blk, uint64_t* wl, hipStream_t s) {
    if (nd <= 0) return hipSuccess;
    // 1024 blocks of the largest piece per workgroup, at most 64 per piece
    const unsigned ny = (unsigned)std::min<int64_t>(64, std::max<int64_t>(1, (max_blk + 1023) / 1024));
    ProfScope prof("k_range_worklist", s);
    hipLaunchKernelGGL(k_range_worklist, dim3((unsigned)nd, ny), dim3(256), 0, s, st, segs, pcs, na, nblk_a,
                       wl);
    return hipGetLastError();
}

hipError_t launch_range_edges(const RangeStream& st, const RangePiece* pcs, int64_t* res, int np,
                              hipStream_t s) {
    if (np <= 0) return hipSuccess;
    ProfScope prof("k_range_edges", s);
    hipLaunchKernelGGL(k_range_edges, dim3((unsigned)np), dim3(256), 0, s, st, pcs, res);
    return hipGetLastError();
}

hipError_t launch_range_reduce(const int64_t* res, int np, const int64_t* idx_err, int64_t total,
                               int64_t* result, hipStream_t s) {
    ProfScope prof("k_range_reduce", s);
    hipLaunchKernelGGL(k_range_reduce, dim3(1), dim3(256), 0, s, res, np, idx_err, total, result);
    return hipGetLastError();
}

}  // namespace bshuf
