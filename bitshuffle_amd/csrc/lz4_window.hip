// lz4_window.hip -- the kernels around the block decode of a window decode
// (bshuf_decompress_lz4_windows_dev, bshuf_decompress_lz4_windows_set_dev,
// bshuf_lz4_stream_set_dev; launch.h, "window decode"): K windows of one length
// whose starts -- and, over a set of streams, stream indices -- live in device
// memory.  k_window_plan turns them into the tables the range decode's host plan
// would have uploaded; the work list is the range decode's (one stream) or
// k_window_set_worklist (a stream per window); the token scan and the block
// decode are the batch decoder's, unchanged; k_window_gather copies every
// window out of its staging area and its stream's verbatim tail,
// k_window_reduce makes the result.  The plan and gather kernels are
// instantiated once per source (WindowStream, WindowSet): what follows is what
// the two sources answer, then the kernels that ask.
#include "launch.h"
#include "range_worklist.h"
#include "window_copy.h"
#include "window_plan.h"

namespace bshuf {

namespace {

// ---- the sources ----------------------------------------------------------
// For the plan: window i's WindowPlan; returns the stream its blocks are read from.
__device__ __forceinline__ const uint8_t* source_plan(const WindowStream& src, const WindowCall& c, int i,
                                                      WindowPlan& w) {
    window_plan(src.size, c.bs, c.E, c.window, c.starts[i], w);
    return src.st.in;
}

// A bad window gets blocks [0, Mw) of the set's stream `ref` and nothing to
// copy; when the set is not the one the call describes, every window is bad and
// has no stream at all (sidx -1).
__device__ __forceinline__ const uint8_t* source_plan(const WindowSet& src, const WindowCall& c, int i,
                                                      WindowPlan& w) {
    const StreamSetHeader h = *src.hdr;
    const bool match = h.magic == kStreamSetMagic && h.count == src.count && h.E == c.E && h.bs == c.bs &&
                       h.nb_max == src.nb_max;
    const int64_t id = src.ids[i];
    const bool known = match && id >= 0 && id < src.count;
    window_set_plan(match ? src.count : 0, id, known ? src.recs[id].size : 0, c.bs, c.E, c.window, c.starts[i],
                    c.Mw, w);
    int32_t s = (int32_t)id;
    if (w.bad) {
        s = match && h.ref >= 0 && h.ref < src.count ? (int32_t)h.ref : -1;
        if (s >= 0) window_plan_blocks(src.recs[s].size, c.bs, c.E, c.window, 0, c.Mw, true, w);
    }
    src.sidx[i] = s;
    return s >= 0 ? src.recs[s].st.in : (const uint8_t*)src.hdr;  // (never read without a stream)
}

// ProfScope names: the ones the two calls had with kernels of their own.
struct Names {
    const char *plan, *gather;
};
constexpr Names names(const WindowStream&) { return {"k_window_plan", "k_window_gather"}; }
constexpr Names names(const WindowSet&) { return {"k_window_set_plan", "k_window_set_gather"}; }

// ---- the kernels ----------------------------------------------------------
// One thread per window.  A bad window of one stream (start out of range) gets
// block 0 on and nothing to copy.
template <class Source>
__global__ __launch_bounds__(256) void k_window_plan(Source src, WindowCall c, Seg* __restrict__ segs,
                                                     RangePiece* __restrict__ pcs,
                                                     WindowTail* __restrict__ wt) {
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= c.K) return;
    WindowPlan w;
    const uint8_t* in = source_plan(src, c, i, w);
    write_window(c, i, w, in, c.out + (int64_t)i * c.wbytes, segs, pcs, wt);
}

// Workgroups (p, 0 .. gridDim.y) share window p's Mw work blocks.
__global__ __launch_bounds__(256) void k_window_set_worklist(WindowSet src, int64_t Mw, Seg* __restrict__ segs,
                                                             const RangePiece* __restrict__ pcs,
                                                             uint64_t* __restrict__ wl) {
    const int p = blockIdx.x;
    const RangePiece pc = pcs[p];
    const int64_t first = (int64_t)p * Mw;
    const int32_t s = src.sidx[p];
    if (s < 0) {
        // no stream: an empty one, every block at the sentinel
        const int64_t stride = (int64_t)blockDim.x * gridDim.y;
        for (int64_t j = (int64_t)blockIdx.y * blockDim.x + threadIdx.x; j < pc.nblk; j += stride)
            wl[first + j] = kNoOffset;
        if (threadIdx.x == 0 && blockIdx.y == 0) {
            segs[p].in_nbytes = 0;
            segs[p].seq0 = pc.seq_base;
        }
        return;
    }
    const RangeStream st = src.recs[s].st;
    range_worklist_piece(st, segs + p, pc, first, wl);
}

// T lanes per window, 256 / T windows per workgroup; the status and the copy
// (Op: SpanCopy) or the conversion (SpanCvt): window_gather_one (window_copy.h).
template <int T, class Source, class Op>
__global__ __launch_bounds__(256) void k_window_gather(Source src, WindowCall c,
                                                       const RangePiece* __restrict__ pcs,
                                                       const WindowTail* __restrict__ wt,
                                                       const int64_t* __restrict__ dstat,
                                                       int64_t* __restrict__ wstat, Op op) {
    const int i = (int)(blockIdx.x * (256 / T) + threadIdx.x / T);
    const int t = (int)(threadIdx.x % T);
    if (i >= c.K) return;
    const WindowTail w = wt[i];
    int64_t err;
    const RangeStream st = source_stream(src, w, i, err);
    window_gather_one(st, err, w, pcs, i, w.t1 > w.t0 ? c.res[i] : 0, dstat + (int64_t)i * c.Mw, c.wbytes,
                      wstat, t, T, op, c.out);
}

__global__ __launch_bounds__(256) void k_stream_set_status(StreamSetRec* __restrict__ recs,
                                                           const int64_t* __restrict__ idx_err,
                                                           int64_t* __restrict__ status, int count) {
    const int s = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (s >= count) return;
    const int64_t e = idx_err[s] != 0 ? -91 : 0;
    recs[s].err = e;
    status[s] = e;
}

__global__ __launch_bounds__(256) void k_window_reduce(const int64_t* __restrict__ wstat,
                                                       const WindowTail* __restrict__ wt, int K,
                                                       const int64_t* idx_err, int64_t total,
                                                       const int64_t* dtotal, int64_t* result) {
    __shared__ int bad, oob;
    if (threadIdx.x == 0) {
        bad = -1;
        oob = 0;
    }
    __syncthreads();
    int m = -1, o = 0;
    for (int i = threadIdx.x; i < K; i += blockDim.x) {
        if (wstat[i] < 0) m = i;
        o |= wt[i].bad;
    }
    if (m >= 0) atomicMax(&bad, m);
    if (o) atomicOr(&oob, 1);
    __syncthreads();
    // (dtotal: the total is device-held, `total` bytes for each of *dtotal elements)
    if (threadIdx.x == 0)
        *result = (idx_err && *idx_err != 0)
                      ? -91
                      : (oob ? -71 : (bad >= 0 ? wstat[bad] : (dtotal ? *dtotal * total : total)));
}

}  // namespace

template <class Source>
hipError_t launch_window_plan(const Source& src, const WindowCall& c, Seg* segs, RangePiece* pcs,
                              WindowTail* wt, hipStream_t s) {
    ProfScope prof(names(src).plan, s);
    hipLaunchKernelGGL(k_window_plan<Source>, dim3((unsigned)((c.K + 255) / 256)), dim3(256), 0, s, src, c, segs,
                       pcs, wt);
    return hipGetLastError();
}

hipError_t launch_window_set_worklist(const WindowSet& src, const WindowCall& c, Seg* segs,
                                      const RangePiece* pcs, uint64_t* wl, hipStream_t s) {
    if (c.K <= 0 || c.Mw <= 0) return hipSuccess;
    // 1024 blocks of a window per workgroup, at most 64 per window (launch_range_worklist)
    const unsigned ny = (unsigned)std::min<int64_t>(64, std::max<int64_t>(1, (c.Mw + 1023) / 1024));
    ProfScope prof("k_window_set_worklist", s);
    hipLaunchKernelGGL(k_window_set_worklist, dim3((unsigned)c.K, ny), dim3(256), 0, s, src, c.Mw, segs, pcs,
                       wl);
    return hipGetLastError();
}

template <class Source>
hipError_t launch_window_gather(const Source& src, const WindowCall& c, const RangePiece* pcs,
                                const WindowTail* wt, const int64_t* dstat, int64_t* wstat, hipStream_t s,
                                const CvtArgs* cvt) {
    ProfScope prof(names(src).gather, s);
    // a wave per window up to 2 KiB (two 16-byte chunks per lane), else a
    // workgroup: a short window would leave most of a workgroup's four waves
    // with nothing to copy.  A converting gather goes by the larger of the
    // window's source and destination bytes (cvt_lane_bytes), so that a lane
    // of the wave has at most two chunks to store: not measured.
    const bool wave = cvt_lane_bytes(cvt, c.wbytes) <= 2048;
    auto go = [&](auto op) {
        using Op = decltype(op);
        if (wave)
            hipLaunchKernelGGL((k_window_gather<64, Source, Op>), dim3((unsigned)((c.K + 3) / 4)), dim3(256), 0, s,
                               src, c, pcs, wt, dstat, wstat, op);
        else
            hipLaunchKernelGGL((k_window_gather<256, Source, Op>), dim3((unsigned)c.K), dim3(256), 0, s, src, c,
                               pcs, wt, dstat, wstat, op);
    };
    if (cvt)
        cvt_dispatch(*cvt, go);
    else
        go(SpanCopy{});
    return hipGetLastError();
}

template hipError_t launch_window_plan(const WindowStream&, const WindowCall&, Seg*, RangePiece*, WindowTail*,
                                       hipStream_t);
template hipError_t launch_window_plan(const WindowSet&, const WindowCall&, Seg*, RangePiece*, WindowTail*,
                                       hipStream_t);
template hipError_t launch_window_gather(const WindowStream&, const WindowCall&, const RangePiece*,
                                         const WindowTail*, const int64_t*, int64_t*, hipStream_t, const CvtArgs*);
template hipError_t launch_window_gather(const WindowSet&, const WindowCall&, const RangePiece*,
                                         const WindowTail*, const int64_t*, int64_t*, hipStream_t, const CvtArgs*);

hipError_t launch_stream_set_status(StreamSetRec* recs, const int64_t* idx_err, int64_t* status, int count,
                                    hipStream_t s) {
    if (count <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_stream_set_status, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, s, recs,
                       idx_err, status, count);
    return hipGetLastError();
}

hipError_t launch_window_reduce(const int64_t* wstat, const WindowTail* wt, int K, const int64_t* idx_err,
                                int64_t total, int64_t* result, hipStream_t s, const int64_t* dtotal) {
    ProfScope prof("k_window_reduce", s);
    hipLaunchKernelGGL(k_window_reduce, dim3(1), dim3(256), 0, s, wstat, wt, K, idx_err, total, dtotal, result);
    return hipGetLastError();
}

}  // namespace bshuf
