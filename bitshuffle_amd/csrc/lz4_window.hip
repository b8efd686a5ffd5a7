// lz4_window.hip -- the kernels around the block decode of a window decode
// (bshuf_decompress_lz4_windows_dev; launch.h, "window decode"): K windows of
// one length whose starts live in device memory.  k_window_plan turns the
// starts into the tables the range decode's host plan would have uploaded; the
// work list, the token scan and the block decode are the range decode's and
// the batch decoder's, unchanged; k_window_gather copies every window out of
// its staging area and the verbatim tail, k_window_reduce makes the result.
#include "launch.h"
#include "window_copy.h"
#include "window_plan.h"

namespace bshuf {

namespace {

// One thread per window: its Seg (Mw consecutive blocks of the stream, decoded
// back to back into staging area i), its piece (the clip of that area) and its
// tail span.  An out-of-range start gets block 0 on and nothing to copy.
__global__ __launch_bounds__(256) void k_window_plan(WindowCall c, Seg* __restrict__ segs,
                                                     RangePiece* __restrict__ pcs,
                                                     WindowTail* __restrict__ wt) {
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= c.K) return;
    WindowPlan w;
    window_plan(c.size, c.bs, c.E, c.window, c.starts[i], w);
    uint8_t* slot = c.slots + (int64_t)i * c.slot;
    Seg g;
    g.in = c.in;
    g.out = slot;
    g.first = (int64_t)i * c.Mw;
    g.nfull = w.nfull;
    g.tail = 0;
    g.in_nbytes = 0;  // k_range_worklist: the end of the window's last record
    g.chunk0 = 0;
    g.nchunks = 0;
    g.seq0 = 0;       // k_range_worklist
    g.result = c.res + i;
    g.last = w.last;
    g.pad_ = 0;
    segs[i] = g;
    RangePiece pc;
    pc.b0 = w.b0;
    pc.nblk = c.Mw;
    pc.seq_base = c.seq_words < 0 ? -1 : (int64_t)i * c.seq_words;
    pc.src = slot + w.clip_lo;
    pc.dst = c.out + (int64_t)i * c.wbytes;
    pc.lo = 0;
    pc.n = w.clip_n;
    pc.kind = kPieceEdge;
    pc.pad_ = 0;
    pcs[i] = pc;
    WindowTail t;
    t.lo = w.tail_lo;
    t.n = w.tail_n;
    t.t0 = (int32_t)w.t0;
    t.t1 = (int32_t)w.t1;
    t.bad = w.bad;
    t.pad_ = 0;
    wt[i] = t;
}

// T lanes per window, 256 / T windows per workgroup.  The window's status:
// -71 for a start out of range; else the code of the highest failing block
// among those that hold clip bytes (the Seg's result says whether any of its Mw
// blocks failed); else -91 when the window reaches the verbatim tail and that
// tail is not inside the stream (the rule of k_range_edges); else its byte
// count, and only then is it copied.
template <int T>
__global__ __launch_bounds__(256) void k_window_gather(RangeStream st, WindowCall c,
                                                       const RangePiece* __restrict__ pcs,
                                                       const WindowTail* __restrict__ wt,
                                                       const int64_t* __restrict__ dstat,
                                                       int64_t* __restrict__ wstat) {
    const int i = (int)(blockIdx.x * (256 / T) + threadIdx.x / T);
    const int t = (int)(threadIdx.x % T);
    if (i >= c.K) return;
    const WindowTail w = wt[i];
    window_gather_one(st, 0, w, pcs, i, w.t1 > w.t0 ? c.res[i] : 0, dstat + (int64_t)i * c.Mw, c.wbytes, wstat,
                      t, T);
}

__global__ __launch_bounds__(256) void k_window_reduce(const int64_t* __restrict__ wstat,
                                                       const WindowTail* __restrict__ wt, int K,
                                                       const int64_t* idx_err, int64_t total,
                                                       int64_t* result) {
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
    if (threadIdx.x == 0)
        *result = (idx_err && *idx_err != 0) ? -91 : (oob ? -71 : (bad >= 0 ? wstat[bad] : total));
}

}  // namespace

hipError_t launch_window_plan(const WindowCall& c, Seg* segs, RangePiece* pcs, WindowTail* wt, hipStream_t s) {
    ProfScope prof("k_window_plan", s);
    hipLaunchKernelGGL(k_window_plan, dim3((unsigned)((c.K + 255) / 256)), dim3(256), 0, s, c, segs, pcs, wt);
    return hipGetLastError();
}

hipError_t launch_window_gather(const RangeStream& st, const WindowCall& c, const RangePiece* pcs,
                                const WindowTail* wt, const int64_t* dstat, int64_t* wstat, hipStream_t s) {
    ProfScope prof("k_window_gather", s);
    // a wave per window up to 2 KiB (two 16-byte chunks per lane), else a
    // workgroup: a short window would leave most of a workgroup's four waves
    // with nothing to copy
    if (c.wbytes <= 2048)
        hipLaunchKernelGGL(k_window_gather<64>, dim3((unsigned)((c.K + 3) / 4)), dim3(256), 0, s, st, c, pcs, wt,
                           dstat, wstat);
    else
        hipLaunchKernelGGL(k_window_gather<256>, dim3((unsigned)c.K), dim3(256), 0, s, st, c, pcs, wt, dstat,
                           wstat);
    return hipGetLastError();
}

hipError_t launch_window_reduce(const int64_t* wstat, const WindowTail* wt, int K, const int64_t* idx_err,
                                int64_t total, int64_t* result, hipStream_t s) {
    ProfScope prof("k_window_reduce", s);
    hipLaunchKernelGGL(k_window_reduce, dim3(1), dim3(256), 0, s, wstat, wt, K, idx_err, total, result);
    return hipGetLastError();
}

}  // namespace bshuf
