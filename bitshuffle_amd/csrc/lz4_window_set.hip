// lz4_window_set.hip -- the kernels around the block decode of a window decode
// over a set of streams (bshuf_lz4_stream_set_dev,
// bshuf_decompress_lz4_windows_set_dev; launch.h, "window decode over a set of
// streams"): K windows of one length, each in a stream of its own, stream
// indices and starts both in device memory.  k_window_set_plan turns them into
// the tables of the window decode; the work list is k_range_worklist's body
// with a stream per piece; the token scan and the block decode are the batch
// decoder's, unchanged; k_window_set_gather copies every window out of its
// staging area and its stream's verbatim tail; the result is k_window_reduce's.
#include "launch.h"
#include "range_worklist.h"
#include "window_copy.h"
#include "window_plan.h"

namespace bshuf {

namespace {

__global__ __launch_bounds__(256) void k_stream_set_status(StreamSetRec* __restrict__ recs,
                                                           const int64_t* __restrict__ idx_err,
                                                           int64_t* __restrict__ status, int count) {
    const int s = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (s >= count) return;
    const int64_t e = idx_err[s] != 0 ? -91 : 0;
    recs[s].err = e;
    status[s] = e;
}

// One thread per window: its stream, its Seg (Mw consecutive blocks of that
// stream, decoded back to back into staging area i), its piece (the clip of
// that area) and its tail span.  A bad window gets blocks [0, Mw) of the set's
// stream `ref` and nothing to copy; when the set is not the one the call
// describes, every window is bad and has no stream at all (sidx -1).
__global__ __launch_bounds__(256) void k_window_set_plan(WindowSetCall c, Seg* __restrict__ segs,
                                                         RangePiece* __restrict__ pcs,
                                                         WindowTail* __restrict__ wt) {
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= c.K) return;
    const StreamSetHeader h = *c.hdr;
    const bool match = h.magic == kStreamSetMagic && h.count == c.count && h.E == c.E && h.bs == c.bs &&
                       h.nb_max == c.nb_max;
    const int64_t id = c.ids[i];
    const bool known = match && id >= 0 && id < c.count;
    WindowPlan w;
    window_set_plan(match ? c.count : 0, id, known ? c.recs[id].size : 0, c.bs, c.E, c.window, c.starts[i],
                    c.Mw, w);
    int32_t s = (int32_t)id;
    if (w.bad) {
        s = match && h.ref >= 0 && h.ref < c.count ? (int32_t)h.ref : -1;
        if (s >= 0) window_plan_blocks(c.recs[s].size, c.bs, c.E, c.window, 0, c.Mw, true, w);
    }
    c.sidx[i] = s;
    uint8_t* slot = c.slots + (int64_t)i * c.slot;
    Seg g;
    g.in = s >= 0 ? c.recs[s].st.in : (const uint8_t*)c.hdr;  // (never read without a stream)
    g.out = slot;
    g.first = (int64_t)i * c.Mw;
    g.nfull = w.nfull;
    g.tail = 0;
    g.in_nbytes = 0;  // k_window_set_worklist: the end of the window's last record
    g.chunk0 = 0;
    g.nchunks = 0;
    g.seq0 = 0;       // k_window_set_worklist
    g.result = c.res + i;
    g.last = w.last;
    g.pad_ = 0;
    segs[i] = g;
    RangePiece pc;
    pc.b0 = w.b0;
    pc.nblk = c.Mw;
    pc.seq_base = (int64_t)i * c.seq_words;
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

// Workgroups (p, 0 .. gridDim.y) share window p's Mw work blocks.
__global__ __launch_bounds__(256) void k_window_set_worklist(WindowSetCall c, Seg* __restrict__ segs,
                                                             const RangePiece* __restrict__ pcs,
                                                             uint64_t* __restrict__ wl) {
    const int p = blockIdx.x;
    const RangePiece pc = pcs[p];
    const int64_t first = (int64_t)p * c.Mw;
    const int32_t s = c.sidx[p];
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
    const RangeStream st = c.recs[s].st;
    range_worklist_piece(st, segs + p, pc, first, wl);
}

// T lanes per window, 256 / T windows per workgroup (window_copy.h).
template <int T>
__global__ __launch_bounds__(256) void k_window_set_gather(WindowSetCall c, const RangePiece* __restrict__ pcs,
                                                           const WindowTail* __restrict__ wt,
                                                           const int64_t* __restrict__ dstat,
                                                           int64_t* __restrict__ wstat) {
    const int i = (int)(blockIdx.x * (256 / T) + threadIdx.x / T);
    const int t = (int)(threadIdx.x % T);
    if (i >= c.K) return;
    const WindowTail w = wt[i];
    RangeStream st{};
    int64_t err = 0;
    if (!w.bad) {
        const StreamSetRec r = c.recs[c.sidx[i]];
        st = r.st;
        err = r.err;
    }
    window_gather_one(st, err, w, pcs, i, w.t1 > w.t0 ? c.res[i] : 0, dstat + (int64_t)i * c.Mw, c.wbytes,
                      wstat, t, T);
}

}  // namespace

hipError_t launch_stream_set_status(StreamSetRec* recs, const int64_t* idx_err, int64_t* status, int count,
                                    hipStream_t s) {
    if (count <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_stream_set_status, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, s, recs,
                       idx_err, status, count);
    return hipGetLastError();
}

hipError_t launch_window_set_plan(const WindowSetCall& c, Seg* segs, RangePiece* pcs, WindowTail* wt,
                                  hipStream_t s) {
    ProfScope prof("k_window_set_plan", s);
    hipLaunchKernelGGL(k_window_set_plan, dim3((unsigned)((c.K + 255) / 256)), dim3(256), 0, s, c, segs, pcs,
                       wt);
    return hipGetLastError();
}

hipError_t launch_window_set_worklist(const WindowSetCall& c, Seg* segs, const RangePiece* pcs, uint64_t* wl,
                                      hipStream_t s) {
    if (c.K <= 0 || c.Mw <= 0) return hipSuccess;
    // 1024 blocks of a window per workgroup, at most 64 per window (launch_range_worklist)
    const unsigned ny = (unsigned)std::min<int64_t>(64, std::max<int64_t>(1, (c.Mw + 1023) / 1024));
    ProfScope prof("k_window_set_worklist", s);
    hipLaunchKernelGGL(k_window_set_worklist, dim3((unsigned)c.K, ny), dim3(256), 0, s, c, segs, pcs, wl);
    return hipGetLastError();
}

hipError_t launch_window_set_gather(const WindowSetCall& c, const RangePiece* pcs, const WindowTail* wt,
                                    const int64_t* dstat, int64_t* wstat, hipStream_t s) {
    ProfScope prof("k_window_set_gather", s);
    // a wave per window up to 2 KiB, else a workgroup (launch_window_gather)
    if (c.wbytes <= 2048)
        hipLaunchKernelGGL(k_window_set_gather<64>, dim3((unsigned)((c.K + 3) / 4)), dim3(256), 0, s, c, pcs, wt,
                           dstat, wstat);
    else
        hipLaunchKernelGGL(k_window_set_gather<256>, dim3((unsigned)c.K), dim3(256), 0, s, c, pcs, wt, dstat,
                           wstat);
    return hipGetLastError();
}

}  // namespace bshuf
