// lz4_ragged.hip -- the kernels around the block decode of a ragged window
// decode (bshuf_decompress_lz4_ragged_dev, bshuf_decompress_lz4_ragged_set_dev;
// launch.h, "ragged window decode"): K windows whose starts AND lengths -- and,
// over a set of streams, stream indices -- live in device memory, written back
// to back (or at a fixed pitch) into one output.  k_ragged_sums + k_ragged_scan
// place the windows, k_ragged_plan writes the window decode's tables with every
// window's own length, k_ragged_worklist gives the blocks that hold bytes of a
// window their header offsets and all others of its Mw the sentinel; the token
// scan and the block decode are the batch decoder's, unchanged; k_ragged_gather
// copies every window out; the result is k_window_reduce's (lz4_window.hip).
// As there, the kernels are instantiated once per source.
#include "launch.h"
#include "range_worklist.h"
#include "window_copy.h"
#include "window_plan.h"

namespace bshuf {

namespace {

// ---- the sources ----------------------------------------------------------
// Window i's stream: its element count and where it lies.  False: the window
// names no stream (never for one stream; over a set an id outside it, or a set
// that is not the one the call describes) -- it is refused, and `in` is then
// some readable address that nothing is read from.  id: the stream's index.
__device__ __forceinline__ bool ragged_stream(const WindowStream& src, const WindowCall&, int, int64_t& size,
                                              const uint8_t*& in, int32_t& id) {
    size = src.size;
    in = src.st.in;
    id = 0;
    return true;
}

__device__ __forceinline__ bool ragged_stream(const WindowSet& src, const WindowCall& c, int i, int64_t& size,
                                              const uint8_t*& in, int32_t& id) {
    const StreamSetHeader h = *src.hdr;
    const bool match = h.magic == kStreamSetMagic && h.count == src.count && h.E == c.E && h.bs == c.bs &&
                       h.nb_max == src.nb_max;
    const int64_t s = src.ids[i];
    size = 0;
    in = (const uint8_t*)src.hdr;
    id = -1;
    if (!match || s < 0 || s >= src.count) return false;
    size = src.recs[s].size;
    in = src.recs[s].st.in;
    id = (int32_t)s;
    return true;
}

// The elements window i takes in a packed output: its count when it is good.
template <class Source>
__device__ __forceinline__ int64_t ragged_eff(const Source& src, const RaggedCall& c, int64_t i) {
    int64_t size;
    const uint8_t* in;
    int32_t id;
    if (!ragged_stream(src, c.w, (int)i, size, in, id)) return 0;
    const int64_t n = c.counts[i];
    return ragged_good(size, c.w.window, c.w.starts[i], n) ? n : 0;
}

// The plan's note of the window's stream, and the work list's and the gather's
// stream of a window that has one.
__device__ __forceinline__ void note_stream(const WindowStream&, int, int32_t) {}
__device__ __forceinline__ void note_stream(const WindowSet& src, int i, int32_t id) { src.sidx[i] = id; }
__device__ __forceinline__ RangeStream live_stream(const WindowStream& src, int) { return src.st; }
__device__ __forceinline__ RangeStream live_stream(const WindowSet& src, int i) {
    return src.recs[src.sidx[i]].st;
}

struct Names {
    const char *scan, *plan, *worklist, *gather;
};
constexpr Names names(const WindowStream&) {
    return {"k_ragged_scan", "k_ragged_plan", "k_ragged_worklist", "k_ragged_gather"};
}
constexpr Names names(const WindowSet&) {
    return {"k_ragged_set_scan", "k_ragged_set_plan", "k_ragged_set_worklist", "k_ragged_set_gather"};
}

// ---- the placement scan ----------------------------------------------------
// offs[0 .. K] = exclusive scan of ragged_eff, in two small launches over at
// most kRaggedScanTiles tiles, in the manner of the pipelined encode's
// k_seg_sums + k_seg_scan (lz4_encode.hip): the tiles' sums, then every tile
// adds up the sums in front of it and scans its own elements.  One wave per
// tile, 256 windows at a time (four per lane, shuffles across the lanes), no
// LDS, no temporary storage but the tile sums; int64 throughout.
constexpr int kScanPerLane = 4;
constexpr int kScanStep = kWave * kScanPerLane;
constexpr int64_t kScanMinTile = 1024;  // a multiple of kScanStep

__device__ __forceinline__ int64_t shfl_i64(int64_t v, int lane) {
    const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)v, lane, kWave);
    const uint32_t hi = (uint32_t)__shfl((int)(uint32_t)((uint64_t)v >> 32), lane, kWave);
    return (int64_t)(((uint64_t)hi << 32) | lo);
}
__device__ __forceinline__ int64_t shfl_up_i64(int64_t v, int d) {
    const uint32_t lo = (uint32_t)__shfl_up((int)(uint32_t)v, d, kWave);
    const uint32_t hi = (uint32_t)__shfl_up((int)(uint32_t)((uint64_t)v >> 32), d, kWave);
    return (int64_t)(((uint64_t)hi << 32) | lo);
}
__device__ __forceinline__ int64_t wave_sum(int64_t v) {
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, d, kWave);
        const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)((uint64_t)v >> 32), d, kWave);
        v += (int64_t)(((uint64_t)hi << 32) | lo);
    }
    return v;
}

template <class Source>
__global__ __launch_bounds__(kWave) void k_ragged_sums(Source src, RaggedCall c, int64_t* __restrict__ sums,
                                                       int64_t tile) {
    const int64_t K = c.w.K;
    const int64_t t0 = (int64_t)blockIdx.x * tile;
    const int64_t t1 = t0 + tile < K ? t0 + tile : K;
    int64_t v = 0;
    for (int64_t i = t0 + threadIdx.x; i < t1; i += kWave) v += ragged_eff(src, c, i);
    v = wave_sum(v);
    if (threadIdx.x == 0) sums[blockIdx.x] = v;
}

template <class Source>
__global__ __launch_bounds__(kWave) void k_ragged_scan(Source src, RaggedCall c,
                                                       const int64_t* __restrict__ sums, int64_t tile) {
    const int lane = threadIdx.x;
    const int64_t K = c.w.K;
    const int64_t t0 = (int64_t)blockIdx.x * tile;
    const int64_t t1 = t0 + tile < K ? t0 + tile : K;
    int64_t v = 0;
    for (int u = lane; u < (int)blockIdx.x; u += kWave) v += sums[u];
    int64_t base = wave_sum(v);
    for (int64_t at = t0; at < t1; at += kScanStep) {
        const int64_t i0 = at + (int64_t)lane * kScanPerLane;
        int64_t x[kScanPerLane], tot = 0;
#pragma unroll
        for (int k = 0; k < kScanPerLane; k++) {
            x[k] = i0 + k < t1 ? ragged_eff(src, c, i0 + k) : 0;
            tot += x[k];
        }
        int64_t inc = tot;  // inclusive scan of the lanes' totals
#pragma unroll
        for (int d = 1; d < kWave; d <<= 1) {
            const int64_t y = shfl_up_i64(inc, d);
            if (lane >= d) inc += y;
        }
        int64_t o = base + inc - tot;
#pragma unroll
        for (int k = 0; k < kScanPerLane; k++) {
            if (i0 + k < t1) c.offs[i0 + k] = o;
            o += x[k];
        }
        base += shfl_i64(inc, kWave - 1);
    }
    if (t1 == K && lane == 0) c.offs[K] = base;  // the last tile: the call's total
}

// ---- plan, work list, gather -----------------------------------------------
// One thread per window.  A good window whose place in a packed output ends
// behind the output's capacity is refused like one out of range (an empty one
// writes nothing and needs no room).
template <class Source>
__global__ __launch_bounds__(256) void k_ragged_plan(Source src, RaggedCall c, Seg* __restrict__ segs,
                                                     RangePiece* __restrict__ pcs,
                                                     WindowTail* __restrict__ wt) {
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= c.w.K) return;
    int64_t size;
    const uint8_t* in;
    int32_t id;
    const bool known = ragged_stream(src, c.w, i, size, in, id);
    const int64_t n = c.counts[i], start = c.w.starts[i];
    const int64_t at = c.pitch ? (int64_t)i * c.pitch : c.offs[i];
    bool refused = !known;
    if (!refused && ragged_good(size, c.w.window, start, n)) refused = c.pitch == 0 && n > 0 && n > c.capacity - at;
    WindowPlan w;
    ragged_plan(size, c.w.bs, c.w.E, c.w.window, n, start, c.w.Mw, refused, w);
    note_stream(src, i, w.bad ? -1 : id);
    write_window(c.w, i, w, in, c.w.out + at * c.w.E, segs, pcs, wt);
}

// Workgroups (p, 0 .. gridDim.y) share window p's Mw work blocks: the block ->
// window map of all of them, and their offsets.  Work blocks [t0, t1) are the
// live ones, blocks [b0 + t0, b0 + t1) of the window's stream; their records lie
// in [B, end), B the first one's offset and end the offset of the block behind
// the last -- or, for the stream's last block, where its header says its record
// ends -- both forced into the stream as in range_worklist_piece, with the same
// bound on every token position.  The window may read [0, end) of its stream
// (the decoder's in_nbytes) and every offset outside [B, end] is the sentinel,
// as is every work block that is not live: clamp_span (lz4_decode.hip) turns
// that into an empty span at `end`, so the last live block's record ends where
// it should and no record byte of another block is read.  A window without live
// blocks reads an empty stream.
template <class Source>
__global__ __launch_bounds__(256) void k_ragged_worklist(Source src, int64_t Mw, Seg* __restrict__ segs,
                                                         const RangePiece* __restrict__ pcs,
                                                         const WindowTail* __restrict__ wt,
                                                         uint64_t* __restrict__ wl,
                                                         uint32_t* __restrict__ blk_seg) {
    const int p = blockIdx.x;
    const RangePiece pc = pcs[p];
    const WindowTail w = wt[p];
    const int64_t first = (int64_t)p * Mw;
    const int64_t stride = (int64_t)blockDim.x * gridDim.y;
    const int64_t j0 = (int64_t)blockIdx.y * blockDim.x + threadIdx.x;
    RangeStream st{};
    bool live = w.t1 > w.t0 && !w.bad;
    if (live) {
        st = live_stream(src, p);
        live = pc.b0 + w.t1 <= st.nb;  // (what the plan made of the stream's size)
    }
    if (!live) {
        for (int64_t j = j0; j < Mw; j += stride) {
            wl[first + j] = kNoOffset;
            blk_seg[first + j] = (uint32_t)p;
        }
        if (threadIdx.x == 0 && blockIdx.y == 0) {
            segs[p].in_nbytes = 0;
            segs[p].seq0 = pc.seq_base < 0 ? 0 : pc.seq_base;
        }
        return;
    }
    const uint64_t N = (uint64_t)st.in_nbytes;
    uint64_t B = st.offs[pc.b0 + w.t0];
    if (B > N) B = N;
    const uint64_t cap = (uint64_t)(w.t1 - w.t0) * (4 + (uint64_t)st.maxlen);
    const uint64_t lim = N - B < cap ? N : B + cap;
    const int64_t b1 = pc.b0 + w.t1;
    uint64_t end = lim;
    if (b1 < st.nb) {
        end = st.offs[b1];
    } else {
        const uint64_t h = st.offs[st.nb - 1];
        if (h >= B && h <= lim && lim - h >= 4) end = h + 4 + be32_at(st.in + h);
    }
    if (end < B || end > lim) end = lim;
    for (int64_t j = j0; j < Mw; j += stride) {
        uint64_t v = kNoOffset;
        if (j >= w.t0 && j < w.t1) v = st.offs[pc.b0 + j];
        wl[first + j] = (v >= B && v <= end) ? v : kNoOffset;
        blk_seg[first + j] = (uint32_t)p;
    }
    if (threadIdx.x == 0 && blockIdx.y == 0) {
        segs[p].in_nbytes = (int64_t)end;
        segs[p].seq0 = pc.seq_base < 0 ? 0 : pc.seq_base - (int64_t)(B / 3);
    }
}

// T lanes per window, 256 / T windows per workgroup (k_window_gather).
template <int T, class Source, class Op>
__global__ __launch_bounds__(256) void k_ragged_gather(Source src, RaggedCall c,
                                                       const RangePiece* __restrict__ pcs,
                                                       const WindowTail* __restrict__ wt,
                                                       const int64_t* __restrict__ dstat,
                                                       int64_t* __restrict__ wstat, Op op) {
    const int i = (int)(blockIdx.x * (256 / T) + threadIdx.x / T);
    const int t = (int)(threadIdx.x % T);
    if (i >= c.w.K) return;
    const WindowTail w = wt[i];
    int64_t err;
    const RangeStream st = source_stream(src, w, i, err);
    window_gather_one(st, err, w, pcs, i, w.t1 > w.t0 ? c.w.res[i] : 0, dstat + (int64_t)i * c.w.Mw,
                      w.bad ? 0 : c.counts[i] * c.w.E, wstat, t, T, op, c.w.out);
}

}  // namespace

template <class Source>
hipError_t launch_ragged_scan(const Source& src, const RaggedCall& c, int64_t* sums, hipStream_t s) {
    const int64_t K = c.w.K;
    const int64_t per = (K + kRaggedScanTiles - 1) / kRaggedScanTiles;
    const int64_t tile = std::max(kScanMinTile, (per + kScanStep - 1) / kScanStep * kScanStep);
    const unsigned tiles = (unsigned)std::max<int64_t>(1, (K + tile - 1) / tile);
    ProfScope prof(names(src).scan, s);
    if (tiles > 1) {
        hipLaunchKernelGGL(k_ragged_sums<Source>, dim3(tiles), dim3(kWave), 0, s, src, c, sums, tile);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(k_ragged_scan<Source>, dim3(tiles), dim3(kWave), 0, s, src, c, sums, tile);
    return hipGetLastError();
}

template <class Source>
hipError_t launch_ragged_plan(const Source& src, const RaggedCall& c, Seg* segs, RangePiece* pcs,
                              WindowTail* wt, hipStream_t s) {
    ProfScope prof(names(src).plan, s);
    hipLaunchKernelGGL(k_ragged_plan<Source>, dim3((unsigned)((c.w.K + 255) / 256)), dim3(256), 0, s, src, c,
                       segs, pcs, wt);
    return hipGetLastError();
}

template <class Source>
hipError_t launch_ragged_worklist(const Source& src, const RaggedCall& c, Seg* segs, const RangePiece* pcs,
                                  const WindowTail* wt, uint64_t* wl, uint32_t* blk_seg, hipStream_t s) {
    if (c.w.K <= 0 || c.w.Mw <= 0) return hipSuccess;
    // 1024 blocks of a window per workgroup, at most 64 per window (launch_range_worklist)
    const unsigned ny = (unsigned)std::min<int64_t>(64, std::max<int64_t>(1, (c.w.Mw + 1023) / 1024));
    ProfScope prof(names(src).worklist, s);
    hipLaunchKernelGGL(k_ragged_worklist<Source>, dim3((unsigned)c.w.K, ny), dim3(256), 0, s, src, c.w.Mw, segs,
                       pcs, wt, wl, blk_seg);
    return hipGetLastError();
}

template <class Source>
hipError_t launch_ragged_gather(const Source& src, const RaggedCall& c, const RangePiece* pcs,
                                const WindowTail* wt, const int64_t* dstat, int64_t* wstat, hipStream_t s,
                                const CvtArgs* cvt) {
    ProfScope prof(names(src).gather, s);
    // by the longest window a call may hold (launch_window_gather, also for a
    // converting gather: not measured)
    const bool wave = cvt_lane_bytes(cvt, c.w.wbytes) <= 2048;
    auto go = [&](auto op) {
        using Op = decltype(op);
        if (wave)
            hipLaunchKernelGGL((k_ragged_gather<64, Source, Op>), dim3((unsigned)((c.w.K + 3) / 4)), dim3(256), 0,
                               s, src, c, pcs, wt, dstat, wstat, op);
        else
            hipLaunchKernelGGL((k_ragged_gather<256, Source, Op>), dim3((unsigned)c.w.K), dim3(256), 0, s, src, c,
                               pcs, wt, dstat, wstat, op);
    };
    if (cvt)
        cvt_dispatch(*cvt, go);
    else
        go(SpanCopy{});
    return hipGetLastError();
}

#define BSHUF_RAGGED_INST(Source)                                                                              \
    template hipError_t launch_ragged_scan(const Source&, const RaggedCall&, int64_t*, hipStream_t);           \
    template hipError_t launch_ragged_plan(const Source&, const RaggedCall&, Seg*, RangePiece*, WindowTail*,   \
                                           hipStream_t);                                                       \
    template hipError_t launch_ragged_worklist(const Source&, const RaggedCall&, Seg*, const RangePiece*,      \
                                               const WindowTail*, uint64_t*, uint32_t*, hipStream_t);          \
    template hipError_t launch_ragged_gather(const Source&, const RaggedCall&, const RangePiece*,              \
                                             const WindowTail*, const int64_t*, int64_t*, hipStream_t,     \
                                             const CvtArgs*);
BSHUF_RAGGED_INST(WindowStream)
BSHUF_RAGGED_INST(WindowSet)
#undef BSHUF_RAGGED_INST

}  // namespace bshuf
