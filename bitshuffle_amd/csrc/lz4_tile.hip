// lz4_tile.hip -- the kernels around the block decode of a tile decode
// (bshuf_decompress_lz4_tiles_dev, bshuf_decompress_lz4_tiles_set_dev; launch.h,
// "tile decode"): K tiles of rows x cols elements whose flat starts -- and, over
// a set of streams, stream indices -- live in device memory.  k_tile_plan turns
// them into the window decode's tables with a GROUP of rows in a window's place
// (tile_plan.h); work list, token scan and block decode are that decode's,
// unchanged; k_tile_gather settles every tile's status and copies the rows of
// the good tiles; k_tile_reduce makes the result.  Plan and gather are
// instantiated once per source (WindowStream, WindowSet).
#include "launch.h"
#include "range_worklist.h"
#include "tile_plan.h"
#include "window_copy.h"

namespace bshuf {

namespace {

BSHUF_WINDOW_FN TileShape shape_of(const TileCall& c) { return TileShape{c.rg, c.G, c.Mg}; }
BSHUF_WINDOW_FN int64_t span_of(const TileCall& c) { return (c.rows - 1) * c.pitch + c.cols; }

// ---- the sources ----------------------------------------------------------
// For the plan: group g of tile i (piece p = i * G + g) and the tile's info;
// returns the stream the group's blocks are read from.
__device__ __forceinline__ const uint8_t* source_plan(const WindowStream& src, const TileCall& c, int64_t,
                                                      int64_t g, int64_t start, WindowPlan& w, TileInfo& info) {
    info.bad = tile_bad(src.size, span_of(c), start) ? 1 : 0;
    info.sidx = 0;
    tile_group(src.size, c.bs, c.E, c.rows, c.cols, c.pitch, shape_of(c), start, g, info.bad != 0, w);
    return src.st.in;
}

// A bad tile gets blocks [0, Mg) of the set's stream `ref` in every group and
// nothing to copy; when the set is not the one the call describes, every tile
// is bad and has no stream at all (sidx -1).
__device__ __forceinline__ const uint8_t* source_plan(const WindowSet& src, const TileCall& c, int64_t p,
                                                      int64_t g, int64_t start, WindowPlan& w, TileInfo& info) {
    const StreamSetHeader h = *src.hdr;
    const bool match = h.magic == kStreamSetMagic && h.count == src.count && h.E == c.E && h.bs == c.bs &&
                       h.nb_max == src.nb_max;
    const int64_t id = src.ids[p / c.G];
    const bool known = match && id >= 0 && id < src.count;
    const bool bad = tile_set_bad(match ? src.count : 0, id, known ? src.recs[id].size : 0, c.bs, span_of(c),
                                  start, c.Mg);
    int32_t s = (int32_t)id;
    if (bad) s = match && h.ref >= 0 && h.ref < src.count ? (int32_t)h.ref : -1;
    w = WindowPlan{};
    w.nfull = c.Mg;
    w.bad = 1;
    if (s >= 0) tile_group(src.recs[s].size, c.bs, c.E, c.rows, c.cols, c.pitch, shape_of(c), start, g, bad, w);
    src.sidx[p] = s;
    info.bad = bad ? 1 : 0;
    info.sidx = bad ? -1 : s;
    return s >= 0 ? src.recs[s].st.in : (const uint8_t*)src.hdr;  // (never read without a stream)
}

// For the gather: a good tile's stream, its element count and its error word.
__device__ __forceinline__ RangeStream source_stream(const WindowStream& src, const TileInfo&, int64_t& size,
                                                     int64_t& err) {
    size = src.size;
    err = 0;
    return src.st;
}

__device__ __forceinline__ RangeStream source_stream(const WindowSet& src, const TileInfo& info, int64_t& size,
                                                     int64_t& err) {
    const StreamSetRec r = src.recs[info.sidx];
    size = r.size;
    err = r.err;
    return r.st;
}

struct Names {
    const char *plan, *gather;
};
constexpr Names names(const WindowStream&) { return {"k_tile_plan", "k_tile_gather"}; }
constexpr Names names(const WindowSet&) { return {"k_tile_set_plan", "k_tile_set_gather"}; }

// ---- the kernels ----------------------------------------------------------
// One thread per (tile, group).
template <class Source>
__global__ __launch_bounds__(256) void k_tile_plan(Source src, TileCall c, Seg* __restrict__ segs,
                                                   RangePiece* __restrict__ pcs, TileInfo* __restrict__ ti) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= (int64_t)c.K * c.G) return;
    const int64_t i = p / c.G, g = p - i * c.G;
    WindowPlan w;
    TileInfo info;
    info.start = c.starts[i];
    const uint8_t* in = source_plan(src, c, p, g, info.start, w, info);
    uint8_t* slot = c.slots + p * c.slot;
    Seg sg;
    sg.in = in;
    sg.out = slot;
    sg.first = p * c.Mg;
    sg.nfull = w.nfull;
    sg.tail = 0;
    sg.in_nbytes = 0;  // the work list: the end of the group's last record
    sg.chunk0 = 0;
    sg.nchunks = 0;
    sg.seq0 = 0;       // the work list
    sg.result = c.res + p;
    sg.last = w.last;
    sg.pad_ = 0;
    segs[p] = sg;
    RangePiece pc;
    pc.b0 = w.b0;
    pc.nblk = c.Mg;
    pc.seq_base = c.seq_words < 0 ? -1 : p * c.seq_words;
    pc.src = slot;  // (rows are cut out of the area by k_tile_gather)
    pc.dst = c.out;
    pc.lo = 0;
    pc.n = 0;
    pc.kind = kPieceEdge;
    pc.pad_ = 0;
    pcs[p] = pc;
    if (g == 0) ti[i] = info;
}

// A workgroup per tile.  Phase 1, the status (launch.h): lanes walk the groups'
// Seg results, and only when one is negative the rows, each looking at the
// statuses of the work blocks [t0, t1) that hold its clip; the highest failing
// block in stream order is reduced through LDS.  Then the verbatim tail, which
// the tile reaches exactly when its last row does.  Phase 2, only for a tile
// without a code: T lanes per row, 256 / T rows at a time, every row by
// span_copy out of its group's staging area and the tail.  Reads stay inside
// the tile's staging areas (16-byte granules of areas that are 16-byte aligned
// and a multiple of 16 long) and its stream, writes inside its slice of out.
// Op: SpanCopy, or SpanCvt for the converting entries (window_copy.h), whose
// rows land where op.place() puts the plain call's.
template <int T, class Source, class Op>
__global__ __launch_bounds__(256) void k_tile_gather(Source src, TileCall c, const RangePiece* __restrict__ pcs,
                                                     const TileInfo* __restrict__ ti,
                                                     const int64_t* __restrict__ dstat,
                                                     int64_t* __restrict__ tstat, Op op) {
    __shared__ unsigned long long worst;  // 1 + the highest failing stream block with a tile element
    __shared__ int64_t worst_code;
    const int64_t i = blockIdx.x;
    const int tid = (int)threadIdx.x;
    const TileInfo info = ti[i];
    const int64_t p0 = i * c.G;
    int64_t code = 0, size = 0;
    RangeStream st{};
    const uint8_t* tsrc = nullptr;
    if (info.bad) {
        code = -71;
    } else {
        int64_t err;
        st = source_stream(src, info, size, err);
        code = err;
    }
    const int64_t covered = tile_covered(size, c.bs);
    if (code == 0) {  // (uniform: of the tile)
        if (tid == 0) worst = 0;
        int neg = 0;
        for (int64_t g = tid; g < c.G; g += 256) neg |= c.res[p0 + g] < 0;
        if (__syncthreads_or(neg)) {
            unsigned long long mine = 0;
            int64_t mine_code = 0;
            for (int64_t r = tid; r < c.rows; r += 256) {
                const int64_t p = p0 + r / c.rg;
                if (c.res[p] >= 0) continue;
                const int64_t b0 = pcs[p].b0;
                TileRow o;
                tile_row(covered, c.bs, c.E, c.cols, c.pitch, c.rg, info.start, r, b0, o);
                for (int64_t j = o.t0; j < o.t1; j++) {
                    const int64_t v = dstat[p * c.Mg + j];
                    if (v < 0 && (unsigned long long)(b0 + j + 1) > mine) {
                        mine = (unsigned long long)(b0 + j + 1);
                        mine_code = v;
                    }
                }
            }
            if (mine) atomicMax(&worst, mine);
            __syncthreads();
            // (work blocks of two groups that are the same block of the stream fail alike)
            if (mine && mine == worst) worst_code = mine_code;
            __syncthreads();
            if (worst) code = worst_code;
        }
        if (code == 0 && info.start + span_of(c) > covered) {
            uint64_t ts;
            if (tail_start(st, ts))
                tsrc = st.in + ts;
            else
                code = -91;
        }
    }
    if (tid == 0) tstat[i] = code ? code : c.rows * c.rbytes;
    if (code) return;
    const int t = tid % T;
    uint8_t* out = c.out + i * c.rows * c.rbytes;
    for (int64_t r = tid / T; r < c.rows; r += 256 / T) {
        const int64_t p = p0 + (c.G == 1 ? 0 : r / c.rg);
        TileRow o;
        tile_row(covered, c.bs, c.E, c.cols, c.pitch, c.rg, info.start, r, pcs[p].b0, o);
        uint8_t* dst = op.place(c.out, out + r * c.rbytes);
        if (o.n > 0) op.span(c.slots + p * c.slot + o.lo, dst, o.n, t, T);
        if (o.tail_n > 0) op.tail(tsrc + o.tail_lo, op.behind(dst, o.n), o.tail_n, t, T);
    }
}

__global__ __launch_bounds__(256) void k_tile_reduce(const int64_t* __restrict__ tstat,
                                                     const TileInfo* __restrict__ ti, int K,
                                                     const int64_t* idx_err, int64_t total, int64_t* result) {
    __shared__ int bad, oob;
    if (threadIdx.x == 0) {
        bad = -1;
        oob = 0;
    }
    __syncthreads();
    int m = -1, o = 0;
    for (int i = threadIdx.x; i < K; i += blockDim.x) {
        if (tstat[i] < 0) m = i;
        o |= ti[i].bad;
    }
    if (m >= 0) atomicMax(&bad, m);
    if (o) atomicOr(&oob, 1);
    __syncthreads();
    if (threadIdx.x == 0)
        *result = (idx_err && *idx_err != 0) ? -91 : (oob ? -71 : (bad >= 0 ? tstat[bad] : total));
}

}  // namespace

template <class Source>
hipError_t launch_tile_plan(const Source& src, const TileCall& c, Seg* segs, RangePiece* pcs, TileInfo* ti,
                            hipStream_t s) {
    ProfScope prof(names(src).plan, s);
    const int64_t n = (int64_t)c.K * c.G;
    hipLaunchKernelGGL(k_tile_plan<Source>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, src, c, segs, pcs,
                       ti);
    return hipGetLastError();
}

template <class Source>
hipError_t launch_tile_gather(const Source& src, const TileCall& c, const RangePiece* pcs, const TileInfo* ti,
                              const int64_t* dstat, int64_t* tstat, hipStream_t s, const CvtArgs* cvt) {
    ProfScope prof(names(src).gather, s);
    // Lanes per row, by the row's bytes: 16 up to 1 KiB (16 rows of a workgroup
    // in flight, up to four 16-byte chunks per lane), a wave up to 2 KiB, else
    // the workgroup (above 1 KiB the window gather's rule).  Measured on 1024
    // tiles of 256 x 256 (profiles/tile_decode, tools/tile_bench.py, the lanes
    // forced by bshuf_set_variant kTileLanes16 / 64 / 256): this kernel takes
    // 0.083 / 0.137 / 0.341 ms with 512-byte rows and 0.128 / 0.156 / 0.430 ms
    // with 1024-byte rows.  Longer rows were not measured.  A converting gather
    // goes by the larger of the row's source and destination bytes
    // (cvt_lane_bytes), the same thresholds: not measured.
    const int v = tuning_variant();
    const int64_t lb = cvt_lane_bytes(cvt, c.rbytes);
    int T = lb <= 1024 ? 16 : lb <= 2048 ? 64 : 256;
    if (v == kTileLanes16) T = 16;
    if (v == kTileLanes64) T = 64;
    if (v == kTileLanes256) T = 256;
    const dim3 grid((unsigned)c.K), block(256);
    auto go = [&](auto op) {
        using Op = decltype(op);
        if (T == 16)
            hipLaunchKernelGGL((k_tile_gather<16, Source, Op>), grid, block, 0, s, src, c, pcs, ti, dstat, tstat,
                               op);
        else if (T == 64)
            hipLaunchKernelGGL((k_tile_gather<64, Source, Op>), grid, block, 0, s, src, c, pcs, ti, dstat, tstat,
                               op);
        else
            hipLaunchKernelGGL((k_tile_gather<256, Source, Op>), grid, block, 0, s, src, c, pcs, ti, dstat, tstat,
                               op);
    };
    if (cvt)
        cvt_dispatch(*cvt, go);
    else
        go(SpanCopy{});
    return hipGetLastError();
}

template hipError_t launch_tile_plan(const WindowStream&, const TileCall&, Seg*, RangePiece*, TileInfo*,
                                     hipStream_t);
template hipError_t launch_tile_plan(const WindowSet&, const TileCall&, Seg*, RangePiece*, TileInfo*, hipStream_t);
template hipError_t launch_tile_gather(const WindowStream&, const TileCall&, const RangePiece*, const TileInfo*,
                                       const int64_t*, int64_t*, hipStream_t, const CvtArgs*);
template hipError_t launch_tile_gather(const WindowSet&, const TileCall&, const RangePiece*, const TileInfo*,
                                       const int64_t*, int64_t*, hipStream_t, const CvtArgs*);

hipError_t launch_tile_reduce(const int64_t* tstat, const TileInfo* ti, int K, const int64_t* idx_err,
                              int64_t total, int64_t* result, hipStream_t s) {
    ProfScope prof("k_tile_reduce", s);
    hipLaunchKernelGGL(k_tile_reduce, dim3(1), dim3(256), 0, s, tstat, ti, K, idx_err, total, result);
    return hipGetLastError();
}

}  // namespace bshuf
