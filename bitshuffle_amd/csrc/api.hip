// api.hip -- the device-resident C-ABI (include/bitshuffle.h,
// include/bitshuffle_core.h): default block size, compress bound, the *_dev
// and *_batch_dev entry points (device pointers, enqueue only).  The
// host-pointer drop-in entry points live in host.hip.  There is no CPU compute
// path: without a usable HIP device every entry point returns -70.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <mutex>
#include <vector>

#include "../../include/bitshuffle.h"
#include "launch.h"
#include "plan.h"
#include "range_plan.h"
#include "tile_plan.h"
#include "window_plan.h"

using namespace bshuf;

namespace {

inline size_t al256(size_t x) { return (x + 255) & ~(size_t)255; }

struct Carver {
    uint8_t* base;
    size_t off = 0;
    template <class T>
    T* take(size_t bytes) {
        T* p = reinterpret_cast<T*>(base ? base + off : nullptr);
        off += al256(bytes);
        return p;
    }
};

// ---- workspace layouts -------------------------------------------------------
size_t enc_ws(const Plan& p, EncodeBufs* b, uint8_t* base) {
    Carver c{base};
    const int64_t slot = encode_slot_bytes(p.L);
    EncodeBufs x;
    x.slot = slot;
    x.scratch = c.take<uint8_t>((size_t)(p.nb * slot));
    x.foot = c.take<uint64_t>((size_t)(p.nb + 1) * 8 + kEncTicketSets * kTicketSetBytes);
    x.offs = c.take<uint64_t>((size_t)(p.nb + 1) * 8);
    x.scan_tmp_bytes = encode_scan_tmp_bytes(p.nb);
    x.scan_tmp = c.take<void>(x.scan_tmp_bytes);
    if ((int64_t)p.L.bs * p.L.E > max_lds_encode_bytes()) {
        // large blocks: bit-transposed copy (+ over-read pad) and LZ4 tables
        x.shuf = c.take<uint8_t>((size_t)(p.L.nfull * (int64_t)p.L.bs + p.L.last) * p.L.E + 64);
        x.tables = c.take<uint32_t>((size_t)p.nb * kLargeTableWords * 4);
    }
    if (b) *b = x;
    return c.off;
}

size_t dec_ws(const Plan& p, int64_t blocks_end, int64_t in_nbytes, bool need_index, DecodeBufs* b,
              uint8_t* base) {
    Carver c{base};
    DecodeBufs x;
    x.chunk = index_chunk_bytes(p.L);
    x.nchunks = blocks_end > 0 ? (blocks_end + x.chunk - 1) / x.chunk : 0;
    x.offs = c.take<uint64_t>((size_t)p.nb * 8 + 8);
    x.status = c.take<int64_t>((size_t)p.nb * 8 + 8);
    // one u32 per 3 stream bytes (a sequence takes >= 3), + a 64-lane prefetch
    x.seq = c.take<uint32_t>(((size_t)in_nbytes / 3 + 80) * 4);
    x.exits = c.take<int64_t>((size_t)x.nchunks * 8 + 8);
    x.cnt = c.take<uint64_t>((size_t)(x.nchunks + 1) * 8);
    x.base = c.take<uint64_t>((size_t)(x.nchunks + 1) * 8);
    x.idx_err = c.take<int64_t>(8);
    x.bad = c.take<long long>(8);
    x.tickets = c.take<uint32_t>(kTicketSetBytes);
    x.scan_tmp_bytes = need_index ? decode_scan_tmp_bytes(x.nchunks) : 0;
    x.scan_tmp = c.take<void>(x.scan_tmp_bytes + 8);
    if ((int64_t)p.L.bs * p.L.E > max_lds_decode_bytes())
        x.shuf = c.take<uint8_t>((size_t)(p.L.nfull * (int64_t)p.L.bs + p.L.last) * p.L.E + 64);
    if (b) *b = x;
    return c.off;
}

// Workspace of a *_dev call made with ws == NULL: stream-ordered allocation,
// freed stream-ordered when the call returns -- from the library's OWN memory
// pool, whose release threshold keeps freed memory mapped for reuse.  The
// device's default pool (release threshold 0) hands freed blocks back to the
// OS at synchronisation points and maps memory again at the next allocation;
// kernels working in such re-mapped workspaces produced wrong results early in
// a process (round-2 host-path defect, DESIGN.md §4.2: 16 of 40 fresh HDF5
// regression processes with the default pool, 0 of 40 with a pool that never
// trims).  In the diagnostic build only, BSHUF_DIAG_POOL=default brings the
// default pool back for that experiment (tools/h5_repro.sh).  This is a WORKAROUND for re-mapping
// behaviour whose mechanism is not understood, not a proven
// root cause.  What the pool keeps is capped at the largest single workspace
// requested so far (pool_keep): one call's worth stays mapped, not every
// concurrent call's.
std::atomic<uint64_t> g_pool_keep{0};
bool g_pool_is_default = false;  // BSHUF_DIAG_POOL=default: leave its threshold alone
void pool_keep(hipMemPool_t pool, size_t n) {
    if (g_pool_is_default) return;
    uint64_t cur = g_pool_keep.load(std::memory_order_relaxed);
    while (cur < n && !g_pool_keep.compare_exchange_weak(cur, (uint64_t)n, std::memory_order_relaxed)) {
    }
    if (cur < n) {
        uint64_t keep = g_pool_keep.load(std::memory_order_relaxed);
        (void)hipMemPoolSetAttribute(pool, hipMemPoolAttrReleaseThreshold, &keep);
    }
}
hipMemPool_t workspace_pool() {
    static hipMemPool_t pool = nullptr;
    static bool tried = false;
    static std::mutex mu;
    std::lock_guard<std::mutex> g(mu);
    if (tried) return pool;
    tried = true;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return nullptr;
#ifdef BSHUF_DIAG
    const char* e = getenv("BSHUF_DIAG_POOL");
#else
    const char* e = nullptr;
#endif
    if (e && !strcmp(e, "default")) {
        (void)hipDeviceGetDefaultMemPool(&pool, dev);
        g_pool_is_default = true;
        return pool;
    }
    hipMemPoolProps props = {};
    props.allocType = hipMemAllocationTypePinned;
    props.handleTypes = hipMemHandleTypeNone;
    props.location.type = hipMemLocationTypeDevice;
    props.location.id = dev;
    if (hipMemPoolCreate(&pool, &props) != hipSuccess) {
        pool = nullptr;
        return nullptr;
    }
    return pool;
}

struct DevBuf {
    void* p = nullptr;
    hipStream_t s = nullptr;
    hipError_t alloc(size_t n, hipStream_t st) {
        s = st;
        hipMemPool_t pool = workspace_pool();
        if (!pool) return hipErrorOutOfMemory;
        pool_keep(pool, n ? n : 1);
        return hipMallocFromPoolAsync(&p, n ? n : 1, pool, st);
    }
    ~DevBuf() {
        if (p) (void)hipFreeAsync(p, s);
    }
};

}  // namespace

extern "C" {

int bshuf_using_SSE2(void) { return 0; }
int bshuf_using_NEON(void) { return 0; }
int bshuf_using_AVX2(void) { return 0; }
int bshuf_using_AVX512(void) { return 0; }
int bshuf_using_HIP(void) { return have_device() ? 1 : 0; }

// src/bitshuffle_core.c:2038-2046 -- format-stable, never change.
size_t bshuf_default_block_size(const size_t elem_size) {
    size_t bs = 8192 / elem_size;
    bs = (bs / kBlockedMult) * kBlockedMult;
    return bs > 128 ? bs : 128;
}

// src/bitshuffle.c:214-233, including its (size_t)-81 quirk.
size_t bshuf_compress_lz4_bound(const size_t size, const size_t elem_size, size_t block_size) {
    if (block_size == 0) block_size = bshuf_default_block_size(elem_size);
    if (block_size % kBlockedMult) return (size_t)-81;
    size_t bound = ((size_t)lz4_bound((int)(block_size * elem_size)) + 4) * (size / block_size);
    size_t leftover = ((size % block_size) / kBlockedMult) * kBlockedMult;
    if (leftover) bound += (size_t)lz4_bound((int)(leftover * elem_size)) + 4;
    bound += (size % kBlockedMult) * elem_size;
    return bound;
}

size_t bshuf_lz4_dev_nblocks(size_t size, size_t elem_size, size_t block_size) {
    Plan p;
    return make_plan(size, elem_size, block_size, p) == 0 ? (size_t)p.nb : 0;
}

// ---------------------------------------------------------------------------
// device-resident entry points
// ---------------------------------------------------------------------------

static int64_t transpose_dev(const void* in, void* out, size_t size, size_t elem_size,
                             size_t block_size, void* stream, bool fwd) {
    Plan p;
    const int64_t r = make_plan(size, elem_size, block_size, p);
    if (r) return r;
    if (!have_device()) return kErrHip;
    hipStream_t s = (hipStream_t)stream;
    const uint8_t* i8 = (const uint8_t*)in;
    uint8_t* o8 = (uint8_t*)out;
    if (launch_transpose(i8, o8, p.L, fwd, s) != hipSuccess) return kErrHip;
    if (p.tail) {
        const int64_t off = (p.L.nfull * (int64_t)p.L.bs + p.L.last) * p.L.E;
        if (hipMemcpyAsync(o8 + off, i8 + off, (size_t)p.tail, hipMemcpyDeviceToDevice, s) !=
            hipSuccess)
            return kErrHip;
    }
    return (int64_t)(size * elem_size);
}

int64_t bshuf_bitshuffle_dev(const void* in, void* out, size_t size, size_t elem_size,
                             size_t block_size, void* stream) {
    return transpose_dev(in, out, size, elem_size, block_size, stream, true);
}

int64_t bshuf_bitunshuffle_dev(const void* in, void* out, size_t size, size_t elem_size,
                               size_t block_size, void* stream) {
    return transpose_dev(in, out, size, elem_size, block_size, stream, false);
}

size_t bshuf_compress_lz4_dev_workspace(size_t size, size_t elem_size, size_t block_size) {
    Plan p;
    if (make_plan(size, elem_size, block_size, p)) return 0;
    return enc_ws(p, nullptr, nullptr);
}

static int64_t compress_dev(const void* in, void* out, size_t size, size_t elem_size,
                            size_t block_size, void* ws, size_t ws_bytes, int64_t* d_result,
                            uint64_t* block_offsets, void* stream, bool fast) {
    Plan p;
    const int64_t r = make_plan(size, elem_size, block_size, p);
    if (r) return r;
    if (!have_device()) return kErrHip;
    hipStream_t s = (hipStream_t)stream;
    const size_t need = enc_ws(p, nullptr, nullptr);
    DevBuf own;
    if (!ws) {
        if (own.alloc(need, s) != hipSuccess) return -1;
        ws = own.p;
    } else if (ws_bytes < need || ((uintptr_t)ws & 255)) {
        return kErrUnsupported;
    }
    EncodeBufs b;
    enc_ws(p, &b, (uint8_t*)ws);
    if (launch_encode((const uint8_t*)in, (uint8_t*)out, p.L, p.tail, b, d_result, s, fast) !=
        hipSuccess)
        return kErrHip;
    if (block_offsets && p.nb &&
        hipMemcpyAsync(block_offsets, b.offs, (size_t)p.nb * 8, hipMemcpyDeviceToDevice, s) !=
            hipSuccess)
        return kErrHip;
    return 0;
}

int64_t bshuf_compress_lz4_dev(const void* in, void* out, size_t size, size_t elem_size,
                               size_t block_size, void* ws, size_t ws_bytes, int64_t* d_result,
                               uint64_t* block_offsets, void* stream) {
    return compress_dev(in, out, size, elem_size, block_size, ws, ws_bytes, d_result, block_offsets,
                        stream, false);
}

// Fast parse v1 (lz4_fast.hip): same framing, workspace and error codes; blocks
// above 65536 bytes take the exact parse, so such a stream is the exact one.
int bshuf_lz4_fast_version(void) { return 1; }

int64_t bshuf_compress_lz4_fast_dev(const void* in, void* out, size_t size, size_t elem_size,
                                    size_t block_size, void* ws, size_t ws_bytes, int64_t* d_result,
                                    uint64_t* block_offsets, void* stream) {
    return compress_dev(in, out, size, elem_size, block_size, ws, ws_bytes, d_result, block_offsets,
                        stream, true);
}

size_t bshuf_decompress_lz4_dev_workspace(size_t in_nbytes, size_t size, size_t elem_size,
                                          size_t block_size) {
    Plan p;
    if (make_plan(size, elem_size, block_size, p)) return 0;
    const int64_t cb = (int64_t)in_nbytes - p.tail;
    return dec_ws(p, cb > 0 ? cb : 0, (int64_t)in_nbytes, true, nullptr, nullptr);
}

// in_nbytes: the stream's readable bytes -- or, with dlen, the capacity of
// `in`, the length itself being read by the kernels from *dlen
static int64_t decompress_dev(const void* in, size_t in_nbytes, const int64_t* dlen, void* out,
                              size_t size, size_t elem_size, size_t block_size, void* ws,
                              size_t ws_bytes, int64_t* d_result, const uint64_t* block_offsets,
                              void* stream) {
    Plan p;
    const int64_t r = make_plan(size, elem_size, block_size, p);
    if (r) return r;
    if (!have_device()) return kErrHip;
    hipStream_t s = (hipStream_t)stream;
    int64_t cb = (int64_t)in_nbytes - p.tail;
    if (cb < 0) cb = 0;
    const bool need_index = block_offsets == nullptr;
    const size_t need = dec_ws(p, cb, (int64_t)in_nbytes, need_index, nullptr, nullptr);
    DevBuf own;
    if (!ws) {
        if (own.alloc(need, s) != hipSuccess) return -1;
        ws = own.p;
    } else if (ws_bytes < need || ((uintptr_t)ws & 255)) {
        return kErrUnsupported;
    }
    DecodeBufs b;
    dec_ws(p, cb, (int64_t)in_nbytes, need_index, &b, (uint8_t*)ws);
    const uint8_t* i8 = (const uint8_t*)in;
    if (need_index) {
        if (launch_index(i8, cb, p.L, b, s, dlen, (int64_t)in_nbytes, p.tail) != hipSuccess)
            return kErrHip;
    } else {
        b.offs = const_cast<uint64_t*>(block_offsets);
        b.idx_err = nullptr;
    }
    if (launch_decode(i8, (int64_t)in_nbytes, (uint8_t*)out, p.L, p.tail, b, d_result, s, dlen) !=
        hipSuccess)
        return kErrHip;
    return 0;
}

int64_t bshuf_decompress_lz4_dev(const void* in, size_t in_nbytes, void* out, size_t size,
                                 size_t elem_size, size_t block_size, void* ws, size_t ws_bytes,
                                 int64_t* d_result, const uint64_t* block_offsets,
                                 void* stream) {
    return decompress_dev(in, in_nbytes, nullptr, out, size, elem_size, block_size, ws, ws_bytes,
                          d_result, block_offsets, stream);
}

int64_t bshuf_decompress_lz4_dev_dlen(const void* in, const int64_t* d_in_nbytes, size_t in_capacity,
                                      void* out, size_t size, size_t elem_size, size_t block_size,
                                      void* ws, size_t ws_bytes, int64_t* d_result,
                                      const uint64_t* block_offsets, void* stream) {
    if (!d_in_nbytes) return kErrUnsupported;
    return decompress_dev(in, in_capacity, d_in_nbytes, out, size, elem_size, block_size, ws,
                          ws_bytes, d_result, block_offsets, stream);
}

// The block index of a framed stream alone (K6, the decoder's parallel
// header walk): block k's byte offset in `in`, for callers that split one
// stream's decode across devices (bitshuffle_amd/split.py).  *d_status: 0 when
// the records tile the stream exactly, else the index's error word (the
// decoder would return -91); a block the walk could not place holds ~0.
// Replaces the reference's serial header walk (src/iochain.c:42-64 inside
// bshuf_blocked_wrap_fun, src/bitshuffle_core.c:1877-1931) when run alone.
int64_t bshuf_lz4_block_index_dev(const void* in, size_t in_nbytes, size_t size, size_t elem_size,
                                  size_t block_size, void* ws, size_t ws_bytes,
                                  uint64_t* block_offsets, int64_t* d_status, void* stream) {
    Plan p;
    const int64_t r = make_plan(size, elem_size, block_size, p);
    if (r) return r;
    if (!block_offsets || !d_status) return kErrUnsupported;
    if (!have_device()) return kErrHip;
    hipStream_t s = (hipStream_t)stream;
    int64_t cb = (int64_t)in_nbytes - p.tail;
    if (cb < 0) cb = 0;
    const size_t need = dec_ws(p, cb, (int64_t)in_nbytes, true, nullptr, nullptr);
    DevBuf own;
    if (!ws) {
        if (own.alloc(need, s) != hipSuccess) return -1;
        ws = own.p;
    } else if (ws_bytes < need || ((uintptr_t)ws & 255)) {
        return kErrUnsupported;
    }
    DecodeBufs b;
    dec_ws(p, cb, (int64_t)in_nbytes, true, &b, (uint8_t*)ws);
    if (launch_index((const uint8_t*)in, cb, p.L, b, s, nullptr, (int64_t)in_nbytes, p.tail) !=
        hipSuccess)
        return kErrHip;
    if (p.nb && hipMemcpyAsync(block_offsets, b.offs, (size_t)p.nb * 8, hipMemcpyDeviceToDevice, s) !=
                    hipSuccess)
        return kErrHip;
    if (hipMemcpyAsync(d_status, b.idx_err, 8, hipMemcpyDeviceToDevice, s) != hipSuccess)
        return kErrHip;
    return 0;
}

// ---------------------------------------------------------------------------
// batched device entry points: `count` independent streams per launch
// ---------------------------------------------------------------------------

namespace {

struct BatchPlan {
    std::vector<Seg> segs;
    Layout L;        // shared bs, E; L.nfull = total blocks
    int64_t nb = 0;  // total blocks
    int64_t nchunks = 0;
    int64_t seq_words = 0;
    int64_t chunk = 0;
};

// Segment table of a batch (src/bitshuffle_core.c:1877-1931 blocking per
// stream); in_nbytes == nullptr for the encoder.
int64_t make_batch(const void* const* in, void* const* out, const size_t* sizes,
                   const size_t* in_nbytes, size_t count, size_t elem_size, size_t block_size,
                   BatchPlan& bp) {
    if (count == 0 || count > (size_t)INT32_MAX) return kErrUnsupported;
    bp.segs.resize(count);
    for (size_t i = 0; i < count; i++) {
        Plan p;
        const int64_t r = make_plan(sizes[i], elem_size, block_size, p);
        if (r) return r;
        if (i == 0) {
            bp.L = p.L;
            bp.chunk = index_chunk_bytes(p.L);
        }
        Seg& g = bp.segs[i];
        g.in = in ? (const uint8_t*)in[i] : nullptr;
        g.out = out ? (uint8_t*)out[i] : nullptr;
        g.first = bp.nb;
        g.nfull = p.L.nfull;
        g.last = p.L.last;
        g.pad_ = 0;
        g.tail = p.tail;
        g.in_nbytes = in_nbytes ? (int64_t)in_nbytes[i] : 0;
        const int64_t cb = std::max<int64_t>(g.in_nbytes - g.tail, 0);
        g.chunk0 = bp.nchunks;
        g.nchunks = cb > 0 ? (cb + bp.chunk - 1) / bp.chunk : 0;
        g.seq0 = bp.seq_words;
        g.result = nullptr;
        bp.nb += p.nb;
        bp.nchunks += g.nchunks;
        bp.seq_words += g.in_nbytes / 3 + 80;
    }
    bp.L.nfull = bp.nb;
    bp.L.last = 0;
    return 0;
}

size_t enc_batch_ws(const BatchPlan& bp, EncodeBufs* b, Seg** dsegs, uint32_t** blk_seg,
                    uint8_t* base) {
    Carver c{base};
    Seg* sg = c.take<Seg>(bp.segs.size() * sizeof(Seg));
    uint32_t* bm = c.take<uint32_t>((size_t)bp.nb * 4 + 4);
    EncodeBufs x;
    x.slot = encode_slot_bytes(bp.L);
    x.scratch = c.take<uint8_t>((size_t)(bp.nb * x.slot));
    x.foot = c.take<uint64_t>((size_t)(bp.nb + 1) * 8 + kEncTicketSets * kTicketSetBytes);
    x.offs = c.take<uint64_t>((size_t)(bp.nb + 1) * 8);
    x.scan_tmp_bytes = encode_scan_tmp_bytes(bp.nb);
    x.scan_tmp = c.take<void>(x.scan_tmp_bytes);
    if (b) *b = x;
    if (dsegs) *dsegs = sg;
    if (blk_seg) *blk_seg = bm;
    return c.off;
}

size_t dec_batch_ws(const BatchPlan& bp, DecodeBufs* b, Seg** dsegs, uint32_t** blk_seg,
                    uint32_t** chunk_seg, uint8_t* base) {
    Carver c{base};
    const size_t ns = bp.segs.size();
    Seg* sg = c.take<Seg>(ns * sizeof(Seg));
    uint32_t* bm = c.take<uint32_t>((size_t)bp.nb * 4 + 4);
    uint32_t* cm = c.take<uint32_t>((size_t)bp.nchunks * 4 + 4);
    DecodeBufs x;
    x.chunk = bp.chunk;
    x.nchunks = bp.nchunks;
    x.offs = c.take<uint64_t>((size_t)bp.nb * 8 + 8);
    x.status = c.take<int64_t>((size_t)bp.nb * 8 + 8);
    x.seq = c.take<uint32_t>((size_t)bp.seq_words * 4);
    x.exits = c.take<int64_t>((size_t)bp.nchunks * 8 + 8);
    x.cnt = c.take<uint64_t>((size_t)(bp.nchunks + 1) * 8);
    x.base = c.take<uint64_t>((size_t)(bp.nchunks + 1) * 8);
    x.idx_err = c.take<int64_t>(ns * 8);
    x.bad = c.take<long long>(ns * 8);
    x.tickets = c.take<uint32_t>(kTicketSetBytes);
    x.scan_tmp_bytes = decode_scan_tmp_bytes(bp.nchunks);
    x.scan_tmp = c.take<void>(x.scan_tmp_bytes + 8);
    if (b) *b = x;
    if (dsegs) *dsegs = sg;
    if (blk_seg) *blk_seg = bm;
    if (chunk_seg) *chunk_seg = cm;
    return c.off;
}

// Caller workspace, or a stream-ordered allocation owned by `own`.
int64_t get_ws(void*& ws, size_t ws_bytes, size_t need, DevBuf& own, hipStream_t s) {
    if (!ws) {
        if (own.alloc(need, s) != hipSuccess) return -1;
        ws = own.p;
    } else if (ws_bytes < need || ((uintptr_t)ws & 255)) {
        return kErrUnsupported;
    }
    return 0;
}

}  // namespace

// Batches encoded one stream at a time: blocks above the LDS encoder's size,
// or blocks of both LZ4 table types in one batch (a byU32-size block_size
// with a byU16-size partial block).
static bool enc_batch_per_stream(const BatchPlan& bp) {
    const bool wide = (int64_t)bp.L.bs * bp.L.E >= kU16TableLimit;
    bool mixed = (int64_t)bp.L.bs * bp.L.E > max_lds_encode_bytes();
    for (const Seg& g : bp.segs) mixed = mixed || (g.last && ((int64_t)g.last * bp.L.E >= kU16TableLimit) != wide);
    return mixed;
}

// ... their workspace: the largest single stream's (the streams follow each
// other on the stream and take the workspace in turn).
static size_t enc_per_stream_ws(const size_t* sizes, size_t count, size_t elem_size, size_t block_size) {
    size_t need = 0;
    for (size_t i = 0; i < count; i++) {
        Plan p;
        if (make_plan(sizes[i], elem_size, block_size, p)) return 0;
        need = std::max(need, enc_ws(p, nullptr, nullptr));
    }
    return need;
}

size_t bshuf_compress_lz4_batch_dev_workspace(const size_t* sizes, size_t count, size_t elem_size,
                                              size_t block_size) {
    BatchPlan bp;
    if (make_batch(nullptr, nullptr, sizes, nullptr, count, elem_size, block_size, bp)) return 0;
    if (enc_batch_per_stream(bp)) return enc_per_stream_ws(sizes, count, elem_size, block_size);
    return enc_batch_ws(bp, nullptr, nullptr, nullptr, nullptr);
}

static int64_t compress_batch(const void* const* in, void* const* out, const size_t* sizes,
                              size_t count, size_t elem_size, size_t block_size, void* ws,
                              size_t ws_bytes, int64_t* d_results, uint64_t* block_offsets,
                              void* stream, bool fast) {
    BatchPlan bp;
    const int64_t r = make_batch(in, out, sizes, nullptr, count, elem_size, block_size, bp);
    if (r) return r;
    if (!have_device()) return kErrHip;
    hipStream_t s = (hipStream_t)stream;
    for (size_t i = 0; i < count; i++) bp.segs[i].result = d_results + i;
    if (enc_batch_per_stream(bp)) {
        // one stream at a time, each in the caller's workspace when there is one
        if (ws && (ws_bytes < enc_per_stream_ws(sizes, count, elem_size, block_size) || ((uintptr_t)ws & 255)))
            return kErrUnsupported;
        for (size_t i = 0; i < count; i++) {
            const int64_t e = compress_dev(in[i], out[i], sizes[i], elem_size, block_size, ws, ws ? ws_bytes : 0,
                                           d_results + i,
                                           block_offsets ? block_offsets + bp.segs[i].first : nullptr,
                                           stream, fast);
            if (e) return e;
        }
        return 0;
    }
    DevBuf own;
    const size_t need = enc_batch_ws(bp, nullptr, nullptr, nullptr, nullptr);
    const int64_t w = get_ws(ws, ws_bytes, need, own, s);
    if (w) return w;
    EncodeBufs b;
    Seg* dsegs = nullptr;
    uint32_t* blk_seg = nullptr;
    enc_batch_ws(bp, &b, &dsegs, &blk_seg, (uint8_t*)ws);
    if (stage_upload(bp.segs.data(), count * sizeof(Seg), dsegs, s) != hipSuccess ||
        launch_seg_map(dsegs, (int)count, blk_seg, false, s) != hipSuccess ||
        launch_encode_batch(dsegs, bp.segs.data(), (int)count, blk_seg, bp.L, b, block_offsets, s,
                            fast) != hipSuccess)
        return kErrHip;
    return 0;
}

int64_t bshuf_compress_lz4_batch_dev(const void* const* in, void* const* out, const size_t* sizes,
                                     size_t count, size_t elem_size, size_t block_size, void* ws,
                                     size_t ws_bytes, int64_t* d_results, uint64_t* block_offsets,
                                     void* stream) {
    return compress_batch(in, out, sizes, count, elem_size, block_size, ws, ws_bytes, d_results,
                          block_offsets, stream, false);
}

int64_t bshuf_compress_lz4_fast_batch_dev(const void* const* in, void* const* out, const size_t* sizes,
                                          size_t count, size_t elem_size, size_t block_size, void* ws,
                                          size_t ws_bytes, int64_t* d_results, uint64_t* block_offsets,
                                          void* stream) {
    return compress_batch(in, out, sizes, count, elem_size, block_size, ws, ws_bytes, d_results,
                          block_offsets, stream, true);
}

// Blocks above the LDS decoder's size are decoded one stream at a time, in a
// workspace of the largest single stream's size (as the encoder's, above).
static size_t dec_per_stream_ws(const size_t* in_nbytes, const size_t* sizes, size_t count, size_t elem_size,
                                size_t block_size) {
    size_t need = 0;
    for (size_t i = 0; i < count; i++)
        need = std::max(need, bshuf_decompress_lz4_dev_workspace(in_nbytes[i], sizes[i], elem_size, block_size));
    return need;
}

size_t bshuf_decompress_lz4_batch_dev_workspace(const size_t* in_nbytes, const size_t* sizes,
                                                size_t count, size_t elem_size, size_t block_size) {
    BatchPlan bp;
    if (make_batch(nullptr, nullptr, sizes, in_nbytes, count, elem_size, block_size, bp)) return 0;
    if ((int64_t)bp.L.bs * bp.L.E > max_lds_decode_bytes())
        return dec_per_stream_ws(in_nbytes, sizes, count, elem_size, block_size);
    return dec_batch_ws(bp, nullptr, nullptr, nullptr, nullptr, nullptr);
}

// in_nbytes: per stream, its readable bytes -- or, with dlens (device), the
// capacity of in[i], the length itself being dlens[i]
static int64_t decompress_batch(const void* const* in, const size_t* in_nbytes, const int64_t* dlens,
                                void* const* out, const size_t* sizes, size_t count,
                                size_t elem_size, size_t block_size, void* ws, size_t ws_bytes,
                                int64_t* d_results, void* stream) {
    BatchPlan bp;
    const int64_t r = make_batch(in, out, sizes, in_nbytes, count, elem_size, block_size, bp);
    if (r) return r;
    if (!have_device()) return kErrHip;
    hipStream_t s = (hipStream_t)stream;
    for (size_t i = 0; i < count; i++) bp.segs[i].result = d_results + i;
    if ((int64_t)bp.L.bs * bp.L.E > max_lds_decode_bytes()) {
        // blocks above the LDS decoder's size: one stream at a time, each in
        // the caller's workspace when there is one
        if (ws && (ws_bytes < dec_per_stream_ws(in_nbytes, sizes, count, elem_size, block_size) ||
                   ((uintptr_t)ws & 255)))
            return kErrUnsupported;
        for (size_t i = 0; i < count; i++) {
            const int64_t e = decompress_dev(in[i], in_nbytes[i], dlens ? dlens + i : nullptr, out[i],
                                             sizes[i], elem_size, block_size, ws, ws ? ws_bytes : 0, d_results + i,
                                             nullptr, stream);
            if (e) return e;
        }
        return 0;
    }
    DevBuf own;
    const size_t need = dec_batch_ws(bp, nullptr, nullptr, nullptr, nullptr, nullptr);
    const int64_t w = get_ws(ws, ws_bytes, need, own, s);
    if (w) return w;
    DecodeBufs b;
    Seg* dsegs = nullptr;
    uint32_t *blk_seg = nullptr, *chunk_seg = nullptr;
    dec_batch_ws(bp, &b, &dsegs, &blk_seg, &chunk_seg, (uint8_t*)ws);
    if (stage_upload(bp.segs.data(), count * sizeof(Seg), dsegs, s) != hipSuccess ||
        (dlens && launch_seg_dlen(dsegs, dlens, (int)count, s) != hipSuccess) ||
        launch_seg_map(dsegs, (int)count, blk_seg, false, s) != hipSuccess ||
        launch_seg_map(dsegs, (int)count, chunk_seg, true, s) != hipSuccess ||
        launch_index_batch(dsegs, (int)count, chunk_seg, bp.L, bp.nchunks, b, s) != hipSuccess ||
        launch_decode_batch(dsegs, bp.segs.data(), (int)count, blk_seg, bp.L, b, s, dlens) != hipSuccess)
        return kErrHip;
    return 0;
}

int64_t bshuf_decompress_lz4_batch_dev(const void* const* in, const size_t* in_nbytes,
                                       void* const* out, const size_t* sizes, size_t count,
                                       size_t elem_size, size_t block_size, void* ws,
                                       size_t ws_bytes, int64_t* d_results, void* stream) {
    return decompress_batch(in, in_nbytes, nullptr, out, sizes, count, elem_size, block_size, ws,
                            ws_bytes, d_results, stream);
}

int64_t bshuf_decompress_lz4_batch_dev_dlen(const void* const* in, const int64_t* d_in_nbytes,
                                            const size_t* in_capacity, void* const* out,
                                            const size_t* sizes, size_t count, size_t elem_size,
                                            size_t block_size, void* ws, size_t ws_bytes,
                                            int64_t* d_results, void* stream) {
    if (!d_in_nbytes) return kErrUnsupported;
    return decompress_batch(in, in_capacity, d_in_nbytes, out, sizes, count, elem_size, block_size,
                            ws, ws_bytes, d_results, stream);
}

// ---------------------------------------------------------------------------
// element ranges of one stream
// ---------------------------------------------------------------------------

namespace {

// The pieces of every range of a call (range_plan.h), before they have
// addresses: decode pieces (interior blocks, edge blocks) and tail spans.
struct ProtoPiece {
    int kind;
    int64_t b0, nblk;  // decode pieces: blocks of the stream
    int64_t nfull;     // ... of which full ones
    int32_t last;      // ... and the elements of the stream's partial block, when it is one of them
    int64_t dst;       // byte offset in the output (interior, clip, tail span)
    int64_t lo, n;     // edge: clip bytes of the staging block; tail span: bytes of the tail
    int64_t slot;      // edge: its staging block
};

struct RangePlan {
    std::vector<ProtoPiece> dec, tails;
    int64_t nblk = 0;       // work blocks (every decode piece's)
    int64_t nedge = 0;      // staging blocks
    int64_t max_blk = 0;    // most blocks / elements of one piece (large blocks: one piece at a time)
    int64_t max_elems = 0;
    int64_t seq_words = 0;  // token positions: a private area per piece, or (shared_seq) the
    bool shared_seq = false;  // whole decode's area indexed by stream offset, when that is smaller
    int64_t total = 0;      // output bytes
    bool large = false;
};

int64_t plan_ranges(const Plan& p, size_t size, size_t in_nbytes, const size_t* starts,
                    const size_t* counts, size_t nranges, RangePlan& rp) {
    if (nranges > (size_t)INT32_MAX / 4) return kErrUnsupported;
    const Layout& L = p.L;
    const int64_t E = L.E, maxlen = lz4_bound(L.bs * L.E);
    int64_t private_words = 0;
    auto add_dec = [&](int kind, int64_t b0, int64_t b1, int64_t dst, int64_t lo, int64_t n) {
        ProtoPiece q{};
        q.kind = kind;
        q.b0 = b0;
        q.nblk = b1 - b0;
        q.nfull = std::min(b1, L.nfull) - b0;
        q.last = b1 > L.nfull ? L.last : 0;
        q.dst = dst;
        q.lo = lo;
        q.n = n;
        q.slot = kind == kPieceEdge ? rp.nedge++ : 0;
        rp.nblk += q.nblk;
        rp.max_blk = std::max(rp.max_blk, q.nblk);
        rp.max_elems = std::max(rp.max_elems, q.nfull * L.bs + q.last);
        private_words += q.nblk * (4 + maxlen) / 3 + 80;
        rp.dec.push_back(q);
    };
    for (size_t i = 0; i < nranges; i++) {
        if (starts[i] > size || counts[i] > size - starts[i]) return kErrUnsupported;
        RangePieces r;
        range_pieces((int64_t)size, L.bs, E, (int64_t)starts[i], (int64_t)counts[i], rp.total, r);
        rp.total += (int64_t)counts[i] * E;
        if (r.b1 > r.b0) add_dec(kPieceInterior, r.b0, r.b1, r.int_dst, 0, 0);
        for (const RangeEdge* e : {&r.head, &r.tail})
            if (e->hi > e->lo) add_dec(kPieceEdge, e->blk, e->blk + 1, e->dst, e->lo * E, (e->hi - e->lo) * E);
        if (r.tail_n > 0) {
            ProtoPiece q{};
            q.kind = kPieceTail;
            q.dst = r.tail_dst;
            q.lo = r.tail_lo * E;
            q.n = r.tail_n * E;
            rp.tails.push_back(q);
        }
    }
    if (rp.nblk >= ((int64_t)1 << 31)) return kErrUnsupported;
    rp.large = (int64_t)L.bs * L.E > max_lds_decode_bytes();
    const int64_t shared_words = (int64_t)in_nbytes / 3 + 80;
    rp.shared_seq = rp.large || shared_words < private_words;
    rp.seq_words = rp.shared_seq ? shared_words : private_words;
    return 0;
}

// The buffers of the whole-stream index rebuild of a range or window call
// (x.offs: the block index), carved whether or not the caller supplies an
// index: one size per call shape.
void carve_index(Carver& c, const Plan& p, int64_t blocks_end, DecodeBufs& x) {
    x.chunk = index_chunk_bytes(p.L);
    x.nchunks = blocks_end > 0 ? (blocks_end + x.chunk - 1) / x.chunk : 0;
    x.offs = c.take<uint64_t>((size_t)p.nb * 8 + 8);
    x.exits = c.take<int64_t>((size_t)x.nchunks * 8 + 8);
    x.cnt = c.take<uint64_t>((size_t)(x.nchunks + 1) * 8);
    x.base = c.take<uint64_t>((size_t)(x.nchunks + 1) * 8);
    x.idx_err = c.take<int64_t>(8);
    x.scan_tmp_bytes = decode_scan_tmp_bytes(x.nchunks);
    x.scan_tmp = c.take<void>(x.scan_tmp_bytes + 8);
}

// The stream of a range or window call as its kernels see it, with the caller's
// block index, or, without one, the index that the rebuild launched here writes
// into idx; idx_err is then the rebuild's error word, else nullptr.
hipError_t stream_with_index(const uint8_t* in, size_t in_nbytes, int64_t blocks_end, const Plan& p,
                             const uint64_t* block_offsets, const DecodeBufs& idx, hipStream_t s,
                             RangeStream& st, const int64_t*& idx_err) {
    st = RangeStream{in, (int64_t)in_nbytes, block_offsets, p.nb, p.tail, (uint32_t)lz4_bound(p.L.bs * p.L.E)};
    idx_err = nullptr;
    if (block_offsets) return hipSuccess;
    st.offs = idx.offs;
    idx_err = idx.idx_err;
    return launch_index(in, blocks_end, p.L, idx, s, nullptr, (int64_t)in_nbytes, p.tail);
}

struct RangeBufs {
    Seg* segs;          // one per decode piece; behind them (16-aligned) the RangePiece table
    RangePiece* pcs;
    size_t tab_bytes;   // ... both, as uploaded
    uint32_t* blk_seg;
    DecodeBufs d;       // offs: the work list; idx_err: zeros, one per decode piece
    int64_t* res;       // one per piece
    uint8_t* slots;     // staging blocks
    int64_t slot;       // bytes of one
    DecodeBufs idx;     // index rebuild of the whole stream (offs: its block index)
};

size_t range_ws(const Plan& p, const RangePlan& rp, int64_t blocks_end, RangeBufs* b, uint8_t* base) {
    Carver c{base};
    RangeBufs x{};
    const size_t nd = rp.dec.size(), np = nd + rp.tails.size();
    const size_t seg_bytes = (nd * sizeof(Seg) + 15) & ~(size_t)15;
    x.tab_bytes = seg_bytes + np * sizeof(RangePiece);
    x.segs = c.take<Seg>(x.tab_bytes);
    x.pcs = reinterpret_cast<RangePiece*>(base ? reinterpret_cast<uint8_t*>(x.segs) + seg_bytes : nullptr);
    const int64_t nwork = rp.large ? rp.max_blk : rp.nblk;
    x.blk_seg = c.take<uint32_t>((size_t)nwork * 4 + 4);
    x.d.offs = c.take<uint64_t>((size_t)nwork * 8 + 8);
    x.d.status = c.take<int64_t>((size_t)nwork * 8 + 8);
    x.d.seq = c.take<uint32_t>((size_t)rp.seq_words * 4);
    x.d.idx_err = c.take<int64_t>(nd * 8 + 8);
    x.d.bad = c.take<long long>(nd * 8 + 8);
    x.d.tickets = c.take<uint32_t>(kTicketSetBytes);
    if (rp.large) x.d.shuf = c.take<uint8_t>((size_t)rp.max_elems * p.L.E + 64);
    x.res = c.take<int64_t>(np * 8 + 8);
    x.slot = ((int64_t)p.L.bs * p.L.E + 15) & ~(int64_t)15;
    x.slots = c.take<uint8_t>((size_t)(rp.nedge * x.slot));
    carve_index(c, p, blocks_end, x.idx);
    if (b) *b = x;
    return c.off;
}

}  // namespace

size_t bshuf_decompress_lz4_ranges_dev_workspace(size_t in_nbytes, size_t size, size_t elem_size,
                                                 size_t block_size, const size_t* starts,
                                                 const size_t* counts, size_t nranges) {
    Plan p;
    RangePlan rp;
    if (make_plan(size, elem_size, block_size, p) ||
        plan_ranges(p, size, in_nbytes, starts, counts, nranges, rp))
        return 0;
    const int64_t cb = (int64_t)in_nbytes - p.tail;
    return range_ws(p, rp, cb > 0 ? cb : 0, nullptr, nullptr);
}

int64_t bshuf_decompress_lz4_ranges_dev(const void* in, size_t in_nbytes, size_t size, size_t elem_size,
                                        size_t block_size, const size_t* starts, const size_t* counts,
                                        size_t nranges, void* out, void* ws, size_t ws_bytes,
                                        int64_t* d_result, const uint64_t* block_offsets, void* stream) {
    Plan p;
    int64_t r = make_plan(size, elem_size, block_size, p);
    if (r) return r;
    RangePlan rp;
    r = plan_ranges(p, size, in_nbytes, starts, counts, nranges, rp);
    if (r) return r;
    if (!have_device()) return kErrHip;
    hipStream_t s = (hipStream_t)stream;
    const size_t nd = rp.dec.size(), np = nd + rp.tails.size();
    if (np == 0) return dev_fill(d_result, 0, sizeof(int64_t), s) == hipSuccess ? 0 : kErrHip;
    int64_t cb = (int64_t)in_nbytes - p.tail;
    if (cb < 0) cb = 0;
    const size_t need = range_ws(p, rp, cb, nullptr, nullptr);
    DevBuf own;
    r = get_ws(ws, ws_bytes, need, own, s);
    if (r) return r;
    RangeBufs b;
    range_ws(p, rp, cb, &b, (uint8_t*)ws);
    const uint8_t* i8 = (const uint8_t*)in;
    uint8_t* o8 = (uint8_t*)out;

    // addresses: the decode pieces whose destination is 16-byte aligned first
    // (every edge's staging block is), then the others: the aligned kernel
    // instantiations for the former, the byte-store path for the latter
    std::vector<uint8_t> tab(b.tab_bytes);
    Seg* hsegs = reinterpret_cast<Seg*>(tab.data());
    RangePiece* hpcs = reinterpret_cast<RangePiece*>(tab.data() + ((uint8_t*)b.pcs - (uint8_t*)b.segs));
    auto where = [&](const ProtoPiece& q) {
        return q.kind == kPieceEdge ? b.slots + q.slot * b.slot : o8 + q.dst;
    };
    size_t at = 0;
    int na = 0;
    int64_t nblk_a = 0, seq_at = 0;
    for (int pass = 0; pass < 2; pass++) {
        int64_t first = 0;
        for (const ProtoPiece& q : rp.dec) {
            uint8_t* dst = where(q);
            if ((((uintptr_t)dst & 15) != 0) != (pass == 1)) continue;
            Seg& g = hsegs[at];
            g = Seg{};
            g.in = i8;
            g.out = dst;
            g.first = first;
            g.nfull = q.nfull;
            g.last = q.last;
            g.in_nbytes = (int64_t)in_nbytes;
            g.result = b.res + at;
            RangePiece& pc = hpcs[at];
            pc = RangePiece{};
            pc.b0 = q.b0;
            pc.nblk = q.nblk;
            pc.seq_base = rp.shared_seq ? -1 : seq_at;
            pc.src = dst + q.lo;
            pc.dst = o8 + q.dst;
            pc.n = q.n;
            pc.kind = q.kind;
            seq_at += q.nblk * (4 + (int64_t)lz4_bound(p.L.bs * p.L.E)) / 3 + 80;
            first += q.nblk;
            at++;
        }
        if (pass == 0) {
            na = (int)at;
            nblk_a = first;
        }
    }
    for (const ProtoPiece& q : rp.tails) {
        RangePiece& pc = hpcs[at++];
        pc = RangePiece{};
        pc.seq_base = -1;
        pc.dst = o8 + q.dst;
        pc.lo = q.lo;
        pc.n = q.n;
        pc.kind = kPieceTail;
    }
    if (stage_upload(tab.data(), tab.size(), b.segs, s) != hipSuccess) return kErrHip;

    RangeStream st;
    const int64_t* idx_err;
    if (stream_with_index(i8, in_nbytes, cb, p, block_offsets, b.idx, s, st, idx_err) != hipSuccess) return kErrHip;
    if (rp.large) {
        // blocks above the LDS decoder's size: one piece at a time through the
        // whole decode's route, its index being the stream's from block b0 on
        for (size_t i = 0; i < nd; i++) {
            Layout L = p.L;
            L.nfull = hsegs[i].nfull;
            L.last = hsegs[i].last;
            DecodeBufs d = b.d;
            d.offs = const_cast<uint64_t*>(st.offs) + hpcs[i].b0;
            d.idx_err = nullptr;
            if (launch_decode(i8, (int64_t)in_nbytes, hsegs[i].out, L, 0, d, b.res + i, s) != hipSuccess)
                return kErrHip;
        }
    } else if (nd) {
        if (dev_fill(b.d.idx_err, 0, nd * 8, s) != hipSuccess ||
            launch_range_worklist(st, b.segs, b.pcs, (int)nd, na, nblk_a, rp.max_blk, b.d.offs, s) != hipSuccess)
            return kErrHip;
        // one scan + decode launch over every 16-byte aligned piece of every
        // range, one over the others
        const int ng[2] = {na, (int)nd - na};
        const int64_t nbk[2] = {nblk_a, rp.nblk - nblk_a};
        for (int g = 0; g < 2; g++) {
            if (ng[g] == 0) continue;
            const int s0 = g ? na : 0;
            const int64_t k0 = g ? nblk_a : 0;
            Layout L = p.L;
            L.nfull = nbk[g];
            L.last = 0;
            DecodeBufs d = b.d;
            d.offs += k0;
            d.status += k0;
            d.idx_err += s0;
            d.bad += s0;
            if (launch_seg_map(b.segs + s0, ng[g], b.blk_seg + k0, false, s) != hipSuccess ||
                launch_decode_batch(b.segs + s0, hsegs + s0, ng[g], b.blk_seg + k0, L, d, s) != hipSuccess)
                return kErrHip;
        }
    }
    if (launch_range_edges(st, b.pcs, b.res, (int)np, s) != hipSuccess ||
        launch_range_reduce(b.res, (int)np, idx_err, rp.total, d_result, s) != hipSuccess)
        return kErrHip;
    return 0;
}

// ---------------------------------------------------------------------------
// fixed-length windows of one stream at device-held starts
// ---------------------------------------------------------------------------

namespace {

// A converting call's bshuf_cvt (launch.h, "converting gathers"): -71 without
// one, for a kind that is not one, for a source kind that is not elem_size
// bytes (so for every elem_size but 1, 2 and 4) and for an `out` that is not
// aligned to the destination's element.
int64_t cvt_check(const bshuf_cvt* cvt, size_t elem_size, const void* out, CvtArgs& a) {
    if (!cvt) return kErrUnsupported;
    if (cvt->src < 0 || cvt->src >= kCvtSrcKinds || cvt->dst < 0 || cvt->dst >= kCvtDstKinds)
        return kErrUnsupported;
    if ((size_t)cvt_src_size(cvt->src) != elem_size) return kErrUnsupported;
    if ((uintptr_t)out % (size_t)cvt_dst_size(cvt->dst)) return kErrUnsupported;
    a = CvtArgs{cvt->src, cvt->dst, cvt->scale, cvt->offset};
    return 0;
}

// What the host knows of a window call, over one stream or over a set:
// everything but the starts (and the stream indices).
struct WindowShape {
    int64_t K = 0, window = 0;
    int64_t Mw = 0;         // work blocks per window
    int64_t seq_words = 0;  // token positions: a private area per window, or (shared_seq) the
    bool shared_seq = false;  // whole decode's area indexed by stream offset, when that is smaller
    int64_t pw = 0;         // words of one private area
    int64_t slot = 0;       // bytes of one staging area
    bool set = false;       // over a set: a stream index per window, no index rebuild
};

// p, size: of the stream, or (set) of the set's largest stream, and then the
// token positions are private: offsets of different streams collide in a shared
// area, and in_nbytes is not looked at.
int64_t window_shape(const Plan& p, size_t size, size_t in_nbytes, size_t nwindows, size_t window, bool set,
                     WindowShape& w) {
    const Layout& L = p.L;
    w.set = set;
    if (window > size) return kErrUnsupported;
    const uint64_t M = window ? ((uint64_t)window + L.bs - 2) / L.bs + 1 : 1;
    if (nwindows >= ((uint64_t)1 << 31) || M >= ((uint64_t)1 << 31) || nwindows * M >= ((uint64_t)1 << 31))
        return kErrUnsupported;
    // (the large-block route decodes one host-known piece at a time)
    if ((int64_t)L.bs * L.E > max_lds_decode_bytes()) return kErrUnsupported;
    w.K = (int64_t)nwindows;
    w.window = (int64_t)window;
    w.Mw = window ? window_blocks((int64_t)size, L.bs, (int64_t)window) : 0;
    const int64_t maxlen = lz4_bound(L.bs * L.E);
    w.pw = w.Mw * (4 + maxlen) / 3 + 80;
    const int64_t shared_words = (int64_t)in_nbytes / 3 + 80;
    w.shared_seq = !set && shared_words < w.K * w.pw;
    w.seq_words = w.shared_seq ? shared_words : w.K * w.pw;
    w.slot = (w.Mw * (int64_t)L.bs * L.E + 15) & ~(int64_t)15;
    return 0;
}

struct WindowBufs {
    Seg* segs;
    RangePiece* pcs;
    WindowTail* wt;
    uint32_t* blk_seg;
    DecodeBufs d;    // offs: the work list; idx_err: zeros, one per window
    int64_t* res;    // one per window: its Seg's result
    int64_t* wstat;  // one per window, when the caller passes no d_status
    uint8_t* slots;  // staging areas
    DecodeBufs idx;  // one stream: index rebuild of the whole stream (offs: its block index)
    int32_t* sidx;   // set: per window, its stream
};

// K Seg, RangePiece and WindowTail records, K * Mw work blocks (map, offsets,
// status), the token positions, K * Mw staging blocks, and the index rebuild's
// buffers (one stream) or the windows' stream indices (set).
size_t window_ws(const Plan& p, const WindowShape& w, int64_t blocks_end, WindowBufs* b, uint8_t* base) {
    Carver c{base};
    WindowBufs x{};
    const size_t K = (size_t)w.K, nwork = (size_t)(w.K * w.Mw);
    x.segs = c.take<Seg>(K * sizeof(Seg));
    x.pcs = c.take<RangePiece>(K * sizeof(RangePiece));
    x.wt = c.take<WindowTail>(K * sizeof(WindowTail));
    x.blk_seg = c.take<uint32_t>(nwork * 4 + 4);
    x.d.offs = c.take<uint64_t>(nwork * 8 + 8);
    x.d.status = c.take<int64_t>(nwork * 8 + 8);
    x.d.seq = c.take<uint32_t>((size_t)w.seq_words * 4);
    x.d.idx_err = c.take<int64_t>(K * 8 + 8);
    x.d.bad = c.take<long long>(K * 8 + 8);
    x.d.tickets = c.take<uint32_t>(kTicketSetBytes);
    x.res = c.take<int64_t>(K * 8 + 8);
    x.wstat = c.take<int64_t>(K * 8 + 8);
    x.slots = c.take<uint8_t>(K * (size_t)w.slot);
    if (w.set)
        x.sidx = c.take<int32_t>(K * 4 + 4);
    else
        carve_index(c, p, blocks_end, x.idx);
    if (b) *b = x;
    return c.off;
}

// What the two window entry points share, from the workspace to the result.
// make_source(b): the call's source, with what of it lies in the workspace.
// worklist(src, c, b, idx_err): the source's index rebuild, if it has one
// (idx_err: its error word), and then, when there are blocks (c.Mw > 0), the
// zeroed per-window error words of the decode and the work list.
extern "C++" template <class MakeSource, class Worklist>
int64_t window_decode(const Plan& p, const WindowShape& w, int64_t blocks_end, size_t need,
                      const int64_t* d_starts, void* out, void* ws, size_t ws_bytes, int64_t* d_result,
                      int64_t* d_status, hipStream_t s, const CvtArgs* cvt, MakeSource make_source,
                      Worklist worklist) {
    DevBuf own;
    const int64_t r = get_ws(ws, ws_bytes, need, own, s);
    if (r) return r;
    WindowBufs b;
    window_ws(p, w, blocks_end, &b, (uint8_t*)ws);
    const int K = (int)w.K;
    int64_t* wstat = d_status ? d_status : b.wstat;

    auto src = make_source(b);
    WindowCall c{};
    c.starts = d_starts;
    c.out = (uint8_t*)out;
    c.slots = b.slots;
    c.res = b.res;
    c.window = w.window;
    c.wbytes = w.window * p.L.E;
    c.slot = w.slot;
    c.Mw = w.Mw;
    c.seq_words = w.shared_seq ? -1 : w.pw;
    c.bs = p.L.bs;
    c.E = p.L.E;
    c.K = K;
    if (launch_window_plan(src, c, b.segs, b.pcs, b.wt, s) != hipSuccess) return kErrHip;
    const int64_t* idx_err = nullptr;
    if (worklist(src, c, b, idx_err) != hipSuccess) return kErrHip;
    if (w.Mw > 0) {
        // every window's staging area is 16-byte aligned: one scan and one
        // decode launch over all K * Mw work blocks, no host copy of the table
        Layout L = p.L;
        L.nfull = w.K * w.Mw;
        L.last = 0;
        if (launch_seg_map(b.segs, K, b.blk_seg, false, s) != hipSuccess ||
            launch_decode_batch(b.segs, nullptr, K, b.blk_seg, L, b.d, s) != hipSuccess)
            return kErrHip;
    }
    if (launch_window_gather(src, c, b.pcs, b.wt, b.d.status, wstat, s, cvt) != hipSuccess ||
        launch_window_reduce(wstat, b.wt, K, idx_err, w.K * c.wbytes, d_result, s) != hipSuccess)
        return kErrHip;
    return 0;
}

}  // namespace

size_t bshuf_decompress_lz4_windows_dev_workspace(size_t in_nbytes, size_t size, size_t elem_size,
                                                  size_t block_size, size_t nwindows, size_t window) {
    Plan p;
    WindowShape w;
    if (make_plan(size, elem_size, block_size, p) || window_shape(p, size, in_nbytes, nwindows, window, false, w))
        return 0;
    const int64_t cb = (int64_t)in_nbytes - p.tail;
    return window_ws(p, w, cb > 0 ? cb : 0, nullptr, nullptr);
}

namespace {
// The entry and its converting twin (cvt: checked, or nullptr).
int64_t windows_dev(const void* in, size_t in_nbytes, size_t size, size_t elem_size, size_t block_size,
                    const int64_t* d_starts, size_t nwindows, size_t window, void* out, void* ws,
                    size_t ws_bytes, int64_t* d_result, int64_t* d_status, const uint64_t* block_offsets,
                    void* stream, const CvtArgs* cvt) {
    Plan p;
    int64_t r = make_plan(size, elem_size, block_size, p);
    if (r) return r;
    WindowShape w;
    r = window_shape(p, size, in_nbytes, nwindows, window, false, w);
    if (r) return r;
    int64_t cb = (int64_t)in_nbytes - p.tail;
    if (cb < 0) cb = 0;
    const size_t need = window_ws(p, w, cb, nullptr, nullptr);
    if (ws && (ws_bytes < need || ((uintptr_t)ws & 255))) return kErrUnsupported;
    if (!have_device()) return kErrHip;
    hipStream_t s = (hipStream_t)stream;
    if (nwindows == 0 || window == 0) return dev_fill(d_result, 0, sizeof(int64_t), s) == hipSuccess ? 0 : kErrHip;
    const uint8_t* i8 = (const uint8_t*)in;
    return window_decode(
        p, w, cb, need, d_starts, out, ws, ws_bytes, d_result, d_status, s, cvt,
        // the plan reads the stream's address and size only: the index comes behind it
        [&](const WindowBufs&) { return WindowStream{RangeStream{i8}, (int64_t)size}; },
        [&](WindowStream& src, const WindowCall& c, const WindowBufs& b, const int64_t*& idx_err) {
            hipError_t e = stream_with_index(i8, in_nbytes, cb, p, block_offsets, b.idx, s, src.st, idx_err);
            if (e != hipSuccess || c.Mw <= 0) return e;
            e = dev_fill(b.d.idx_err, 0, (size_t)c.K * 8, s);
            if (e != hipSuccess) return e;
            return launch_range_worklist(src.st, b.segs, b.pcs, c.K, c.K, 0, c.Mw, b.d.offs, s);
        });
}
}  // namespace

int64_t bshuf_decompress_lz4_windows_dev(const void* in, size_t in_nbytes, size_t size, size_t elem_size,
                                         size_t block_size, const int64_t* d_starts, size_t nwindows,
                                         size_t window, void* out, void* ws, size_t ws_bytes,
                                         int64_t* d_result, int64_t* d_status,
                                         const uint64_t* block_offsets, void* stream) {
    return windows_dev(in, in_nbytes, size, elem_size, block_size, d_starts, nwindows, window, out, ws, ws_bytes,
                       d_result, d_status, block_offsets, stream, nullptr);
}

int64_t bshuf_decompress_lz4_windows_cvt_dev(const void* in, size_t in_nbytes, size_t size, size_t elem_size,
                                             size_t block_size, const int64_t* d_starts, size_t nwindows,
                                             size_t window, void* out, void* ws, size_t ws_bytes,
                                             int64_t* d_result, int64_t* d_status,
                                             const uint64_t* block_offsets, void* stream,
                                             const bshuf_cvt* cvt) {
    CvtArgs a;
    const int64_t r = cvt_check(cvt, elem_size, out, a);
    if (r) return r;
    return windows_dev(in, in_nbytes, size, elem_size, block_size, d_starts, nwindows, window, out, ws, ws_bytes,
                       d_result, d_status, block_offsets, stream, &a);
}

// ---------------------------------------------------------------------------
// fixed-length windows over a set of streams, stream indices and starts
// device-held
// ---------------------------------------------------------------------------

namespace {

// What the host knows of a stream set: the batch table of its index rebuild
// (streams whose index the caller supplies: no blocks and no chunks there).
struct SetPlan {
    BatchPlan bp;               // segs[s].first: stream s's place in the set's index memory
    std::vector<int64_t> nb;    // blocks per stream
    int64_t nb_total = 0, nb_max = 0, ref = -1;
};

int64_t make_set(const void* const* ins, const size_t* in_nbytes, const size_t* sizes, size_t count,
                 size_t elem_size, size_t block_size, const uint64_t* const* block_offsets, SetPlan& sp) {
    Plan p0;
    int64_t r = make_plan(0, elem_size, block_size, p0);
    if (r) return r;
    if ((int64_t)p0.L.bs * p0.L.E > max_lds_decode_bytes()) return kErrUnsupported;
    if (count > (size_t)INT32_MAX) return kErrUnsupported;
    BatchPlan& bp = sp.bp;
    bp.L = p0.L;
    bp.chunk = index_chunk_bytes(p0.L);
    bp.segs.resize(count);
    sp.nb.resize(count);
    for (size_t i = 0; i < count; i++) {
        Plan p;
        r = make_plan(sizes[i], elem_size, block_size, p);
        if (r) return r;
        const bool own = !(block_offsets && block_offsets[i]);
        Seg& g = bp.segs[i];
        g = Seg{};
        g.in = ins ? (const uint8_t*)ins[i] : nullptr;
        g.first = sp.nb_total;
        g.nfull = own ? p.L.nfull : 0;
        g.last = own ? p.L.last : 0;
        g.tail = p.tail;
        g.in_nbytes = in_nbytes ? (int64_t)in_nbytes[i] : 0;
        const int64_t cb = std::max<int64_t>(g.in_nbytes - g.tail, 0);
        g.chunk0 = bp.nchunks;
        g.nchunks = own && cb > 0 ? (cb + bp.chunk - 1) / bp.chunk : 0;
        bp.nchunks += g.nchunks;
        sp.nb[i] = p.nb;
        sp.nb_total += p.nb;
        if (sp.ref < 0 || p.nb > sp.nb_max) {
            sp.nb_max = p.nb;
            sp.ref = (int64_t)i;
        }
        if (sp.nb_total >= ((int64_t)1 << 31) || bp.nchunks >= ((int64_t)1 << 31)) return kErrUnsupported;
    }
    bp.nb = sp.nb_total;
    bp.L.nfull = sp.nb_total;
    bp.L.last = 0;
    return 0;
}

size_t set_bytes_of(size_t count, int64_t nb_total) {
    return al256(kStreamSetRecs + count * sizeof(StreamSetRec)) + al256((size_t)nb_total * 8 + 8);
}

struct SetBufs {
    Seg* segs;
    uint32_t* chunk_seg;
    DecodeBufs idx;
};

// the batched index rebuild's buffers, sized as if no index were supplied
size_t set_ws(const SetPlan& sp, SetBufs* b, uint8_t* base) {
    Carver c{base};
    SetBufs x{};
    const size_t ns = sp.bp.segs.size(), nch = (size_t)sp.bp.nchunks;
    x.segs = c.take<Seg>(ns * sizeof(Seg) + 8);
    x.chunk_seg = c.take<uint32_t>(nch * 4 + 4);
    x.idx.chunk = sp.bp.chunk;
    x.idx.nchunks = sp.bp.nchunks;
    x.idx.exits = c.take<int64_t>(nch * 8 + 8);
    x.idx.cnt = c.take<uint64_t>((nch + 1) * 8);
    x.idx.base = c.take<uint64_t>((nch + 1) * 8);
    x.idx.idx_err = c.take<int64_t>(ns * 8 + 8);
    x.idx.scan_tmp_bytes = decode_scan_tmp_bytes(sp.bp.nchunks);
    x.idx.scan_tmp = c.take<void>(x.idx.scan_tmp_bytes + 8);
    if (b) *b = x;
    return c.off;
}

}  // namespace

size_t bshuf_lz4_stream_set_dev_bytes(const size_t* sizes, size_t count, size_t elem_size, size_t block_size) {
    SetPlan sp;
    if (make_set(nullptr, nullptr, sizes, count, elem_size, block_size, nullptr, sp)) return 0;
    return set_bytes_of(count, sp.nb_total);
}

size_t bshuf_lz4_stream_set_dev_workspace(const size_t* in_nbytes, const size_t* sizes, size_t count,
                                          size_t elem_size, size_t block_size) {
    SetPlan sp;
    if (make_set(nullptr, in_nbytes, sizes, count, elem_size, block_size, nullptr, sp)) return 0;
    return set_ws(sp, nullptr, nullptr);
}

int64_t bshuf_lz4_stream_set_dev(const void* const* ins, const size_t* in_nbytes, const size_t* sizes,
                                 size_t count, size_t elem_size, size_t block_size,
                                 const uint64_t* const* block_offsets, void* d_set, size_t set_bytes, void* ws,
                                 size_t ws_bytes, int64_t* d_status, void* stream) {
    SetPlan sp, full;
    int64_t r = make_set(ins, in_nbytes, sizes, count, elem_size, block_size, block_offsets, sp);
    if (r) return r;
    // the workspace is sized without a look at which indexes are supplied
    r = make_set(nullptr, in_nbytes, sizes, count, elem_size, block_size, nullptr, full);
    if (r) return r;
    const size_t need = set_ws(full, nullptr, nullptr);
    if (!d_set || ((uintptr_t)d_set & 255) || set_bytes < set_bytes_of(count, sp.nb_total)) return kErrUnsupported;
    if (ws && (ws_bytes < need || ((uintptr_t)ws & 255))) return kErrUnsupported;
    if (!have_device()) return kErrHip;
    hipStream_t s = (hipStream_t)stream;
    DevBuf own;
    r = get_ws(ws, ws_bytes, need, own, s);
    if (r) return r;
    SetBufs b;
    set_ws(sp, &b, (uint8_t*)ws);

    uint8_t* set8 = (uint8_t*)d_set;
    uint64_t* index = (uint64_t*)(set8 + al256(kStreamSetRecs + count * sizeof(StreamSetRec)));
    std::vector<uint8_t> table(kStreamSetRecs + count * sizeof(StreamSetRec), 0);
    StreamSetHeader h{};
    h.magic = kStreamSetMagic;
    h.count = (int64_t)count;
    h.E = sp.bp.L.E;
    h.bs = sp.bp.L.bs;
    h.nb_max = sp.nb_max;
    h.ref = sp.ref;
    memcpy(table.data(), &h, sizeof(h));
    const uint32_t maxlen = (uint32_t)lz4_bound(sp.bp.L.bs * sp.bp.L.E);
    for (size_t i = 0; i < count; i++) {
        const Seg& g = sp.bp.segs[i];
        StreamSetRec rec{};
        rec.st.in = g.in;
        rec.st.in_nbytes = g.in_nbytes;
        rec.st.offs = block_offsets && block_offsets[i] ? block_offsets[i] : index + g.first;
        rec.st.nb = sp.nb[i];
        rec.st.tail = g.tail;
        rec.st.maxlen = maxlen;
        rec.size = (int64_t)sizes[i];
        memcpy(table.data() + kStreamSetRecs + i * sizeof(StreamSetRec), &rec, sizeof(rec));
    }
    if (stage_upload(table.data(), table.size(), d_set, s) != hipSuccess) return kErrHip;
    if (count == 0) return 0;
    b.idx.offs = index;
    if (stage_upload(sp.bp.segs.data(), count * sizeof(Seg), b.segs, s) != hipSuccess ||
        launch_seg_map(b.segs, (int)count, b.chunk_seg, true, s) != hipSuccess ||
        launch_index_batch(b.segs, (int)count, b.chunk_seg, sp.bp.L, sp.bp.nchunks, b.idx, s) != hipSuccess ||
        launch_stream_set_status((StreamSetRec*)(set8 + kStreamSetRecs), b.idx.idx_err, d_status, (int)count,
                                 s) != hipSuccess)
        return kErrHip;
    return 0;
}

size_t bshuf_decompress_lz4_windows_set_dev_workspace(size_t max_size, size_t elem_size, size_t block_size,
                                                      size_t nwindows, size_t window) {
    Plan p;
    WindowShape w;
    if (make_plan(max_size, elem_size, block_size, p) || window_shape(p, max_size, 0, nwindows, window, true, w))
        return 0;
    return window_ws(p, w, 0, nullptr, nullptr);
}

namespace {
int64_t windows_set_dev(const void* d_set, size_t count, size_t max_size, size_t elem_size, size_t block_size,
                        const int64_t* d_ids, const int64_t* d_starts, size_t nwindows, size_t window, void* out,
                        void* ws, size_t ws_bytes, int64_t* d_result, int64_t* d_status, void* stream,
                        const CvtArgs* cvt) {
    Plan p;
    int64_t r = make_plan(max_size, elem_size, block_size, p);
    if (r) return r;
    WindowShape w;
    r = window_shape(p, max_size, 0, nwindows, window, true, w);
    if (r) return r;
    if (count > (size_t)INT32_MAX) return kErrUnsupported;
    const size_t need = window_ws(p, w, 0, nullptr, nullptr);
    if (ws && (ws_bytes < need || ((uintptr_t)ws & 255))) return kErrUnsupported;
    if (!d_set || ((uintptr_t)d_set & 255)) return kErrUnsupported;
    if (!have_device()) return kErrHip;
    hipStream_t s = (hipStream_t)stream;
    if (nwindows == 0 || window == 0) return dev_fill(d_result, 0, sizeof(int64_t), s) == hipSuccess ? 0 : kErrHip;
    return window_decode(
        p, w, 0, need, d_starts, out, ws, ws_bytes, d_result, d_status, s, cvt,
        [&](const WindowBufs& b) {
            return WindowSet{(const StreamSetHeader*)d_set,
                             (const StreamSetRec*)((const uint8_t*)d_set + kStreamSetRecs),
                             d_ids,
                             b.sidx,
                             (int64_t)count,
                             p.nb};
        },
        // (the set's indexes were made by its build: nothing to rebuild)
        [&](const WindowSet& src, const WindowCall& c, const WindowBufs& b, const int64_t*&) {
            if (c.Mw <= 0) return hipSuccess;
            const hipError_t e = dev_fill(b.d.idx_err, 0, (size_t)c.K * 8, s);
            if (e != hipSuccess) return e;
            return launch_window_set_worklist(src, c, b.segs, b.pcs, b.d.offs, s);
        });
}
}  // namespace

int64_t bshuf_decompress_lz4_windows_set_dev(const void* d_set, size_t count, size_t max_size, size_t elem_size,
                                             size_t block_size, const int64_t* d_ids, const int64_t* d_starts,
                                             size_t nwindows, size_t window, void* out, void* ws,
                                             size_t ws_bytes, int64_t* d_result, int64_t* d_status,
                                             void* stream) {
    return windows_set_dev(d_set, count, max_size, elem_size, block_size, d_ids, d_starts, nwindows, window, out,
                           ws, ws_bytes, d_result, d_status, stream, nullptr);
}

int64_t bshuf_decompress_lz4_windows_set_cvt_dev(const void* d_set, size_t count, size_t max_size,
                                                 size_t elem_size, size_t block_size, const int64_t* d_ids,
                                                 const int64_t* d_starts, size_t nwindows, size_t window,
                                                 void* out, void* ws, size_t ws_bytes, int64_t* d_result,
                                                 int64_t* d_status, void* stream, const bshuf_cvt* cvt) {
    CvtArgs a;
    const int64_t r = cvt_check(cvt, elem_size, out, a);
    if (r) return r;
    return windows_set_dev(d_set, count, max_size, elem_size, block_size, d_ids, d_starts, nwindows, window, out,
                           ws, ws_bytes, d_result, d_status, stream, &a);
}

// ---------------------------------------------------------------------------
// ragged windows: device-held starts and lengths, of one stream or of a set,
// packed (values + offsets) or at a fixed pitch
// ---------------------------------------------------------------------------

namespace {

// The window decode's buffers for windows of max_window elements, and behind
// them the placement scan's.
struct RaggedBufs {
    WindowBufs w;
    int64_t* offs;  // K + 1: the windows' places, when the caller passes no d_out_offsets
    int64_t* sums;  // the scan's tile sums
};

size_t ragged_ws(const Plan& p, const WindowShape& w, int64_t blocks_end, RaggedBufs* b, uint8_t* base) {
    RaggedBufs x{};
    Carver c{base};
    c.off = window_ws(p, w, blocks_end, &x.w, base);
    x.offs = c.take<int64_t>(((size_t)w.K + 1) * 8);
    x.sums = c.take<int64_t>((size_t)kRaggedScanTiles * 8);
    if (b) *b = x;
    return c.off;
}

// What the host refuses of the output's description.
int64_t ragged_output(size_t nwindows, size_t max_window, size_t out_capacity, size_t out_pitch,
                      const int64_t* d_out_offsets) {
    if (out_capacity >= ((uint64_t)1 << 62) || out_pitch >= ((uint64_t)1 << 62)) return kErrUnsupported;
    if (out_pitch == 0) return d_out_offsets ? 0 : kErrUnsupported;
    if (out_pitch < max_window) return kErrUnsupported;
    if (nwindows && out_pitch > out_capacity / nwindows) return kErrUnsupported;
    return 0;
}

// Nothing to decode (no windows, or none longer than 0): result 0, offsets 0.
int64_t ragged_empty(size_t nwindows, int64_t* d_out_offsets, int64_t* d_result, hipStream_t s) {
    if (dev_fill(d_result, 0, sizeof(int64_t), s) != hipSuccess) return kErrHip;
    if (d_out_offsets && dev_fill(d_out_offsets, 0, (nwindows + 1) * sizeof(int64_t), s) != hipSuccess)
        return kErrHip;
    return 0;
}

// What the two ragged entry points share, from the workspace to the result:
// one linear chain on s.  make_source(b): the call's source, with what of it
// lies in the workspace.  index(src, b, idx_err): the source's index rebuild,
// if it has one (idx_err: its error word).
extern "C++" template <class MakeSource, class Index>
int64_t ragged_decode(const Plan& p, const WindowShape& w, int64_t blocks_end, size_t need,
                      const int64_t* d_starts, const int64_t* d_counts, void* out, size_t out_capacity,
                      size_t out_pitch, int64_t* d_out_offsets, void* ws, size_t ws_bytes, int64_t* d_result,
                      int64_t* d_status, hipStream_t s, const CvtArgs* cvt, MakeSource make_source,
                      Index index) {
    DevBuf own;
    const int64_t r = get_ws(ws, ws_bytes, need, own, s);
    if (r) return r;
    RaggedBufs rb;
    ragged_ws(p, w, blocks_end, &rb, (uint8_t*)ws);
    const WindowBufs& b = rb.w;
    const int K = (int)w.K;
    int64_t* wstat = d_status ? d_status : b.wstat;

    auto src = make_source(b);
    RaggedCall c{};
    c.w.starts = d_starts;
    c.w.out = (uint8_t*)out;
    c.w.slots = b.slots;
    c.w.res = b.res;
    c.w.window = w.window;
    c.w.wbytes = w.window * p.L.E;
    c.w.slot = w.slot;
    c.w.Mw = w.Mw;
    c.w.seq_words = w.shared_seq ? -1 : w.pw;
    c.w.bs = p.L.bs;
    c.w.E = p.L.E;
    c.w.K = K;
    c.counts = d_counts;
    c.offs = d_out_offsets ? d_out_offsets : rb.offs;
    c.capacity = (int64_t)out_capacity;
    c.pitch = (int64_t)out_pitch;
    if (launch_ragged_scan(src, c, rb.sums, s) != hipSuccess ||
        launch_ragged_plan(src, c, b.segs, b.pcs, b.wt, s) != hipSuccess)
        return kErrHip;
    const int64_t* idx_err = nullptr;
    if (index(src, b, idx_err) != hipSuccess) return kErrHip;
    if (w.Mw > 0) {
        // as window_decode: one scan and one decode launch over all K * Mw work
        // blocks, most of them inert when the windows are short
        Layout L = p.L;
        L.nfull = w.K * w.Mw;
        L.last = 0;
        if (dev_fill(b.d.idx_err, 0, (size_t)K * 8, s) != hipSuccess ||
            launch_ragged_worklist(src, c, b.segs, b.pcs, b.wt, b.d.offs, b.blk_seg, s) != hipSuccess ||
            launch_decode_batch(b.segs, nullptr, K, b.blk_seg, L, b.d, s) != hipSuccess)
            return kErrHip;
    }
    if (launch_ragged_gather(src, c, b.pcs, b.wt, b.d.status, wstat, s, cvt) != hipSuccess ||
        launch_window_reduce(wstat, b.wt, K, idx_err, p.L.E, d_result, s, c.offs + K) != hipSuccess)
        return kErrHip;
    return 0;
}

}  // namespace

size_t bshuf_decompress_lz4_ragged_dev_workspace(size_t in_nbytes, size_t size, size_t elem_size,
                                                 size_t block_size, size_t nwindows, size_t max_window) {
    Plan p;
    WindowShape w;
    if (make_plan(size, elem_size, block_size, p) ||
        window_shape(p, size, in_nbytes, nwindows, max_window, false, w))
        return 0;
    const int64_t cb = (int64_t)in_nbytes - p.tail;
    return ragged_ws(p, w, cb > 0 ? cb : 0, nullptr, nullptr);
}

namespace {
int64_t ragged_dev(const void* in, size_t in_nbytes, size_t size, size_t elem_size, size_t block_size,
                   const int64_t* d_starts, const int64_t* d_counts, size_t nwindows, size_t max_window, void* out,
                   size_t out_capacity, size_t out_pitch, int64_t* d_out_offsets, void* ws, size_t ws_bytes,
                   int64_t* d_result, int64_t* d_status, const uint64_t* block_offsets, void* stream,
                   const CvtArgs* cvt) {
    Plan p;
    int64_t r = make_plan(size, elem_size, block_size, p);
    if (r) return r;
    WindowShape w;
    r = window_shape(p, size, in_nbytes, nwindows, max_window, false, w);
    if (r) return r;
    r = ragged_output(nwindows, max_window, out_capacity, out_pitch, d_out_offsets);
    if (r) return r;
    int64_t cb = (int64_t)in_nbytes - p.tail;
    if (cb < 0) cb = 0;
    const size_t need = ragged_ws(p, w, cb, nullptr, nullptr);
    if (ws && (ws_bytes < need || ((uintptr_t)ws & 255))) return kErrUnsupported;
    if (!have_device()) return kErrHip;
    hipStream_t s = (hipStream_t)stream;
    if (nwindows == 0 || max_window == 0) return ragged_empty(nwindows, d_out_offsets, d_result, s);
    const uint8_t* i8 = (const uint8_t*)in;
    return ragged_decode(
        p, w, cb, need, d_starts, d_counts, out, out_capacity, out_pitch, d_out_offsets, ws, ws_bytes, d_result,
        d_status, s, cvt,
        // the scan and the plan read the stream's address and size only: the index comes behind them
        [&](const WindowBufs&) { return WindowStream{RangeStream{i8}, (int64_t)size}; },
        [&](WindowStream& src, const WindowBufs& b, const int64_t*& idx_err) {
            return stream_with_index(i8, in_nbytes, cb, p, block_offsets, b.idx, s, src.st, idx_err);
        });
}
}  // namespace

int64_t bshuf_decompress_lz4_ragged_dev(const void* in, size_t in_nbytes, size_t size, size_t elem_size,
                                        size_t block_size, const int64_t* d_starts, const int64_t* d_counts,
                                        size_t nwindows, size_t max_window, void* out, size_t out_capacity,
                                        size_t out_pitch, int64_t* d_out_offsets, void* ws, size_t ws_bytes,
                                        int64_t* d_result, int64_t* d_status, const uint64_t* block_offsets,
                                        void* stream) {
    return ragged_dev(in, in_nbytes, size, elem_size, block_size, d_starts, d_counts, nwindows, max_window, out,
                      out_capacity, out_pitch, d_out_offsets, ws, ws_bytes, d_result, d_status, block_offsets,
                      stream, nullptr);
}

int64_t bshuf_decompress_lz4_ragged_cvt_dev(const void* in, size_t in_nbytes, size_t size, size_t elem_size,
                                            size_t block_size, const int64_t* d_starts, const int64_t* d_counts,
                                            size_t nwindows, size_t max_window, void* out, size_t out_capacity,
                                            size_t out_pitch, int64_t* d_out_offsets, void* ws, size_t ws_bytes,
                                            int64_t* d_result, int64_t* d_status,
                                            const uint64_t* block_offsets, void* stream, const bshuf_cvt* cvt) {
    CvtArgs a;
    const int64_t r = cvt_check(cvt, elem_size, out, a);
    if (r) return r;
    return ragged_dev(in, in_nbytes, size, elem_size, block_size, d_starts, d_counts, nwindows, max_window, out,
                      out_capacity, out_pitch, d_out_offsets, ws, ws_bytes, d_result, d_status, block_offsets,
                      stream, &a);
}

size_t bshuf_decompress_lz4_ragged_set_dev_workspace(size_t max_size, size_t elem_size, size_t block_size,
                                                     size_t nwindows, size_t max_window) {
    Plan p;
    WindowShape w;
    if (make_plan(max_size, elem_size, block_size, p) ||
        window_shape(p, max_size, 0, nwindows, max_window, true, w))
        return 0;
    return ragged_ws(p, w, 0, nullptr, nullptr);
}

namespace {
int64_t ragged_set_dev(const void* d_set, size_t count, size_t max_size, size_t elem_size, size_t block_size,
                       const int64_t* d_ids, const int64_t* d_starts, const int64_t* d_counts, size_t nwindows,
                       size_t max_window, void* out, size_t out_capacity, size_t out_pitch,
                       int64_t* d_out_offsets, void* ws, size_t ws_bytes, int64_t* d_result, int64_t* d_status,
                       void* stream, const CvtArgs* cvt) {
    Plan p;
    int64_t r = make_plan(max_size, elem_size, block_size, p);
    if (r) return r;
    WindowShape w;
    r = window_shape(p, max_size, 0, nwindows, max_window, true, w);
    if (r) return r;
    r = ragged_output(nwindows, max_window, out_capacity, out_pitch, d_out_offsets);
    if (r) return r;
    if (count > (size_t)INT32_MAX) return kErrUnsupported;
    const size_t need = ragged_ws(p, w, 0, nullptr, nullptr);
    if (ws && (ws_bytes < need || ((uintptr_t)ws & 255))) return kErrUnsupported;
    if (!d_set || ((uintptr_t)d_set & 255)) return kErrUnsupported;
    if (!have_device()) return kErrHip;
    hipStream_t s = (hipStream_t)stream;
    if (nwindows == 0 || max_window == 0) return ragged_empty(nwindows, d_out_offsets, d_result, s);
    return ragged_decode(
        p, w, 0, need, d_starts, d_counts, out, out_capacity, out_pitch, d_out_offsets, ws, ws_bytes, d_result,
        d_status, s, cvt,
        [&](const WindowBufs& b) {
            return WindowSet{(const StreamSetHeader*)d_set,
                             (const StreamSetRec*)((const uint8_t*)d_set + kStreamSetRecs),
                             d_ids,
                             b.sidx,
                             (int64_t)count,
                             p.nb};
        },
        // (the set's indexes were made by its build: nothing to rebuild)
        [&](const WindowSet&, const WindowBufs&, const int64_t*&) { return hipSuccess; });
}
}  // namespace

int64_t bshuf_decompress_lz4_ragged_set_dev(const void* d_set, size_t count, size_t max_size, size_t elem_size,
                                            size_t block_size, const int64_t* d_ids, const int64_t* d_starts,
                                            const int64_t* d_counts, size_t nwindows, size_t max_window,
                                            void* out, size_t out_capacity, size_t out_pitch,
                                            int64_t* d_out_offsets, void* ws, size_t ws_bytes,
                                            int64_t* d_result, int64_t* d_status, void* stream) {
    return ragged_set_dev(d_set, count, max_size, elem_size, block_size, d_ids, d_starts, d_counts, nwindows,
                          max_window, out, out_capacity, out_pitch, d_out_offsets, ws, ws_bytes, d_result,
                          d_status, stream, nullptr);
}

int64_t bshuf_decompress_lz4_ragged_set_cvt_dev(const void* d_set, size_t count, size_t max_size,
                                                size_t elem_size, size_t block_size, const int64_t* d_ids,
                                                const int64_t* d_starts, const int64_t* d_counts,
                                                size_t nwindows, size_t max_window, void* out,
                                                size_t out_capacity, size_t out_pitch, int64_t* d_out_offsets,
                                                void* ws, size_t ws_bytes, int64_t* d_result, int64_t* d_status,
                                                void* stream, const bshuf_cvt* cvt) {
    CvtArgs a;
    const int64_t r = cvt_check(cvt, elem_size, out, a);
    if (r) return r;
    return ragged_set_dev(d_set, count, max_size, elem_size, block_size, d_ids, d_starts, d_counts, nwindows,
                          max_window, out, out_capacity, out_pitch, d_out_offsets, ws, ws_bytes, d_result,
                          d_status, stream, &a);
}

// ---------------------------------------------------------------------------
// rows x cols tiles at device-held flat starts, of one stream or of a set
// ---------------------------------------------------------------------------

namespace {

// What the host knows of a tile call, over one stream or over a set:
// everything but the starts (and the stream indices).
struct TileShapeH {
    int64_t K = 0, rows = 0, cols = 0, pitch = 0;
    TileShape t{0, 0, 0};   // rg, G, Mg (tile_plan.h)
    int64_t seq_words = 0;  // token positions: a private area per group, or (shared_seq) the
    bool shared_seq = false;  // whole decode's area indexed by stream offset, when that is smaller
    int64_t pw = 0;         // words of one private area
    int64_t slot = 0;       // bytes of one staging area
    bool set = false;       // over a set: a stream index per group, no index rebuild
    bool empty = false;     // ntiles, rows or cols is 0: nothing to decode
};

// p, size: of the stream, or (set) of the set's largest stream; as window_shape.
int64_t tile_shape_host(const Plan& p, size_t size, size_t in_nbytes, size_t ntiles, size_t rows, size_t cols,
                        size_t pitch, bool set, TileShapeH& w) {
    const Layout& L = p.L;
    w.set = set;
    w.empty = ntiles == 0 || rows == 0 || cols == 0;
    if (ntiles >= ((uint64_t)1 << 31)) return kErrUnsupported;
    if ((int64_t)L.bs * L.E > max_lds_decode_bytes()) return kErrUnsupported;
    w.K = (int64_t)ntiles;
    if (!w.empty) {
        if (pitch < cols) return kErrUnsupported;
        // span = (rows - 1) * pitch + cols <= size, without overflow
        if (cols > size || (rows > 1 && pitch > (size - cols) / (rows - 1))) return kErrUnsupported;
        // the output's byte count fits int64
        const unsigned __int128 total = (unsigned __int128)ntiles * rows * cols * (uint64_t)L.E;
        if (total >= ((unsigned __int128)1 << 62)) return kErrUnsupported;
        w.rows = (int64_t)rows;
        w.cols = (int64_t)cols;
        w.pitch = (int64_t)pitch;
        tile_shape(w.rows, w.cols, w.pitch, L.bs, p.nb, w.t);
        const unsigned __int128 pieces = (unsigned __int128)ntiles * (uint64_t)w.t.G;
        if (pieces >= ((uint64_t)1 << 31) || pieces * (uint64_t)w.t.Mg >= ((uint64_t)1 << 31)) return kErrUnsupported;
    }
    const int64_t maxlen = lz4_bound(L.bs * L.E);
    const int64_t pieces = w.K * w.t.G;
    w.pw = w.t.Mg * (4 + maxlen) / 3 + 80;
    const int64_t shared_words = (int64_t)in_nbytes / 3 + 80;
    w.shared_seq = !set && shared_words < pieces * w.pw;
    w.seq_words = w.shared_seq ? shared_words : pieces * w.pw;
    w.slot = (w.t.Mg * (int64_t)L.bs * L.E + 15) & ~(int64_t)15;
    return 0;
}

struct TileBufs {
    Seg* segs;
    RangePiece* pcs;
    TileInfo* ti;
    uint32_t* blk_seg;
    DecodeBufs d;    // offs: the work list; idx_err: zeros, one per group
    int64_t* res;    // one per group: its Seg's result
    int64_t* tstat;  // one per tile, when the caller passes no d_status
    uint8_t* slots;  // staging areas
    DecodeBufs idx;  // one stream: index rebuild of the whole stream (offs: its block index)
    int32_t* sidx;   // set: per group, its stream
};

// K * G Seg and RangePiece records, K TileInfo, K * G * Mg work blocks (map,
// offsets, status), the token positions, K * G staging areas of Mg blocks, and
// the index rebuild's buffers (one stream) or the groups' stream indices (set).
size_t tile_ws(const Plan& p, const TileShapeH& w, int64_t blocks_end, TileBufs* b, uint8_t* base) {
    Carver c{base};
    TileBufs x{};
    const size_t K = (size_t)w.K, P = (size_t)(w.K * w.t.G), nwork = P * (size_t)w.t.Mg;
    x.segs = c.take<Seg>(P * sizeof(Seg));
    x.pcs = c.take<RangePiece>(P * sizeof(RangePiece));
    x.ti = c.take<TileInfo>(K * sizeof(TileInfo));
    x.blk_seg = c.take<uint32_t>(nwork * 4 + 4);
    x.d.offs = c.take<uint64_t>(nwork * 8 + 8);
    x.d.status = c.take<int64_t>(nwork * 8 + 8);
    x.d.seq = c.take<uint32_t>((size_t)w.seq_words * 4);
    x.d.idx_err = c.take<int64_t>(P * 8 + 8);
    x.d.bad = c.take<long long>(P * 8 + 8);
    x.d.tickets = c.take<uint32_t>(kTicketSetBytes);
    x.res = c.take<int64_t>(P * 8 + 8);
    x.tstat = c.take<int64_t>(K * 8 + 8);
    x.slots = c.take<uint8_t>(P * (size_t)w.slot);
    if (w.set)
        x.sidx = c.take<int32_t>(P * 4 + 4);
    else
        carve_index(c, p, blocks_end, x.idx);
    if (b) *b = x;
    return c.off;
}

// What the two tile entry points share, from the workspace to the result; the
// two callables as window_decode's, with a group in a window's place.
extern "C++" template <class MakeSource, class Worklist>
int64_t tile_decode(const Plan& p, const TileShapeH& w, int64_t blocks_end, size_t need, const int64_t* d_starts,
                    void* out, void* ws, size_t ws_bytes, int64_t* d_result, int64_t* d_status, hipStream_t s,
                    const CvtArgs* cvt, MakeSource make_source, Worklist worklist) {
    DevBuf own;
    const int64_t r = get_ws(ws, ws_bytes, need, own, s);
    if (r) return r;
    TileBufs b;
    tile_ws(p, w, blocks_end, &b, (uint8_t*)ws);
    const int K = (int)w.K, P = (int)(w.K * w.t.G);
    int64_t* tstat = d_status ? d_status : b.tstat;

    auto src = make_source(b);
    TileCall c{};
    c.starts = d_starts;
    c.out = (uint8_t*)out;
    c.slots = b.slots;
    c.res = b.res;
    c.rows = w.rows;
    c.cols = w.cols;
    c.pitch = w.pitch;
    c.rg = w.t.rg;
    c.G = w.t.G;
    c.Mg = w.t.Mg;
    c.rbytes = w.cols * p.L.E;
    c.slot = w.slot;
    c.seq_words = w.shared_seq ? -1 : w.pw;
    c.bs = p.L.bs;
    c.E = p.L.E;
    c.K = K;
    if (launch_tile_plan(src, c, b.segs, b.pcs, b.ti, s) != hipSuccess) return kErrHip;
    const int64_t* idx_err = nullptr;
    if (worklist(src, c, b, idx_err) != hipSuccess) return kErrHip;
    if (c.Mg > 0) {
        // every group's staging area is 16-byte aligned: one scan and one decode
        // launch over all K * G * Mg work blocks, no host copy of the table
        Layout L = p.L;
        L.nfull = (int64_t)P * c.Mg;
        L.last = 0;
        if (launch_seg_map(b.segs, P, b.blk_seg, false, s) != hipSuccess ||
            launch_decode_batch(b.segs, nullptr, P, b.blk_seg, L, b.d, s) != hipSuccess)
            return kErrHip;
    }
    if (launch_tile_gather(src, c, b.pcs, b.ti, b.d.status, tstat, s, cvt) != hipSuccess ||
        launch_tile_reduce(tstat, b.ti, K, idx_err, w.K * c.rows * c.rbytes, d_result, s) != hipSuccess)
        return kErrHip;
    return 0;
}

}  // namespace

size_t bshuf_decompress_lz4_tiles_dev_workspace(size_t in_nbytes, size_t size, size_t elem_size,
                                                size_t block_size, size_t ntiles, size_t rows, size_t cols,
                                                size_t pitch) {
    Plan p;
    TileShapeH w;
    if (make_plan(size, elem_size, block_size, p) ||
        tile_shape_host(p, size, in_nbytes, ntiles, rows, cols, pitch, false, w))
        return 0;
    const int64_t cb = (int64_t)in_nbytes - p.tail;
    return tile_ws(p, w, cb > 0 ? cb : 0, nullptr, nullptr);
}

namespace {
int64_t tiles_dev(const void* in, size_t in_nbytes, size_t size, size_t elem_size, size_t block_size,
                  const int64_t* d_starts, size_t ntiles, size_t rows, size_t cols, size_t pitch, void* out,
                  void* ws, size_t ws_bytes, int64_t* d_result, int64_t* d_status, const uint64_t* block_offsets,
                  void* stream, const CvtArgs* cvt) {
    Plan p;
    int64_t r = make_plan(size, elem_size, block_size, p);
    if (r) return r;
    TileShapeH w;
    r = tile_shape_host(p, size, in_nbytes, ntiles, rows, cols, pitch, false, w);
    if (r) return r;
    int64_t cb = (int64_t)in_nbytes - p.tail;
    if (cb < 0) cb = 0;
    const size_t need = tile_ws(p, w, cb, nullptr, nullptr);
    if (ws && (ws_bytes < need || ((uintptr_t)ws & 255))) return kErrUnsupported;
    if (!have_device()) return kErrHip;
    hipStream_t s = (hipStream_t)stream;
    if (w.empty) return dev_fill(d_result, 0, sizeof(int64_t), s) == hipSuccess ? 0 : kErrHip;
    const uint8_t* i8 = (const uint8_t*)in;
    return tile_decode(
        p, w, cb, need, d_starts, out, ws, ws_bytes, d_result, d_status, s, cvt,
        // the plan reads the stream's address and size only: the index comes behind it
        [&](const TileBufs&) { return WindowStream{RangeStream{i8}, (int64_t)size}; },
        [&](WindowStream& src, const TileCall& c, const TileBufs& b, const int64_t*& idx_err) {
            hipError_t e = stream_with_index(i8, in_nbytes, cb, p, block_offsets, b.idx, s, src.st, idx_err);
            if (e != hipSuccess || c.Mg <= 0) return e;
            const int P = (int)(c.K * c.G);
            e = dev_fill(b.d.idx_err, 0, (size_t)P * 8, s);
            if (e != hipSuccess) return e;
            return launch_range_worklist(src.st, b.segs, b.pcs, P, P, 0, c.Mg, b.d.offs, s);
        });
}
}  // namespace

int64_t bshuf_decompress_lz4_tiles_dev(const void* in, size_t in_nbytes, size_t size, size_t elem_size,
                                       size_t block_size, const int64_t* d_starts, size_t ntiles, size_t rows,
                                       size_t cols, size_t pitch, void* out, void* ws, size_t ws_bytes,
                                       int64_t* d_result, int64_t* d_status, const uint64_t* block_offsets,
                                       void* stream) {
    return tiles_dev(in, in_nbytes, size, elem_size, block_size, d_starts, ntiles, rows, cols, pitch, out, ws,
                     ws_bytes, d_result, d_status, block_offsets, stream, nullptr);
}

int64_t bshuf_decompress_lz4_tiles_cvt_dev(const void* in, size_t in_nbytes, size_t size, size_t elem_size,
                                           size_t block_size, const int64_t* d_starts, size_t ntiles,
                                           size_t rows, size_t cols, size_t pitch, void* out, void* ws,
                                           size_t ws_bytes, int64_t* d_result, int64_t* d_status,
                                           const uint64_t* block_offsets, void* stream, const bshuf_cvt* cvt) {
    CvtArgs a;
    const int64_t r = cvt_check(cvt, elem_size, out, a);
    if (r) return r;
    return tiles_dev(in, in_nbytes, size, elem_size, block_size, d_starts, ntiles, rows, cols, pitch, out, ws,
                     ws_bytes, d_result, d_status, block_offsets, stream, &a);
}

size_t bshuf_decompress_lz4_tiles_set_dev_workspace(size_t max_size, size_t elem_size, size_t block_size,
                                                    size_t ntiles, size_t rows, size_t cols, size_t pitch) {
    Plan p;
    TileShapeH w;
    if (make_plan(max_size, elem_size, block_size, p) ||
        tile_shape_host(p, max_size, 0, ntiles, rows, cols, pitch, true, w))
        return 0;
    return tile_ws(p, w, 0, nullptr, nullptr);
}

namespace {
int64_t tiles_set_dev(const void* d_set, size_t count, size_t max_size, size_t elem_size, size_t block_size,
                      const int64_t* d_ids, const int64_t* d_starts, size_t ntiles, size_t rows, size_t cols,
                      size_t pitch, void* out, void* ws, size_t ws_bytes, int64_t* d_result, int64_t* d_status,
                      void* stream, const CvtArgs* cvt) {
    Plan p;
    int64_t r = make_plan(max_size, elem_size, block_size, p);
    if (r) return r;
    TileShapeH w;
    r = tile_shape_host(p, max_size, 0, ntiles, rows, cols, pitch, true, w);
    if (r) return r;
    if (count > (size_t)INT32_MAX) return kErrUnsupported;
    const size_t need = tile_ws(p, w, 0, nullptr, nullptr);
    if (ws && (ws_bytes < need || ((uintptr_t)ws & 255))) return kErrUnsupported;
    if (!d_set || ((uintptr_t)d_set & 255)) return kErrUnsupported;
    if (!have_device()) return kErrHip;
    hipStream_t s = (hipStream_t)stream;
    if (w.empty) return dev_fill(d_result, 0, sizeof(int64_t), s) == hipSuccess ? 0 : kErrHip;
    return tile_decode(
        p, w, 0, need, d_starts, out, ws, ws_bytes, d_result, d_status, s, cvt,
        [&](const TileBufs& b) {
            return WindowSet{(const StreamSetHeader*)d_set,
                             (const StreamSetRec*)((const uint8_t*)d_set + kStreamSetRecs),
                             d_ids,
                             b.sidx,
                             (int64_t)count,
                             p.nb};
        },
        // (the set's indexes were made by its build: nothing to rebuild)
        [&](const WindowSet& src, const TileCall& c, const TileBufs& b, const int64_t*&) {
            if (c.Mg <= 0) return hipSuccess;
            const int64_t P = (int64_t)c.K * c.G;
            const hipError_t e = dev_fill(b.d.idx_err, 0, (size_t)P * 8, s);
            if (e != hipSuccess) return e;
            // the window decode's work list, a group being its window
            WindowCall wc{};
            wc.K = (int32_t)P;
            wc.Mw = c.Mg;
            return launch_window_set_worklist(src, wc, b.segs, b.pcs, b.d.offs, s);
        });
}
}  // namespace

int64_t bshuf_decompress_lz4_tiles_set_dev(const void* d_set, size_t count, size_t max_size, size_t elem_size,
                                           size_t block_size, const int64_t* d_ids, const int64_t* d_starts,
                                           size_t ntiles, size_t rows, size_t cols, size_t pitch, void* out,
                                           void* ws, size_t ws_bytes, int64_t* d_result, int64_t* d_status,
                                           void* stream) {
    return tiles_set_dev(d_set, count, max_size, elem_size, block_size, d_ids, d_starts, ntiles, rows, cols, pitch,
                         out, ws, ws_bytes, d_result, d_status, stream, nullptr);
}

int64_t bshuf_decompress_lz4_tiles_set_cvt_dev(const void* d_set, size_t count, size_t max_size, size_t elem_size,
                                               size_t block_size, const int64_t* d_ids, const int64_t* d_starts,
                                               size_t ntiles, size_t rows, size_t cols, size_t pitch, void* out,
                                               void* ws, size_t ws_bytes, int64_t* d_result, int64_t* d_status,
                                               void* stream, const bshuf_cvt* cvt) {
    CvtArgs a;
    const int64_t r = cvt_check(cvt, elem_size, out, a);
    if (r) return r;
    return tiles_set_dev(d_set, count, max_size, elem_size, block_size, d_ids, d_starts, ntiles, rows, cols, pitch,
                         out, ws, ws_bytes, d_result, d_status, stream, &a);
}

int64_t bshuf_synth_fill_dev(void* out, size_t n_elem, int gen, uint64_t first, uint64_t seed,
                             void* stream) {
    if (gen < 0 || gen > 2) return kErrUnsupported;
    if (!have_device()) return kErrHip;
    return launch_synth(out, n_elem, gen, first, seed, (hipStream_t)stream) == hipSuccess
               ? 0
               : kErrHip;
}

}  // extern "C"
