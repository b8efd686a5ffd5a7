// window_copy.h -- the copy of one window out of its staging area and its
// stream's verbatim tail, by the window decode of one stream and of a set of
// streams (k_window_gather, lz4_window.hip) and by the ragged one
// (k_ragged_gather, lz4_ragged.hip); and the table entries of one window that
// their plan kernels write.
#pragma once

#include "launch.h"
#include "range_worklist.h"
#include "window_plan.h"

namespace bshuf {

// 16 bytes of dst from two aligned 16-byte granules of a source that lies
// 4 * D + sh bytes behind an aligned address.
template <int D>
__device__ __forceinline__ u32x4 shifted(const u32x4 a, const u32x4 b, uint32_t sh) {
    const uint32_t w[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    return u32x4{__builtin_amdgcn_alignbyte(w[D + 1], w[D], sh), __builtin_amdgcn_alignbyte(w[D + 2], w[D + 1], sh),
                 __builtin_amdgcn_alignbyte(w[D + 3], w[D + 2], sh), __builtin_amdgcn_alignbyte(w[D + 4], w[D + 3], sh)};
}

template <int D>
__device__ __forceinline__ void copy_shifted(const gbl128c* q, gbl128* d16, int64_t nv, uint32_t sh, int t,
                                             int T) {
    for (int64_t i = t; i < nv; i += T) d16[i] = shifted<D>(q[i], q[i + 1], sh);
}

// n bytes src -> dst by lanes t of T.  dst is written in whole 16-byte chunks
// between its first and last 16-byte boundary (the bytes before and behind
// singly), and nothing outside [0, n) of it.  The source: 16-byte loads when it
// is congruent to dst mod 16; else every chunk from the two aligned granules
// that hold its bytes -- a granule holds at least one byte of [0, n), so a read
// never leaves the pages of the source.  Fewer than 32 bytes go singly.
__device__ __forceinline__ void span_copy(const uint8_t* src, uint8_t* dst, int64_t n, int t, int T) {
    const gbl8c* s8 = (const gbl8c*)src;
    gbl8* d8 = (gbl8*)dst;
    if (n < 32) {
        for (int64_t i = t; i < n; i += T) d8[i] = s8[i];
        return;
    }
    const int64_t head = (int64_t)((16 - ((uintptr_t)dst & 15)) & 15);
    const int64_t nv = (n - head) >> 4;
    if (t < head) d8[t] = s8[t];
    gbl128* d16 = (gbl128*)(dst + head);
    const uint32_t r = (uint32_t)((uintptr_t)(src + head) & 15);
    if (r == 0) {
        const gbl128c* s16 = (const gbl128c*)(src + head);
        for (int64_t i = t; i < nv; i += T) d16[i] = s16[i];
    } else {
        const gbl128c* q = g128_aligned_down(src + head);
        switch (r >> 2) {
            case 0: copy_shifted<0>(q, d16, nv, r & 3, t, T); break;
            case 1: copy_shifted<1>(q, d16, nv, r & 3, t, T); break;
            case 2: copy_shifted<2>(q, d16, nv, r & 3, t, T); break;
            default: copy_shifted<3>(q, d16, nv, r & 3, t, T); break;
        }
    }
    for (int64_t i = head + 16 * nv + t; i < n; i += T) d8[i] = s8[i];
}

// Window i's Seg (Mw consecutive blocks of the stream at `in`, decoded back to
// back into staging area i), its piece (the clip of that area, which goes to
// dst) and its tail span.
__device__ __forceinline__ void write_window(const WindowCall& c, int i, const WindowPlan& w, const uint8_t* in,
                                             uint8_t* dst, Seg* __restrict__ segs, RangePiece* __restrict__ pcs,
                                             WindowTail* __restrict__ wt) {
    uint8_t* slot = c.slots + (int64_t)i * c.slot;
    Seg g;
    g.in = in;
    g.out = slot;
    g.first = (int64_t)i * c.Mw;
    g.nfull = w.nfull;
    g.tail = 0;
    g.in_nbytes = 0;  // the work list: the end of the window's last record
    g.chunk0 = 0;
    g.nchunks = 0;
    g.seq0 = 0;       // the work list
    g.result = c.res + i;
    g.last = w.last;
    g.pad_ = 0;
    segs[i] = g;
    RangePiece pc;
    pc.b0 = w.b0;
    pc.nblk = c.Mw;
    pc.seq_base = c.seq_words < 0 ? -1 : (int64_t)i * c.seq_words;
    pc.src = slot + w.clip_lo;
    pc.dst = dst;
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

// For the gather: window i's stream and that stream's error word.
__device__ __forceinline__ RangeStream source_stream(const WindowStream& src, const WindowTail&, int,
                                                     int64_t& err) {
    err = 0;
    return src.st;
}

__device__ __forceinline__ RangeStream source_stream(const WindowSet& src, const WindowTail& w, int i,
                                                     int64_t& err) {
    err = 0;
    if (w.bad) return RangeStream{};
    const StreamSetRec r = src.recs[src.sidx[i]];
    err = r.err;
    return r.st;
}

// Window i of a call by lanes t of T; st is the window's stream and err that
// stream's error word (0, or -91 from a set whose rebuilt index found that the
// records do not tile it).  The window's status: -71 when it is bad; else err;
// else the code of the highest failing block among those that hold clip bytes
// (res: the Seg's result says whether any of its Mw blocks failed; bst: the
// per-block status of the window's Mw work blocks); else -91 when the window
// reaches the verbatim tail and that tail is not inside the stream
// (tail_start); else its byte count wbytes, and only then is it copied.
__device__ __forceinline__ void window_gather_one(const RangeStream& st, int64_t err, const WindowTail& w,
                                                  const RangePiece* __restrict__ pcs, int i, int64_t res,
                                                  const int64_t* __restrict__ bst, int64_t wbytes,
                                                  int64_t* __restrict__ wstat, int t, int T) {
    int64_t code = 0;
    const uint8_t* tsrc = nullptr;
    if (w.bad) {
        code = -71;
    } else if (err) {
        code = err;
    } else {
        if (w.t1 > w.t0 && res < 0) {
            for (int j = w.t0; j < w.t1; j++)
                if (bst[j] < 0) code = bst[j];
        }
        if (code == 0 && w.n > 0) {
            uint64_t ts;
            if (tail_start(st, ts))
                tsrc = st.in + ts + w.lo;
            else
                code = -91;
        }
    }
    if (t == 0) wstat[i] = code ? code : wbytes;
    if (code) return;
    const RangePiece pc = pcs[i];
    if (pc.n > 0) span_copy(pc.src, pc.dst, pc.n, t, T);
    if (w.n > 0) span_copy(tsrc, pc.dst + pc.n, w.n, t, T);
}

}  // namespace bshuf
