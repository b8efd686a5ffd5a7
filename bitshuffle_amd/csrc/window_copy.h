// window_copy.h -- the copy of one window out of its staging area and its
// stream's verbatim tail, by the window decode of one stream and of a set of
// streams (k_window_gather, lz4_window.hip) and by the ragged one
// (k_ragged_gather, lz4_ragged.hip); and the table entries of one window that
// their plan kernels write.  Next to the copy, the converting span of the
// *_cvt_dev entries (span_cvt), which the tile gather (lz4_tile.hip) uses too.
#pragma once

#include <type_traits>

#include "cvt_span.h"
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

// ---- the converting span (the *_cvt_dev entries; launch.h, "converting
// gathers") --------------------------------------------------------------
// One element: X as the fp32 nearest to it (F32: itself), then ONE fused
// multiply-add, then the rounding to Y (F32: none) -- plain casts, which the
// compiler turns into v_cvt_f32_*, v_fma_f32 and the round-to-nearest-even
// v_cvt_f16_f32 / v_cvt_pk_bf16_f32.
template <class X>
__device__ __forceinline__ float cvt_word(uint32_t v) {
    if constexpr (std::is_same<X, float>::value)
        return __uint_as_float(v);
    else
        return (float)(X)v;
}
// element k of a unit's words
template <class X>
__device__ __forceinline__ float cvt_elem(const uint32_t* w, int k) {
    if constexpr (sizeof(X) == 1)
        return cvt_word<X>((w[k >> 2] >> (8 * (k & 3))) & 0xffu);
    else if constexpr (sizeof(X) == 2)
        return cvt_word<X>((w[k >> 1] >> (16 * (k & 1))) & 0xffffu);
    else
        return cvt_word<X>(w[k]);
}
// The fp32 fused multiply-add of one element on its way to Y.  For a half
// destination the compiler would fold it into the conversion
// (v_fma_mixlo_f16), which rounds the exact sum ONCE, to half: the empty asm
// keeps the fp32 rounding the semantics ask for (found on the GPU: x * (1/3)
// differed from the twice-rounded reference in about 3 % of int16 values).
template <class Y>
__device__ __forceinline__ float cvt_fma(float x, float scale, float offset) {
    float y = __builtin_fmaf(x, scale, offset);
    if constexpr (std::is_same<Y, _Float16>::value) asm("" : "+v"(y));
    return y;
}
template <class Y>
__device__ __forceinline__ uint32_t cvt_bits16(float y) {
    return (uint32_t)__builtin_bit_cast(uint16_t, (Y)y);
}
// an S-aligned element of a staging area; an element of the verbatim tail, at
// any byte address
template <class X>
__device__ __forceinline__ float cvt_load(const uint8_t* p) {
    return (float)*(const __attribute__((address_space(1))) X*)p;
}
template <class X>
__device__ __forceinline__ float cvt_load_bytes(const uint8_t* p) {
    const gbl8c* b = (const gbl8c*)p;
    uint32_t v = 0;
#pragma unroll
    for (int j = 0; j < (int)sizeof(X); j++) v |= (uint32_t)b[j] << (8 * j);
    return cvt_word<X>(v);
}
template <class Y>
__device__ __forceinline__ void cvt_store(uint8_t* p, float y) {
    *(__attribute__((address_space(1))) Y*)p = (Y)y;
}

// The units of a span (cvt_span.h) by lanes t of T: unit u is granules [u * G,
// u * G + G) behind q when the source is aligned (D < 0), else 4 * D + sh bytes
// into granules [u * G, u * G + G]; its NC chunks of dst are this lane's.
template <class X, class Y, int D>
__device__ __forceinline__ void cvt_units(const gbl128c* q, gbl128* d16, int64_t nu, uint32_t sh, float scale,
                                          float offset, int t, int T) {
    constexpr int S = (int)sizeof(X), DS = (int)sizeof(Y);
    constexpr int UE = 16 / S > 16 / DS ? 16 / S : 16 / DS;
    constexpr int G = UE * S / 16, NC = UE * DS / 16;
    for (int64_t u = t; u < nu; u += T) {
        uint32_t w[4 * G];
        if constexpr (D < 0) {
#pragma unroll
            for (int j = 0; j < G; j++) {
                const u32x4 v = q[u * G + j];
                w[4 * j] = v.x, w[4 * j + 1] = v.y, w[4 * j + 2] = v.z, w[4 * j + 3] = v.w;
            }
        } else {
            u32x4 a[G + 1];
#pragma unroll
            for (int j = 0; j <= G; j++) a[j] = q[u * G + j];
#pragma unroll
            for (int j = 0; j < G; j++) {
                const u32x4 v = shifted<(D < 0 ? 0 : D)>(a[j], a[j + 1], sh);
                w[4 * j] = v.x, w[4 * j + 1] = v.y, w[4 * j + 2] = v.z, w[4 * j + 3] = v.w;
            }
        }
        float y[UE];
#pragma unroll
        for (int k = 0; k < UE; k++) y[k] = cvt_fma<Y>(cvt_elem<X>(w, k), scale, offset);
        uint32_t o[4 * NC];
        if constexpr (DS == 4) {
#pragma unroll
            for (int k = 0; k < UE; k++) o[k] = __float_as_uint(y[k]);
        } else {
#pragma unroll
            for (int k = 0; k < UE / 2; k++) o[k] = cvt_bits16<Y>(y[2 * k]) | (cvt_bits16<Y>(y[2 * k + 1]) << 16);
        }
#pragma unroll
        for (int c = 0; c < NC; c++) d16[u * NC + c] = u32x4{o[4 * c], o[4 * c + 1], o[4 * c + 2], o[4 * c + 3]};
    }
}

// n elements X at src (S-aligned, in a staging area) -> n elements Y at dst
// (aligned to Y) by lanes t of T (T >= 16), y = (Y)fmaf((float)x, scale,
// offset).  The cut is cvt_span_plan's (cvt_span.h): dst is written in whole
// 16-byte chunks between its first and last 16-byte boundary, element by
// element before and behind, nothing outside; every 16-byte granule read holds
// a byte of the span.  Head, rest chunks and tail go to different ends of the
// lanes.
template <class X, class Y>
__device__ __forceinline__ void span_cvt(const uint8_t* src, uint8_t* dst, int64_t n, float scale, float offset,
                                         int t, int T) {
    constexpr int S = (int)sizeof(X), DS = (int)sizeof(Y), EPC = 16 / DS;
    CvtSpan p;
    cvt_span_plan((uint32_t)(uintptr_t)src, (uint32_t)(uintptr_t)dst, S, DS, n, p);
    for (int64_t i = t; i < p.head; i += T)  // (all of a short span: up to 31 elements)
        cvt_store<Y>(dst + i * DS, cvt_fma<Y>(cvt_load<X>(src + i * S), scale, offset));
    if (p.head == n) return;
    const uint8_t* s = src + p.head * S;
    uint8_t* d = dst + p.head * DS;
    gbl128* d16 = (gbl128*)d;
    if (p.r == 0) {
        cvt_units<X, Y, -1>((const gbl128c*)s, d16, p.nu, 0, scale, offset, t, T);
    } else {
        const gbl128c* q = g128_aligned_down(s);
        const uint32_t sh = (uint32_t)p.r & 3;
        switch (p.r >> 2) {
            case 0: cvt_units<X, Y, 0>(q, d16, p.nu, sh, scale, offset, t, T); break;
            case 1: cvt_units<X, Y, 1>(q, d16, p.nu, sh, scale, offset, t, T); break;
            case 2: cvt_units<X, Y, 2>(q, d16, p.nu, sh, scale, offset, t, T); break;
            default: cvt_units<X, Y, 3>(q, d16, p.nu, sh, scale, offset, t, T); break;
        }
    }
    const int tb = T - 1 - t;
    const int64_t e0 = p.nu * p.ue;  // elements behind the head that the units took
    if (tb < p.nc) {
        const int64_t e = e0 + (int64_t)tb * EPC;
        float y[EPC];
#pragma unroll
        for (int k = 0; k < EPC; k++) y[k] = cvt_fma<Y>(cvt_load<X>(s + (e + k) * S), scale, offset);
        uint32_t o[4];
        if constexpr (DS == 4) {
#pragma unroll
            for (int k = 0; k < 4; k++) o[k] = __float_as_uint(y[k]);
        } else {
#pragma unroll
            for (int k = 0; k < 4; k++) o[k] = cvt_bits16<Y>(y[2 * k]) | (cvt_bits16<Y>(y[2 * k + 1]) << 16);
        }
        d16[e / EPC] = u32x4{o[0], o[1], o[2], o[3]};
    }
    const int64_t e1 = e0 + p.nc * EPC;
    const int tm = (t + T / 2) % T;  // (the tail away from the head's and the chunks' lanes)
    if (tm < p.tail)
        cvt_store<Y>(d + (e1 + tm) * DS, cvt_fma<Y>(cvt_load<X>(s + (e1 + tm) * S), scale, offset));
}

// n elements of the verbatim tail (fewer than 8, at any byte address of the
// caller's stream): byte loads, one element per lane.
template <class X, class Y>
__device__ __forceinline__ void tail_cvt(const uint8_t* src, uint8_t* dst, int64_t n, float scale, float offset,
                                         int t, int T) {
    for (int64_t i = t; i < n; i += T)
        cvt_store<Y>(dst + i * sizeof(Y), cvt_fma<Y>(cvt_load_bytes<X>(src + i * sizeof(X)), scale, offset));
}

// What a gather does with the spans it has found: the copy, or a conversion.
// The tables (plan kernels) place every piece as the plain call does, in source
// bytes behind `out`; place() is where the piece goes, behind() the address
// `bytes` source bytes further on.
struct SpanCopy {
    static constexpr int kWide = 1;  // bytes the lane rule counts per source byte
    __device__ __forceinline__ uint8_t* place(uint8_t*, uint8_t* plain) const { return plain; }
    __device__ __forceinline__ uint8_t* behind(uint8_t* d, int64_t bytes) const { return d + bytes; }
    __device__ __forceinline__ void span(const uint8_t* s, uint8_t* d, int64_t bytes, int t, int T) const {
        span_copy(s, d, bytes, t, T);
    }
    __device__ __forceinline__ void tail(const uint8_t* s, uint8_t* d, int64_t bytes, int t, int T) const {
        span_copy(s, d, bytes, t, T);
    }
};
template <class X, class Y>
struct SpanCvt {
    float scale, offset;
    static constexpr int64_t S = sizeof(X), D = sizeof(Y);
    __device__ __forceinline__ uint8_t* place(uint8_t* out, uint8_t* plain) const {
        return out + (plain - out) / S * D;
    }
    __device__ __forceinline__ uint8_t* behind(uint8_t* d, int64_t bytes) const { return d + bytes / S * D; }
    __device__ __forceinline__ void span(const uint8_t* s, uint8_t* d, int64_t bytes, int t, int T) const {
        span_cvt<X, Y>(s, d, bytes / S, scale, offset, t, T);
    }
    __device__ __forceinline__ void tail(const uint8_t* s, uint8_t* d, int64_t bytes, int t, int T) const {
        tail_cvt<X, Y>(s, d, bytes / S, scale, offset, t, T);
    }
};

// f(SpanCvt<X, Y>) for the kinds of a checked CvtArgs (api.hip, cvt_check).
template <class F>
inline void cvt_dispatch(const CvtArgs& a, F&& f) {
    auto to = [&](auto x) {
        using X = decltype(x);
        if (a.dst == kCvtDstF32) f(SpanCvt<X, float>{a.scale, a.offset});
        if (a.dst == kCvtDstF16) f(SpanCvt<X, _Float16>{a.scale, a.offset});
        if (a.dst == kCvtDstBF16) f(SpanCvt<X, __bf16>{a.scale, a.offset});
    };
    switch (a.src) {
        case kCvtU8: to(uint8_t{}); break;
        case kCvtI8: to(int8_t{}); break;
        case kCvtU16: to(uint16_t{}); break;
        case kCvtI16: to(int16_t{}); break;
        case kCvtU32: to(uint32_t{}); break;
        case kCvtI32: to(int32_t{}); break;
        default: to(float{}); break;
    }
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
// (tail_start); else its byte count wbytes (source bytes), and only then is it
// copied -- or converted: op (SpanCopy, SpanCvt), out the call's output.
template <class Op>
__device__ __forceinline__ void window_gather_one(const RangeStream& st, int64_t err, const WindowTail& w,
                                                  const RangePiece* __restrict__ pcs, int i, int64_t res,
                                                  const int64_t* __restrict__ bst, int64_t wbytes,
                                                  int64_t* __restrict__ wstat, int t, int T, const Op& op,
                                                  uint8_t* out) {
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
    uint8_t* dst = op.place(out, pc.dst);
    if (pc.n > 0) op.span(pc.src, dst, pc.n, t, T);
    if (w.n > 0) op.tail(tsrc, op.behind(dst, pc.n), w.n, t, T);
}

}  // namespace bshuf
