// Host build of the decoder's scan state machine (lz4_scan.h), of the
// ticket-stealing arithmetic (ticket_steal.h), of the pipelined encode's
// segment bounds (pipe_segments.h), of the range decode's piece plan
// (range_plan.h) and of the window decode's plan (window_plan.h) for the CPU
// test suite.  Not part of the product library.
#include <stdint.h>

#include "inplace.h"
#include "lz4_scan.h"
#include "pipe_segments.h"
#include "range_plan.h"
#include "ticket_steal.h"
#include "window_plan.h"

namespace {
struct HostReader {
    const uint8_t* P;
    uint32_t operator()(int p) const { return P[p]; }
};
struct HostOut {
    uint32_t* pos;
    int mx = -(1 << 20);  // max over sequences of (output start - token position), as SeqOut
    void put(int i, uint32_t v, int op) {
        pos[i] = v;
        mx = mx > op - (int)v ? mx : op - (int)v;
    }
};
}  // namespace

extern "C" int bshuf_hostcheck_scan(const uint8_t* payload, int clen, int n, uint32_t* pos,
                                    int* nseq) {
    HostReader rd{payload};
    HostOut out{pos};
    int cnt = 0;
    const int r = bshuf::scan_block(rd, clen, n, out, cnt);
    *nseq = cnt;
    return r;
}

// ... and the in-place decoder's margin value of the block, as k_seq_scan packs
// it into its verdict and k_lz4_decode unpacks it (inplace.h)
extern "C" int bshuf_hostcheck_scan_mx(const uint8_t* payload, int clen, int n, uint32_t* pos,
                                       int* nseq, int* mx_raw, int* mx_seen) {
    HostReader rd{payload};
    HostOut out{pos};
    int cnt = 0;
    const int r = bshuf::scan_block(rd, clen, n, out, cnt);
    *nseq = cnt;
    *mx_raw = out.mx;
    *mx_seen = bshuf::inplace_mx_unpack(bshuf::inplace_mx_pack(out.mx));
    return r;
}

// inplace.h as the launcher and the kernel use it: a span of span_bytes that
// starts `shift` bytes into a 16-byte granule, in the buffer of a block with
// cap reserved bytes.  Returns whether the block is decoded in place.
extern "C" int bshuf_hostcheck_inplace(int cap, int shift, int span_bytes, int mx, int* ip_end,
                                       int* span_off) {
    *ip_end = bshuf::inplace_end(cap);
    *span_off = bshuf::inplace_span_off(*ip_end, bshuf::span_granules(shift, span_bytes));
    return bshuf::inplace_fits(mx, *span_off, shift) ? 1 : 0;
}

// pipe_segments.h as the launcher uses it
extern "C" int bshuf_hostcheck_pipe_schedules(void) { return bshuf::kPipeSchedules; }
extern "C" int bshuf_hostcheck_pipe_segs_max(void) { return bshuf::kPipeSegsMax; }
extern "C" int bshuf_hostcheck_pipe_seg_count(int schedule) { return bshuf::pipe_seg_count(schedule); }
extern "C" int64_t bshuf_hostcheck_pipe_seg_bound(int64_t nb, int schedule, int i) {
    return bshuf::pipe_seg_bound(nb, schedule, i);
}

// ticket_steal.h as the kernels use it
extern "C" int bshuf_hostcheck_ticket_shards(void) { return bshuf::kTicketShards; }
extern "C" int64_t bshuf_hostcheck_ticket_limit(int64_t first, int64_t G, int64_t end, int shard) {
    return bshuf::ticket_limit(first, G, end, shard);
}
extern "C" uint32_t bshuf_hostcheck_ticket_remaining(int64_t limit, uint32_t drawn) {
    return bshuf::ticket_remaining(limit, drawn);
}
// remaining: kTicketShards words
extern "C" int bshuf_hostcheck_ticket_victim(const uint32_t* remaining, int own) {
    uint32_t r[bshuf::kTicketShards];
    for (int c = 0; c < bshuf::kTicketShards; c++) r[c] = remaining[c];
    return bshuf::ticket_victim(r, own);
}

// range_plan.h as the range decode uses it.  out[14]: interior b0, b1, dst;
// head edge blk, lo, hi, dst; tail edge blk, lo, hi, dst; tail span lo, n, dst
// (dst: byte offsets of the dense output, the range's own being dst0).
extern "C" void bshuf_hostcheck_range_pieces(int64_t size, int64_t bs, int64_t E, int64_t start,
                                             int64_t count, int64_t dst0, int64_t* out) {
    bshuf::RangePieces r;
    bshuf::range_pieces(size, bs, E, start, count, dst0, r);
    const int64_t v[14] = {r.b0,      r.b1,      r.int_dst, r.head.blk, r.head.lo, r.head.hi, r.head.dst,
                           r.tail.blk, r.tail.lo, r.tail.hi, r.tail.dst, r.tail_lo, r.tail_n,  r.tail_dst};
    for (int i = 0; i < 14; i++) out[i] = v[i];
}
// ... for n ranges at once (out: 14 words each)
extern "C" void bshuf_hostcheck_range_pieces_n(int64_t size, int64_t bs, int64_t E, const int64_t* starts,
                                               const int64_t* counts, const int64_t* dst0, int64_t n,
                                               int64_t* out) {
    for (int64_t i = 0; i < n; i++)
        bshuf_hostcheck_range_pieces(size, bs, E, starts[i], counts[i], dst0[i], out + 14 * i);
}

// window_plan.h as the window decode uses it, for n (window, start) pairs of
// one stream.  out, 12 words each: Mw, b0, nfull, last, bad, clip_lo, clip_n,
// tail_lo, tail_n (bytes), t0, t1, 0.
extern "C" void bshuf_hostcheck_window_plan(int64_t size, int64_t bs, int64_t E, const int64_t* windows,
                                            const int64_t* starts, int64_t n, int64_t* out) {
    for (int64_t i = 0; i < n; i++) {
        bshuf::WindowPlan w;
        bshuf::window_plan(size, bs, E, windows[i], starts[i], w);
        const int64_t v[12] = {bshuf::window_blocks(size, bs, windows[i]), w.b0, w.nfull, w.last, w.bad,
                               w.clip_lo, w.clip_n, w.tail_lo, w.tail_n, w.t0, w.t1, 0};
        for (int j = 0; j < 12; j++) out[12 * i + j] = v[j];
    }
}

// ... and the plan of windows over a set of `count` streams of sizes[] as
// k_window_set_plan runs it: n (id, window, start) triples, every one with Mw
// forced.  out as above (word 0: Mw as given).
extern "C" void bshuf_hostcheck_window_set_plan(int64_t count, const int64_t* sizes, int64_t bs, int64_t E,
                                                int64_t Mw, const int64_t* ids, const int64_t* windows,
                                                const int64_t* starts, int64_t n, int64_t* out) {
    for (int64_t i = 0; i < n; i++) {
        bshuf::WindowPlan w;
        const int64_t size = ids[i] >= 0 && ids[i] < count ? sizes[ids[i]] : 0;
        bshuf::window_set_plan(count, ids[i], size, bs, E, windows[i], starts[i], Mw, w);
        const int64_t v[12] = {Mw, w.b0, w.nfull, w.last, w.bad, w.clip_lo, w.clip_n, w.tail_lo, w.tail_n,
                               w.t0, w.t1, 0};
        for (int j = 0; j < 12; j++) out[12 * i + j] = v[j];
    }
}
