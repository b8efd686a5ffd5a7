// Host build of the decoder's scan state machine (lz4_scan.h), of the
// ticket-stealing arithmetic (ticket_steal.h), of the pipelined encode's
// segment bounds (pipe_segments.h), of the range decode's piece plan
// (range_plan.h), of the window decode's plan (window_plan.h), of the tile
// decode's shape and plan (tile_plan.h), of the converting gathers' span cut
// (cvt_span.h) and of the launchers' path decisions (dispatch.h) for the CPU
// test suite.  Not part of the product library.
#include <stdint.h>

#include "cvt_span.h"
#include "dispatch.h"
#include "inplace.h"
#include "lz4_scan.h"
#include "pipe_segments.h"
#include "range_plan.h"
#include "ticket_steal.h"
#include "tile_plan.h"
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

// ... and the plan of ragged windows as k_ragged_plan runs it: n (id, count,
// start) triples with Mw forced.  nstreams < 0: every window in ONE stream of
// sizes[0] elements (ids unused); else in stream id of a set of nstreams streams
// of sizes[], an id outside it being refused.  out as above; word 11: the
// elements the window takes in the packed output (its count, 0 when refused).
extern "C" void bshuf_hostcheck_ragged_plan(int64_t nstreams, const int64_t* sizes, int64_t bs, int64_t E,
                                            int64_t max_window, int64_t Mw, const int64_t* ids,
                                            const int64_t* counts, const int64_t* starts, int64_t n,
                                            int64_t* out) {
    for (int64_t i = 0; i < n; i++) {
        bshuf::WindowPlan w;
        const bool known = nstreams < 0 || (ids[i] >= 0 && ids[i] < nstreams);
        const int64_t size = known ? sizes[nstreams < 0 ? 0 : ids[i]] : 0;
        bshuf::ragged_plan(size, bs, E, max_window, counts[i], starts[i], Mw, !known, w);
        const int64_t v[12] = {Mw, w.b0, w.nfull, w.last, w.bad, w.clip_lo, w.clip_n, w.tail_lo, w.tail_n,
                               w.t0, w.t1, w.bad ? 0 : counts[i]};
        for (int j = 0; j < 12; j++) out[12 * i + j] = v[j];
    }
}

// tile_plan.h as the tile decode's host side uses it.  out[3]: rg, G, Mg.
extern "C" void bshuf_hostcheck_tile_shape(int64_t rows, int64_t cols, int64_t pitch, int64_t bs, int64_t nb,
                                           int64_t* out) {
    bshuf::TileShape t;
    bshuf::tile_shape(rows, cols, pitch, bs, nb, t);
    out[0] = t.rg;
    out[1] = t.G;
    out[2] = t.Mg;
}

// ... and one tile as k_tile_plan and k_tile_gather run it, with the shape
// tile_shape gives for nb blocks.  count < 0: the tile at `start` of ONE stream
// of sizes[0] elements.  Else: of stream `id` of a set of `count` streams of
// sizes[], whose stream `ref` (-1: none) serves a bad tile.  groups, 6 words per
// group: the stream its blocks come from (0 for one stream, -1: none), b0,
// nfull, last, bad, 0.  rowsout, 8 words per row (all 0 for a bad tile): g, lo, n,
// tail_lo, tail_n (bytes), t0, t1, 0.  Returns the tile's bad flag.
extern "C" int bshuf_hostcheck_tile_rows(int64_t count, const int64_t* sizes, int64_t id, int64_t ref,
                                         int64_t bs, int64_t E, int64_t rows, int64_t cols, int64_t pitch,
                                         int64_t nb, int64_t start, int64_t* groups, int64_t* rowsout) {
    bshuf::TileShape t;
    bshuf::tile_shape(rows, cols, pitch, bs, nb, t);
    const int64_t span = (rows - 1) * pitch + cols;
    const bool set = count >= 0;
    const bool known = !set || (id >= 0 && id < count);
    const int64_t size = known ? sizes[set ? id : 0] : 0;
    const bool bad = set ? bshuf::tile_set_bad(count, id, size, bs, span, start, t.Mg)
                         : bshuf::tile_bad(size, span, start);
    int64_t s = set ? id : 0;
    if (set && bad) s = ref >= 0 && ref < count ? ref : -1;
    for (int64_t g = 0; g < t.G; g++) {
        bshuf::WindowPlan w{};
        w.nfull = t.Mg;
        w.bad = 1;
        if (s >= 0) bshuf::tile_group(sizes[s], bs, E, rows, cols, pitch, t, start, g, bad, w);
        const int64_t v[6] = {s, w.b0, w.nfull, w.last, w.bad, 0};
        for (int j = 0; j < 6; j++) groups[6 * g + j] = v[j];
    }
    for (int64_t r = 0; r < rows; r++) {
        bshuf::TileRow o{};
        if (!bad) bshuf::tile_row(bshuf::tile_covered(size, bs), bs, E, cols, pitch, t.rg, start, r, groups[6 * (r / t.rg) + 1], o);
        const int64_t v[8] = {o.g, o.lo, o.n, o.tail_lo, o.tail_n, o.t0, o.t1, 0};
        for (int j = 0; j < 8; j++) rowsout[8 * r + j] = v[j];
    }
    return bad ? 1 : 0;
}

// cvt_span.h as span_cvt (window_copy.h) uses it: a span of n elements of S
// bytes whose source starts at byte address src and whose destination, of D-byte
// elements, at dst (only their low 4 bits matter).  out[6]: head, nu, nc, tail,
// ue, r.
extern "C" void bshuf_hostcheck_cvt_span(uint32_t src, uint32_t dst, int S, int D, int64_t n, int64_t* out) {
    bshuf::CvtSpan p;
    bshuf::cvt_span_plan(src, dst, S, D, n, p);
    const int64_t v[6] = {p.head, p.nu, p.nc, p.tail, p.ue, p.r};
    for (int i = 0; i < 6; i++) out[i] = v[i];
}

// dispatch.h as the launchers use it.  The constants, out[14]: kTableBytes,
// kRawBytes, kStageRegBytes, kFastMaxBlockBytes, kU16TableLimit,
// max_device_block_bytes, max_lds_encode_bytes, max_lds_decode_bytes, kDataPad,
// kDescBytes, kLdsBytes, kTileGroups, kSregWords, kInPlaceMargin.
extern "C" void bshuf_hostcheck_dispatch_consts(int64_t* out) {
    const int64_t v[14] = {bshuf::kTableBytes,
                           bshuf::kRawBytes,
                           bshuf::kStageRegBytes,
                           bshuf::kFastMaxBlockBytes,
                           bshuf::kU16TableLimit,
                           bshuf::max_device_block_bytes(),
                           bshuf::max_lds_encode_bytes(),
                           bshuf::max_lds_decode_bytes(),
                           bshuf::kDataPad,
                           bshuf::kDescBytes,
                           bshuf::kLdsBytes,
                           bshuf::kTileGroups,
                           bshuf::kSregWords,
                           bshuf::kInPlaceMargin};
    for (int i = 0; i < 14; i++) out[i] = v[i];
}
// groups the encoders' prefetch registers hold (four: the 4-groups-per-lane form)
extern "C" int bshuf_hostcheck_dispatch_reg_groups(int ek, int four) {
    return four ? bshuf::enc_reg_groups4(ek) : bshuf::enc_reg_groups(ek);
}
// launch_encode (n = 1) / launch_encode_batch over sources at these addresses
// (only their low bits matter), blocks of block_bytes and a partial block of
// last_bytes (0: none).  out[10]: ek, raw8, desc, wide, wide_last, large,
// LDS bytes, desc_off, fast applies, fast's SREG layout.
extern "C" void bshuf_hostcheck_dispatch_encode(int E, int64_t block_bytes, int64_t last_bytes,
                                                const int64_t* addrs, int n, int64_t* out) {
    bshuf::Align al;
    for (int i = 0; i < n; i++) al.add((uintptr_t)addrs[i]);
    const int ek = bshuf::pick_ek(E, al.a16);
    const int64_t v[10] = {ek,
                           bshuf::enc_raw8(E, al.a8),
                           bshuf::enc_desc(block_bytes),
                           bshuf::enc_wide(block_bytes),
                           last_bytes && bshuf::enc_wide(last_bytes),
                           block_bytes > bshuf::max_lds_encode_bytes(),
                           (int64_t)bshuf::enc_lds_bytes(block_bytes),
                           bshuf::enc_desc_off(block_bytes),
                           bshuf::fast_applies(block_bytes),
                           bshuf::fast_sreg(ek, block_bytes)};
    for (int i = 0; i < 10; i++) out[i] = v[i];
}
// launch_decode (n = 1) / launch_decode_batch with outputs at these addresses.
// out[5]: large, ek, stage_off (0 byte stores, -1 registers, else the LDS
// offset), LDS bytes of a workgroup, cap.
extern "C" void bshuf_hostcheck_dispatch_decode(int E, int64_t block_bytes, const int64_t* addrs, int n,
                                                int inplace, int grec, int64_t* out) {
    bshuf::Align al;
    for (int i = 0; i < n; i++) al.add((uintptr_t)addrs[i]);
    const int ek = bshuf::pick_ek(E, al.a16);
    const int32_t cap = bshuf::dec_cap(block_bytes);
    size_t lds = bshuf::dec_lds_bytes(cap, (uint32_t)bshuf::lz4_bound((int)block_bytes), inplace != 0, grec != 0);
    const int32_t so = bshuf::dec_stage_off(ek, E, block_bytes, cap, al.a8, lds);
    const int64_t v[5] = {block_bytes > bshuf::max_lds_decode_bytes(), ek, so, (int64_t)lds, cap};
    for (int i = 0; i < 5; i++) out[i] = v[i];
}
// ... both for every residue 0..15 of one pointer (out: 16 x 15 words, the
// encoder's 10 then the decoder's 5) ...
extern "C" void bshuf_hostcheck_dispatch_residues(int E, int64_t block_bytes, int64_t last_bytes, int inplace,
                                                  int grec, int64_t* out) {
    for (int r = 0; r < 16; r++) {
        const int64_t a = 0x10000 + r;
        bshuf_hostcheck_dispatch_encode(E, block_bytes, last_bytes, &a, 1, out + 15 * r);
        bshuf_hostcheck_dispatch_decode(E, block_bytes, &a, 1, inplace, grec, out + 15 * r + 10);
    }
}
// ... and for every pair of residues of a batch of two (out: 256 x 15 words)
extern "C" void bshuf_hostcheck_dispatch_pairs(int E, int64_t block_bytes, int64_t* out) {
    for (int r = 0; r < 256; r++) {
        const int64_t a[2] = {0x10000 + r / 16, 0x20000 + r % 16};
        bshuf_hostcheck_dispatch_encode(E, block_bytes, 0, a, 2, out + 15 * r);
        bshuf_hostcheck_dispatch_decode(E, block_bytes, a, 2, 1, 0, out + 15 * r + 10);
    }
}
// launch_transpose: the tile kernels (1) or the byte-granular one (0) ...
extern "C" int bshuf_hostcheck_dispatch_transpose(int E, int64_t in_addr, int64_t out_addr) {
    bshuf::Align al;
    al.add((uintptr_t)in_addr);
    al.add((uintptr_t)out_addr);
    return bshuf::transpose_fast(E, al.a16) ? 1 : 0;
}
// ... and a tile of ng groups of a block of P: 16-byte rows (1) or bytes (0)
extern "C" int bshuf_hostcheck_dispatch_rows16(int P, int ng) { return bshuf::transpose_rows16(P, ng) ? 1 : 0; }
