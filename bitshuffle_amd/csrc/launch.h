// launch.h -- host-side launchers for the gfx950 kernels (internal to the .so).
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <algorithm>

#include "bshuf_dev.h"
#include "pipe_segments.h"

namespace bshuf {

// Per-kernel event timing (prof.hip); a no-op unless bshuf_prof_enable(1).
bool prof_on();
class ProfScope {
  public:
    ProfScope(const char* name, hipStream_t s);
    ~ProfScope();

  private:
    const char* name_;
    hipStream_t s_;
    void* a_;
};

// Kernel-variant knob for A/B measurements (bshuf_set_variant, per thread,
// byte-identical variants only); 0 = default.  The kNoPipe, kNoOverlap,
// kAltSegments, kWideCompact, kStaticSched, kTicketSched and kNoSteal bits are not part of
// the variant (pipe_ctx / pipe_overlap / pipe_schedule / ticket_sched /
// ticket_steal read them).
int tuning_variant();
#ifdef BSHUF_DIAG
int diag_variant();  // timing ablations (wrong output), diag build only
#endif

// Pipelined encode.  A long encode runs as several launches of the parse
// kernel (the segments of pipe_segments.h), and each segment's offset scan +
// compaction on a per-thread side stream as soon as that segment is parsed, so
// the HBM-bound compaction overlaps the next segment's (LDS- and latency-bound)
// parse.  The parse launches alternate between the caller's stream (even
// segments) and a second per-thread stream `par` (odd ones): launch i + 1 is
// ordered only behind launch i - 1, so its workgroups wait in the dispatcher
// and take each LDS slot the moment a wave of launch i exits, instead of the
// whole launch waiting for the last wave of launch i and a launch gap.  At
// most two parse launches are in flight.  Segments share nothing but the
// read-only input: blocks, scratch slots, foot entries and ticket sets are
// their own, and all ordering is by events (no kernel waits on memory another
// running kernel writes).  With two launches in flight no CU drains between
// segments, so everything on the side stream is single-wave workgroups of few
// registers, which the dispatcher places beside six resident parse waves: the
// segment-local scan k_seg_sums + k_seg_scan and the compaction
// k_compact_t<1, 2> (lz4_encode.hip).  pipe_ctx(s) returns the calling thread's streams on
// the current device and their fork / join events, or nullptr: pipelining off
// (bshuf_set_variant bit kNoPipe), `s` being captured into a graph, or a
// stream or event that could not be created.  Every fork is joined back into
// `s` before the call returns, also after an error, so callers see one
// stream-ordered operation as before.  With bit kNoOverlap, and while
// per-kernel timing is on (prof_on(): an event pair around a launch queued
// behind another would time the queueing too), every parse runs on `s`, one
// after the other.
constexpr int kPipeSegs = kPipeSegsMax;    // segments of the longest schedule
constexpr int64_t kPipeMinBlocks = 65536;  // shorter calls run unsegmented
constexpr int kPipeEvents = kPipeSegs + 3;  // fork, one per segment, par's join, side's join
constexpr int kNoPipe = 1 << 20;  // no pipelined encode
constexpr int kNoOverlap = 1 << 27;  // pipelined encode with every parse on the caller's stream
constexpr int kAltSegments = 1 << 28;  // the segment schedule that is not the default (A/B)
constexpr int kWideCompact = 1 << 29;  // side-stream compaction by the 256-thread k_compact (A/B)
constexpr int kPipeScheduleDefault = kPipeEqual;
struct PipeCtx {
    hipStream_t side = nullptr;
    hipStream_t par = nullptr;
    hipEvent_t ev[kPipeEvents] = {};
};
PipeCtx* pipe_ctx(hipStream_t s);
bool pipe_overlap();   // parse launches on two streams (not kNoOverlap, not prof_on())
int pipe_schedule();   // PipeSchedule of the calling thread
bool pipe_slim_compact();  // side-stream compaction by k_compact_t<1, 2> (not kWideCompact)
// s waits for everything enqueued on `from` so far (event ev)
hipError_t stream_after(hipStream_t s, hipStream_t from, hipEvent_t ev);

// Dynamic block scheduling of the persistent kernels (k_lz4_encode,
// k_lz4_decode).  A wave's first block is its workgroup index; every later one
// is drawn from a ticket counter in the call's workspace: shard c = workgroup
// & (kTicketShards - 1) hands out blocks G + kTicketShards * t + c (G
// workgroups, ticket t), so a wave whose blocks take longer (their data, a
// crowded SIMD) takes fewer of them and a launch ends within one block of the
// last ticket, not with the wave whose fixed share added up to the most time.
// A shard covers a fixed eighth of the blocks, so an encoder wave whose shard
// has run out steals (blocks of 1 KiB and more; the decoder and smaller blocks
// measured slower with it, prof.hip ticket_steal): it looks at the launch's
// counters, draws (and waits for) one ticket of the shard with the most left
// and goes on there, until every shard is empty (ticket_steal.h; the
// invariants: struct Tickets).  Only the end of a launch pays for that;
// counters over-draw by at most 3 + kTicketShards per wave.
// One set of counters per persistent launch of a call, each on its
// own 64-byte line; zeroed by stream-ordered work the call does anyway (the
// encoder's foot[nb] fill, the decoder's token scan).  Only the wave that
// takes a block changes, never what is written for it.  Which launches draw
// tickets by default is decided per kernel and block size from measurements
// (prof.hip, ticket_sched: eight counters hand out about 400 M tickets/s, which
// the decoder outruns on blocks under 2 KiB); bshuf_set_variant bit
// kStaticSched: none does, workgroup w takes blocks w, w+G, w+2G, ...; bit
// kTicketSched: every launch does, and steals; bit kNoSteal: a wave leaves
// when its own shard runs out.
// (the kernels' side: struct Tickets, bshuf_dev.h)
constexpr size_t kTicketSetBytes = (size_t)kTicketShards * kTicketStride * sizeof(uint32_t);
constexpr int kEncTicketSets = kPipeSegs;  // unsegmented encodes use one or two
constexpr int kStaticSched = 1 << 24;  // static block assignment in both kernels
constexpr int kTicketSched = 1 << 25;  // tickets in both kernels at every block size
constexpr int kNoSteal = 1 << 26;      // no stealing between ticket shards
constexpr int kSideBits = kNoPipe | kNoOverlap | kAltSegments | kWideCompact | kStaticSched | kTicketSched | kNoSteal;
enum TicketKernel { kTicketsEncode, kTicketsDecode };
bool ticket_sched(TicketKernel k, int64_t block_bytes);
bool ticket_steal(int64_t block_bytes);  // k_lz4_encode only

// Workgroups for a persistent launch: resident blocks per CU (occupancy API,
// dynamic LDS included) x CUs of the current device, capped by the work.
int64_t persistent_grid(const void* fn, int threads, size_t lds, int64_t work);
// hipMemsetAsync's job done by a kernel (prof.hip)
hipError_t dev_fill(void* p, int v, size_t n, hipStream_t s);
// Small host table -> device (16-aligned `dev`) on stream s, by a kernel that
// reads a per-thread pinned buffer (host.hip; no DMA engine).  Returns at once;
// the pinned buffer is reused only after that kernel's flags say it was read.
hipError_t stage_upload(const void* host, size_t bytes, void* dev, hipStream_t s);

// One independent framed stream of a batch (bshuf_*_lz4_batch_dev).  All
// streams of a batch share elem_size and block_size; global block k of the
// batch is block k - first of stream blk_seg[k].  The single-stream entry
// points run without a segment table (segs == nullptr).
struct Seg {
    const uint8_t* in;   // encoder: raw input; decoder: framed stream
    uint8_t* out;        // encoder: framed output; decoder: raw output
    int64_t first;       // first global block index
    int64_t nfull;       // full blocks
    int64_t tail;        // raw tail bytes ((size % 8) * elem_size)
    int64_t in_nbytes;   // decoder: readable bytes of the framed stream
    int64_t chunk0;      // decoder: first global index-rebuild chunk
    int64_t nchunks;     // decoder: index-rebuild chunks of this stream
    int64_t seq0;        // decoder: first u32 of this stream's token-position area
    int64_t* result;     // device: bytes written / consumed, or the error code
    int32_t last;        // elements in the partial block (0 = none)
    int32_t pad_;
};

// Fills blk_seg[segs[s].first .. + nblocks(s)) = s for every segment, or with
// chunks = true chunk_seg[segs[s].chunk0 .. + nchunks) = s.
hipError_t launch_seg_map(const Seg* segs, int nsegs, uint32_t* map, bool chunks, hipStream_t s);

// Transpose tiles: kTileGroups (dispatch.h) = 256 groups (2048 elements) per
// 256-thread workgroup.

// bitshuffle / bitunshuffle of all full + partial blocks (tail not included).
hipError_t launch_transpose(const uint8_t* in, uint8_t* out, const Layout& L, bool forward,
                            hipStream_t s);

// ---- LZ4 encode --------------------------------------------------------
struct EncodeBufs {
    uint8_t* scratch;   // nblocks * slot bytes: [BE32 c][c payload] per block
    int64_t slot;       // bytes per scratch slot (16-aligned, >= 4 + lz4_bound)
    uint64_t* foot;     // nblocks + 1 u64: 4 + c per block, last = 0; behind it
                        // kEncTicketSets sets of ticket counters
    uint64_t* offs;     // nblocks + 1 u64: exclusive scan of foot
    void* scan_tmp;     // hipcub temp storage; the pipelined path's tile sums
    size_t scan_tmp_bytes;
    uint8_t* shuf = nullptr;     // large blocks: the bit-transposed input
    uint32_t* tables = nullptr;  // large blocks: kLargeTableWords per block
};
size_t encode_scan_tmp_bytes(int64_t nblocks);
int64_t encode_slot_bytes(const Layout& L);
// fast: the blocks' payloads by the fast parse v1 (lz4_fast.hip) instead of the
// reference's greedy hash parse, when a block is at most kFastMaxBlockBytes;
// scratch slots, offset scan, compaction and finish are the same.
hipError_t launch_encode(const uint8_t* in, uint8_t* out, const Layout& L, int64_t tail_bytes,
                         const EncodeBufs& b, int64_t* d_result, hipStream_t s, bool fast = false);
// Batch of independent streams: segs (device) / hsegs (host copy) describe
// them, L carries the shared bs and E and L.nfull = total blocks.  Every
// stream's blocks must use one LZ4 table type (bs * E < 65547, or every
// block at least that long).  block_offsets (optional): per global block, the
// header offset inside its own stream.
hipError_t launch_encode_batch(const Seg* segs, const Seg* hsegs, int nsegs, const uint32_t* blk_seg,
                               const Layout& L, const EncodeBufs& b, uint64_t* block_offsets,
                               hipStream_t s, bool fast = false);
// (max_device_block_bytes, max_lds_encode_bytes, max_lds_decode_bytes: the
// sizes above which blocks take the global-memory path, dispatch.h)
constexpr int64_t kLargeTableWords = 8192;
// wave-parallel parse of blocks above max_lds_encode_bytes (lz4_encode.hip):
// shuf holds the bit-transposed blocks (64 bytes of pad behind the last)
hipError_t launch_encode_big(const uint8_t* shuf, const Layout& L, const EncodeBufs& b, hipStream_t s);
hipError_t launch_encode_large(const uint8_t* in, const Layout& L, const EncodeBufs& b,
                               uint8_t* shuf, uint32_t* tables, hipStream_t s);

// ---- LZ4 decode --------------------------------------------------------
struct DecodeBufs {
    uint64_t* offs;     // nblocks u64: header offset of each block
    int64_t* status;    // nblocks i64: consumed bytes or error code per block
    uint32_t* seq;      // token positions of the two-phase decode
    // block index rebuild (unused when offsets are supplied)
    int64_t* exits;     // nchunks
    uint64_t* cnt;      // nchunks + 1
    uint64_t* base;     // nchunks + 1
    int64_t* idx_err;   // 1 word
    long long* bad;     // 1 word: highest failing block index
    uint32_t* tickets;  // one set of ticket counters (k_lz4_decode)
    void* scan_tmp;
    size_t scan_tmp_bytes;
    int64_t chunk;      // chunk bytes for the index rebuild
    int64_t nchunks;
    uint8_t* shuf = nullptr;  // large blocks: decoded, still bit-transposed
};
int64_t index_chunk_bytes(const Layout& L);
size_t decode_scan_tmp_bytes(int64_t nchunks);
// dlen (optional): the stream length lives in device memory (read by the
// kernels); blocks_end / in_nbytes are then the CAPACITY's, tail the raw tail.
hipError_t launch_index(const uint8_t* in, int64_t blocks_end, const Layout& L,
                        const DecodeBufs& b, hipStream_t s, const int64_t* dlen = nullptr,
                        int64_t cap = 0, int64_t tail = 0);
hipError_t launch_decode(const uint8_t* in, int64_t in_nbytes, uint8_t* out, const Layout& L,
                         int64_t tail_bytes, const DecodeBufs& b, int64_t* d_result,
                         hipStream_t s, const int64_t* dlen = nullptr);
// wave-parallel execution of blocks above max_lds_decode_bytes (lz4_decode.hip)
hipError_t launch_exec_big(const uint8_t* in, const Layout& L, const DecodeBufs& b, uint8_t* shuf,
                           hipStream_t s);
hipError_t launch_decode_large(const uint8_t* in, int64_t in_nbytes, uint8_t* out, const Layout& L,
                               const DecodeBufs& b, uint8_t* shuf, hipStream_t s);
// Batch versions: L.nfull = total blocks; b.idx_err and b.bad hold one word
// per stream; chunk_seg / blk_seg map global chunks / blocks to streams.
// launch_decode_batch reads of hsegs (the host copy of segs) only the alignment
// of every .out; hsegs == nullptr: the table exists on the device alone, and
// every .out is 16-byte aligned (the window decode's staging areas).
hipError_t launch_index_batch(const Seg* segs, int nsegs, const uint32_t* chunk_seg, const Layout& L,
                              int64_t nchunks, const DecodeBufs& b, hipStream_t s);
hipError_t launch_decode_batch(const Seg* segs, const Seg* hsegs, int nsegs, const uint32_t* blk_seg,
                               const Layout& L, const DecodeBufs& b, hipStream_t s,
                               const int64_t* dlens = nullptr);
// device-held batch stream lengths: segs[i].in_nbytes (the capacity) becomes
// the readable bytes of dlens[i]; run before the index rebuild
hipError_t launch_seg_dlen(Seg* segs, const int64_t* dlens, int nsegs, hipStream_t s);

// ---- range decode (lz4_range.hip) ---------------------------------------
// Element ranges of ONE stream (bshuf_decompress_lz4_ranges_dev): every range
// is cut into pieces (range_plan.h).  A decode piece -- interior blocks, or one
// edge block -- is a Seg of the batch decoder whose input is the stream itself:
// its blocks [b0, b0 + nblk) go to their place in the output (interior) or to a
// staging block of the workspace (edge).  k_range_worklist gathers the
// pieces' header offsets from the stream's index into the work list the batch
// decoder reads as its offs[], k_range_edges copies every edge block's clip
// and every tail span to the output, k_range_reduce makes the call's result.
enum RangePieceKind { kPieceInterior = 0, kPieceEdge = 1, kPieceTail = 2 };
struct RangePiece {
    int64_t b0;          // decode pieces: first block of the stream, and how many
    int64_t nblk;
    int64_t seq_base;    // first u32 of the piece's own token-position area, or -1:
                         // the shared area indexed by stream offset (as a whole decode)
    const uint8_t* src;  // edge: first byte of the clip in the staging block
    uint8_t* dst;        // edge / tail span: where the bytes go
    int64_t lo;          // tail span: first byte inside the verbatim tail
    int64_t n;           // edge / tail span: bytes to copy
    int32_t kind;
    int32_t pad_;
};
// The stream as the range kernels see it.
struct RangeStream {
    const uint8_t* in;
    int64_t in_nbytes;
    const uint64_t* offs;  // block index (supplied, or rebuilt)
    int64_t nb;            // blocks of the whole stream
    int64_t tail;          // verbatim tail bytes of the whole stream
    uint32_t maxlen;       // largest record payload
};
// Decode pieces [0, nd), none of more than max_blk blocks: pieces [0, na) are
// the first launch's (their work blocks start at 0), [na, nd) the second's (at
// nblk_a).  Fills wl[] with each
// work block's header offset (all ones: not inside its piece), and sets every
// Seg's in_nbytes to the end of its piece's last record and seq0 to its
// token-position area.
hipError_t launch_range_worklist(const RangeStream& st, Seg* segs, const RangePiece* pcs, int nd, int na,
                                 int64_t nblk_a, int64_t max_blk, uint64_t* wl, hipStream_t s);
// Pieces [0, np): clips of edge blocks whose decode succeeded (res[p] >= 0)
// and tail spans (res[p] = bytes copied, or -91 when the tail is not inside
// the stream) to their destinations.
hipError_t launch_range_edges(const RangeStream& st, const RangePiece* pcs, int64_t* res, int np,
                              hipStream_t s);
// *result = -91 when *idx_err (nullptr: an index was supplied) is set, else
// the code of the last failing piece, else total.
hipError_t launch_range_reduce(const int64_t* res, int np, const int64_t* idx_err, int64_t total,
                               int64_t* result, hipStream_t s);

// ---- converting gathers (window_copy.h, span_cvt) --------------------------
// The *_cvt_dev entries of the window, ragged and tile decodes: every element x
// of a window or tile lands as (dst kind)fmaf((float)x, scale, offset) instead
// of as itself.  Only the gather kernel differs -- it is instantiated per
// (source kind, destination kind) over SpanCvt instead of SpanCopy -- and only
// where it writes: the plan kernels, the tables, the statuses and the result
// stay the plain call's, in SOURCE bytes; a piece that the tables place b bytes
// behind `out` lands b / sizeof(source) * sizeof(destination) bytes behind it.
// CvtArgs mirrors bshuf_cvt (include/bitshuffle.h), checked by the entry.
enum { kCvtU8, kCvtI8, kCvtU16, kCvtI16, kCvtU32, kCvtI32, kCvtF32, kCvtSrcKinds };
enum { kCvtDstF32, kCvtDstF16, kCvtDstBF16, kCvtDstKinds };
struct CvtArgs {
    int32_t src, dst;
    float scale, offset;
};
constexpr int cvt_src_size(int kind) { return kind < kCvtU16 ? 1 : kind < kCvtU32 ? 2 : 4; }
constexpr int cvt_dst_size(int kind) { return kind == kCvtDstF32 ? 4 : 2; }
// The bytes a gather's lane rule goes by, for n source bytes: the larger of
// what a window or row reads and what it writes.
inline int64_t cvt_lane_bytes(const CvtArgs* cvt, int64_t n) {
    if (!cvt) return n;
    const int S = cvt_src_size(cvt->src), D = cvt_dst_size(cvt->dst);
    return D > S ? n / S * D : n;
}

// ---- window decode (lz4_window.hip) --------------------------------------
// K windows of the same length at DEVICE-held starts, in one stream
// (bshuf_decompress_lz4_windows_dev) or each in a stream of a set
// (bshuf_decompress_lz4_windows_set_dev, below).  With the length and K known
// on the host, every table of the range decode has a host-known shape
// (window_plan.h): window i is one Seg of Mw consecutive blocks of its stream,
// decoded back to back into staging area i, work blocks [i * Mw, (i + 1) * Mw).
// k_window_plan writes the tables from the starts; the work list,
// launch_seg_map and launch_decode_batch run as in the range decode;
// k_window_gather copies each window's clip of its staging area and its span of
// the verbatim tail to the output; k_window_reduce makes the call's result.  No
// host table depends on the starts.  Where a window's stream comes from is the
// call's SOURCE, a template parameter of the plan and gather kernels: WindowStream
// (the one stream of the call) or WindowSet.
//
// A stream set (bshuf_lz4_stream_set_dev) is a device table of `count` framed
// streams that share E and bs: a header, one record per stream, and the block
// indexes the build rebuilt (a stream whose index the caller supplied keeps the
// caller's pointer).  Window i of a call over it is elements [starts[i],
// starts[i] + L) of stream ids[i], both DEVICE arrays.  What differs from one
// stream: Mw = min(M, blocks of the set's largest stream) for every window; a
// token-position area per window (offsets of different streams collide in a
// shared one); a work list of its own, k_window_set_worklist, that takes every
// window's stream from the set.  A bad window (window_plan.h, window_set_plan)
// decodes blocks [0, Mw) of stream `ref`, which has that many, so the work list
// stays dense and inside a real stream; nothing of that decode is used.  When
// the header does not match the call, every window is bad and there is no
// stream to trust: their work blocks then hold the sentinel offset, which the
// decoder rejects without reading anything.
struct WindowTail {
    int64_t lo, n;   // tail span: bytes of the verbatim tail, behind the clip in the window
    int32_t t0, t1;  // work blocks [t0, t1) of the window hold clip bytes
    int32_t bad;     // the window is refused (-71): start out of range, or (set) no such stream
    int32_t pad_;
};
struct WindowCall {
    const int64_t* starts;  // device, K element indices
    uint8_t* out;           // window i at out + i * wbytes
    uint8_t* slots;         // staging areas of `slot` bytes (16-aligned)
    int64_t* res;           // per window: its Seg's result
    int64_t window;         // elements
    int64_t wbytes, slot;
    int64_t Mw;             // work blocks per window
    int64_t seq_words;      // per window, of its own token-position area; -1: the shared area
    int32_t bs, E;
    int32_t K, pad_;
};
constexpr uint64_t kStreamSetMagic = 0x3154455346485342ull;  // "BSHFSET1"
struct StreamSetHeader {
    uint64_t magic;
    int64_t count, E, bs;
    int64_t nb_max;  // blocks of the largest stream
    int64_t ref;     // a stream with nb_max blocks (-1: count == 0)
    int64_t pad_[2];
};
struct StreamSetRec {
    RangeStream st;
    int64_t size;  // elements
    int64_t err;   // 0, or -91: the index was rebuilt and the records do not tile the stream
};
constexpr size_t kStreamSetRecs = 256;  // byte offset of the records in a set
static_assert(sizeof(StreamSetHeader) == 64 && sizeof(StreamSetRec) == 64, "stream set layout");
// rec[s].err and status[s] from the index rebuild's error words (0 -> 0, else -91)
hipError_t launch_stream_set_status(StreamSetRec* recs, const int64_t* idx_err, int64_t* status, int count,
                                    hipStream_t s);
// The two sources.
struct WindowStream {
    RangeStream st;  // (the plan reads st.in only: st.offs may still be under construction)
    int64_t size;    // elements
};
struct WindowSet {
    const StreamSetHeader* hdr;
    const StreamSetRec* recs;
    const int64_t* ids;     // device, K stream indices
    int32_t* sidx;          // per window: the stream its blocks come from (-1: none, sentinel offsets)
    int64_t count, nb_max;  // what the call says of the set
};
// (instantiated for the two sources in lz4_window.hip)
template <class Source>
hipError_t launch_window_plan(const Source& src, const WindowCall& c, Seg* segs, RangePiece* pcs,
                              WindowTail* wt, hipStream_t s);
// k_range_worklist with every piece's stream taken from the set's record of src.sidx[piece]
hipError_t launch_window_set_worklist(const WindowSet& src, const WindowCall& c, Seg* segs,
                                      const RangePiece* pcs, uint64_t* wl, hipStream_t s);
// status[i] (wstat): c.wbytes, or -71 (bad window), -91 (set: the stream's error
// word), the code of the highest failing block that holds clip bytes (dstat: the
// decode's per-block status), or -91 (tail not inside the stream); only windows
// with c.wbytes are copied -- with cvt, converted (window i then lands at out + i *
// window destination elements; the statuses stay source bytes).
template <class Source>
hipError_t launch_window_gather(const Source& src, const WindowCall& c, const RangePiece* pcs,
                                const WindowTail* wt, const int64_t* dstat, int64_t* wstat, hipStream_t s,
                                const CvtArgs* cvt = nullptr);
// *result = -91 when *idx_err (nullptr: no index was rebuilt by the call) is set,
// else -71 when a window was bad, else the status of the highest-numbered
// failing window, else total (K * wbytes) -- or, with dtotal, `total` bytes for
// each of the *dtotal elements of a device-held count (the ragged decode).
hipError_t launch_window_reduce(const int64_t* wstat, const WindowTail* wt, int K, const int64_t* idx_err,
                                int64_t total, int64_t* result, hipStream_t s, const int64_t* dtotal = nullptr);

// ---- ragged window decode (lz4_ragged.hip) ---------------------------------
// K windows at DEVICE-held starts AND lengths (bshuf_decompress_lz4_ragged_dev,
// bshuf_decompress_lz4_ragged_set_dev); the host knows max_window, a bound on
// the lengths, which with K fixes every table of the window decode: window i is
// still one Seg of Mw work blocks with a staging area of its own.  What differs:
// k_ragged_scan places the windows in the output (the exclusive scan of their
// lengths, 0 for a refused one; window_plan.h, ragged_good) and k_ragged_plan
// plans each with its own length (ragged_plan).  Of a window's Mw work blocks
// only [t0, t1) hold bytes of it; k_ragged_worklist gives those their header
// offsets and every other one the sentinel (kNoOffset, range_worklist.h), and
// narrows the window's readable bytes to the live blocks' records, so nothing of
// a block the window does not need is read, and such a block's failure is not
// the window's.  It also writes the block -> window map over all Mw work blocks
// (launch_seg_map would stop at the blocks a short stream of a set has).  The
// token scan and the block decode run unchanged; k_ragged_gather is
// k_window_gather with the window's own byte count, the reduce k_window_reduce
// with the total read from the scan's last entry.
struct RaggedCall {
    WindowCall w;           // (w.window: max_window; w.wbytes: max_window * E; w.out: the output's base)
    const int64_t* counts;  // device, K element counts
    int64_t* offs;          // device, K + 1: the exclusive scan of the good windows' counts
    int64_t capacity;       // elements of the output
    int64_t pitch;          // 0: packed, window i at element offs[i]; else at i * pitch
};
constexpr int kRaggedScanTiles = 1024;  // tile sums of the placement scan (workspace)
// offs[0 .. K] from the starts and counts (and ids); sums: kRaggedScanTiles words.
template <class Source>
hipError_t launch_ragged_scan(const Source& src, const RaggedCall& c, int64_t* sums, hipStream_t s);
// Seg, RangePiece, WindowTail and (set) src.sidx entry i; a refused window, or
// one that has no room in a packed output, has no stream bytes to read at all.
template <class Source>
hipError_t launch_ragged_plan(const Source& src, const RaggedCall& c, Seg* segs, RangePiece* pcs,
                              WindowTail* wt, hipStream_t s);
// wl and blk_seg over the K * Mw work blocks, every Seg's in_nbytes and seq0.
template <class Source>
hipError_t launch_ragged_worklist(const Source& src, const RaggedCall& c, Seg* segs, const RangePiece* pcs,
                                  const WindowTail* wt, uint64_t* wl, uint32_t* blk_seg, hipStream_t s);
// launch_window_gather's rule, window i's byte count being counts[i] * E.
template <class Source>
hipError_t launch_ragged_gather(const Source& src, const RaggedCall& c, const RangePiece* pcs,
                                const WindowTail* wt, const int64_t* dstat, int64_t* wstat, hipStream_t s,
                                const CvtArgs* cvt = nullptr);

// ---- tile decode (lz4_tile.hip) -------------------------------------------
// K tiles of rows x cols elements at DEVICE-held flat starts, row r of tile i
// being elements [starts[i] + r * pitch, ... + cols) of one stream
// (bshuf_decompress_lz4_tiles_dev) or of stream ids[i] of a set
// (bshuf_decompress_lz4_tiles_set_dev).  The host-known shape (tile_plan.h,
// tile_shape) cuts every tile into G groups of rg rows; a group is what a
// window is to the window decode -- Seg i * G + g of Mg consecutive blocks,
// decoded back to back into staging area i * G + g -- so the work list,
// launch_seg_map and launch_decode_batch run as they do there over K * G pieces.
// k_tile_plan writes the tables from the starts (and ids); k_tile_gather settles
// every tile's status and copies the rows of the good ones out of their groups'
// areas and the verbatim tail; k_tile_reduce makes the call's result.  The
// sources are the window decode's.
struct TileInfo {
    int64_t start;  // the tile's flat element index
    int32_t bad;    // refused (-71): start out of range, or (set) no stream that takes the tile
    int32_t sidx;   // set: the tile's stream (a bad tile: none)
};
struct TileCall {
    const int64_t* starts;  // device, K element indices
    uint8_t* out;           // row r of tile i at out + (i * rows + r) * rbytes
    uint8_t* slots;         // K * G staging areas of `slot` bytes (16-aligned)
    int64_t* res;           // per group: its Seg's result
    int64_t rows, cols, pitch;
    int64_t rg, G, Mg;      // tile_shape
    int64_t rbytes, slot;   // bytes of a row, of a staging area
    int64_t seq_words;      // per group, of its own token-position area; -1: the shared area
    int32_t bs, E;
    int32_t K, pad_;
};
// Seg, RangePiece and (set) src.sidx entries i * G + g, TileInfo i.  A bad tile
// of a set decodes blocks [0, Mg) of the set's stream `ref`; with a mismatched
// header no tile has a stream (sidx -1: sentinel offsets), as for windows.
template <class Source>
hipError_t launch_tile_plan(const Source& src, const TileCall& c, Seg* segs, RangePiece* pcs, TileInfo* ti,
                            hipStream_t s);
// status[i] (tstat): rows * rbytes, or -71 (bad tile), -91 (set: the stream's
// error word), the code of the highest failing block -- in stream order -- among
// those that hold an element of the tile (dstat: the decode's per-block
// status), or -91 (a row reaches a verbatim tail that is not inside the stream);
// only tiles with rows * rbytes are copied (with cvt: converted, row r of tile i
// at out + (i * rows + r) * cols destination elements), the others not at all.
template <class Source>
hipError_t launch_tile_gather(const Source& src, const TileCall& c, const RangePiece* pcs, const TileInfo* ti,
                              const int64_t* dstat, int64_t* tstat, hipStream_t s, const CvtArgs* cvt = nullptr);
// A/B of the gather's lanes per row (bshuf_set_variant; values of their own,
// which no other kernel reads): 16, 64 or 256 whatever the row's bytes.
constexpr int kTileLanes16 = 1 << 22;
constexpr int kTileLanes64 = 1 << 23;
constexpr int kTileLanes256 = kTileLanes16 | kTileLanes64;
// launch_window_reduce's rule over tiles.
hipError_t launch_tile_reduce(const int64_t* tstat, const TileInfo* ti, int K, const int64_t* idx_err,
                              int64_t total, int64_t* result, hipStream_t s);

// ---- the reference's internal transpose steps (internals.hip) -------------
// out[(j * lda + i) * es + t] = in[(i * ldb + j) * es + t]  (bshuf_trans_elem)
hipError_t launch_trans_elem(const uint8_t* in, uint8_t* out, int64_t lda, int64_t ldb, int64_t es,
                             hipStream_t s);
// bshuf_shuffle_bit_eightelem_scal of `size` (multiple of 8) E-byte elements
hipError_t launch_shuffle_bit_eightelem(const uint8_t* in, uint8_t* out, int64_t size, int64_t E,
                                        hipStream_t s);

// ---- synthetic inputs ----------------------------------------------------
hipError_t launch_synth(void* out, size_t n, int gen, uint64_t first, uint64_t seed,
                        hipStream_t s);

}  // namespace bshuf
