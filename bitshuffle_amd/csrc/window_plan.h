// window_plan.h -- one fixed-length window of a framed stream as the window
// decode sees it (bshuf_decompress_lz4_windows_dev; launch.h, "window decode").
// One pure function, run per window by k_window_plan on the device (the starts
// live in device memory) and by the CPU suite through libbshuf_hostcheck.so:
// no HIP but the qualifiers below.  window_set_plan, at the end, is the same for
// a window in one of a set of streams (bshuf_decompress_lz4_windows_set_dev),
// ragged_plan for a window with a length of its own (bshuf_decompress_lz4_ragged_dev).
//
// The stream of `size` elements in blocks of `bs` (plan.h, make_plan): nfull
// full blocks, one partial block of `last` elements when that is not 0, then
// size % 8 verbatim tail elements; nb blocks cover elements [0, covered).
// Every window of `window` elements touches at most (window + bs - 2) / bs + 1
// blocks, so every window of a call decodes the same number Mw of consecutive
// blocks [b0, b0 + Mw), back to back into a staging area of its own.  The
// window's decoded elements are then ONE contiguous clip of that area, and the
// rest of it, [max(start, covered), start + window), a span of the verbatim
// tail.
#pragma once

#include <stdint.h>

#ifdef __HIPCC__
#define BSHUF_WINDOW_FN __host__ __device__ __forceinline__
#else
#define BSHUF_WINDOW_FN inline
#endif

namespace bshuf {

struct WindowPlan {
    int64_t b0;       // first block decoded
    int64_t nfull;    // of the Mw decoded blocks, the full ones (Mw, or Mw - 1 and ...
    int32_t last;     // ... the stream's partial block of `last` elements behind them)
    int32_t bad;      // start < 0 or start > size - window: b0 = 0, clip and tail span empty
    int64_t clip_lo;  // clip: bytes [clip_lo, clip_lo + clip_n) of the staging area
    int64_t clip_n;
    int64_t tail_lo;  // tail span: bytes [tail_lo, tail_lo + tail_n) of the verbatim tail,
    int64_t tail_n;   // behind the clip in the window
    int64_t t0, t1;   // the decoded blocks that hold clip bytes: [t0, t1) of the Mw
};

// Work blocks of every window of a call: the same for every start.
BSHUF_WINDOW_FN int64_t window_blocks(int64_t size, int64_t bs, int64_t window) {
    const int64_t last = size % bs - size % 8;
    const int64_t nb = size / bs + (last ? 1 : 0);
    const int64_t m = (window + bs - 2) / bs + 1;
    return m < nb ? m : nb;
}

// The plan of one window that decodes Mw consecutive blocks of its stream
// (Mw <= nb, and at least the blocks a window of that length can touch); bad:
// nothing of the window is copied, blocks [0, Mw) are decoded.
BSHUF_WINDOW_FN void window_plan_blocks(int64_t size, int64_t bs, int64_t E, int64_t window, int64_t start,
                                        int64_t Mw, bool bad, WindowPlan& w) {
    const int64_t sfull = size / bs;
    const int64_t slast = size % bs - size % 8;
    const int64_t covered = sfull * bs + slast;  // the blocks' elements
    const int64_t nb = sfull + (slast ? 1 : 0);
    w.bad = bad ? 1 : 0;
    const int64_t s = w.bad ? 0 : start;
    int64_t b0 = s / bs;
    if (b0 > nb - Mw) b0 = nb - Mw;  // (nb == 0: Mw == 0 and b0 == 0)
    w.b0 = b0;
    const bool ends = b0 + Mw == nb && slast != 0 && Mw > 0;
    w.nfull = ends ? Mw - 1 : Mw;
    w.last = ends ? (int32_t)slast : 0;
    w.clip_lo = w.clip_n = w.tail_lo = w.tail_n = 0;
    w.t0 = w.t1 = 0;
    if (w.bad) return;
    const int64_t end = s + window;
    const int64_t e = end < covered ? end : covered;
    if (e > s) {
        w.clip_lo = (s - b0 * bs) * E;
        w.clip_n = (e - s) * E;
        w.t0 = s / bs - b0;
        w.t1 = (e - 1) / bs - b0 + 1;
    }
    if (end > covered) {
        const int64_t from = s > covered ? s : covered;
        w.tail_lo = (from - covered) * E;
        w.tail_n = (end - from) * E;
    }
}

// 1 <= window <= size (checked by the caller); any start.
BSHUF_WINDOW_FN void window_plan(int64_t size, int64_t bs, int64_t E, int64_t window, int64_t start,
                                 WindowPlan& w) {
    window_plan_blocks(size, bs, E, window, start, window_blocks(size, bs, window),
                       start < 0 || start > size - window, w);
}

// ---- windows over a set of streams (bshuf_decompress_lz4_windows_set_dev) ----
// Window i of such a call is elements [start, start + window) of stream `id` of
// `count` streams that share bs and E.  Every window of the call decodes the
// same number of blocks, Mw = min((window + bs - 2) / bs + 1, blocks of the
// set's largest stream), whatever its stream: one shape per call.  `size` is
// stream id's element count (anything when id is outside [0, count)).  The
// window is bad -- status -71, nothing copied -- when id is outside [0, count),
// window > size, start is outside [0, size - window], or the stream has fewer
// than Mw blocks.  A good window gets window_plan's result for its stream with
// Mw forced (a stream of at least Mw blocks holds every block a window of that
// length touches: Mw is either that bound or all blocks of the largest stream).
// A bad one has nothing to copy and b0 = 0: with only its start out of range it
// is window_plan's bad window of its stream, else Mw full blocks; the caller
// decodes blocks [0, Mw) of a stream that has them in its place.
BSHUF_WINDOW_FN void window_set_plan(int64_t count, int64_t id, int64_t size, int64_t bs, int64_t E,
                                     int64_t window, int64_t start, int64_t Mw, WindowPlan& w) {
    bool bad = id < 0 || id >= count || window > size;
    if (!bad) {
        const int64_t nb = size / bs + (size % bs - size % 8 ? 1 : 0);
        bad = nb < Mw;
    }
    if (bad) {
        w = WindowPlan{};
        w.nfull = Mw;
        w.bad = 1;
        return;
    }
    window_plan_blocks(size, bs, E, window, start, Mw, start < 0 || start > size - window, w);
}

// ---- ragged windows (bshuf_decompress_lz4_ragged_dev, ..._ragged_set_dev) ----
// Window i of such a call is elements [start, start + count) of its stream, the
// count device-held like the start; the host knows an upper bound max_window,
// and Mw = window_blocks(size of the (largest) stream, bs, max_window) for every
// window.  The window is good when 0 <= count <= max_window and 0 <= start <=
// size - count (`size`: its stream's; 0 for a stream the set does not have, so
// that only count 0 at start 0 could pass -- the caller refuses an unknown id
// itself).
BSHUF_WINDOW_FN bool ragged_good(int64_t size, int64_t max_window, int64_t start, int64_t count) {
    return count >= 0 && count <= max_window && count <= size && start >= 0 && start <= size - count;
}

// The plan of one ragged window: window_plan_blocks with the window's own count
// and min(Mw, nb) blocks, nb the blocks of its stream.  A stream with at least
// Mw blocks gets what a fixed-length window of `count` elements with Mw forced
// gets: of the Mw work blocks only [t0, t1) hold bytes of the window, and the
// caller leaves the others inert.  A stream of a set with fewer blocks than Mw
// plans good all the same: b0 = 0, nfull / last describe its nb blocks, and work
// blocks [nb, Mw) are inert like the others outside [t0, t1).  refused: the
// caller's own reasons (unknown stream, no room in the output) on top of
// ragged_good; a refused window has b0 = 0, t0 = t1 = 0 and nothing to copy.
BSHUF_WINDOW_FN void ragged_plan(int64_t size, int64_t bs, int64_t E, int64_t max_window, int64_t count,
                                 int64_t start, int64_t Mw, bool refused, WindowPlan& w) {
    const int64_t nb = size / bs + (size % bs - size % 8 ? 1 : 0);
    const bool bad = refused || !ragged_good(size, max_window, start, count);
    window_plan_blocks(size, bs, E, bad ? 0 : count, start, Mw < nb ? Mw : nb, bad, w);
}

}  // namespace bshuf
