// window_plan.h -- one fixed-length window of a framed stream as the window
// decode sees it (bshuf_decompress_lz4_windows_dev; launch.h, "window decode").
// One pure function, run per window by k_window_plan on the device (the starts
// live in device memory) and by the CPU suite through libbshuf_hostcheck.so:
// no HIP but the qualifiers below.
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

// 1 <= window <= size (checked by the caller); any start.
BSHUF_WINDOW_FN void window_plan(int64_t size, int64_t bs, int64_t E, int64_t window, int64_t start,
                                 WindowPlan& w) {
    const int64_t sfull = size / bs;
    const int64_t slast = size % bs - size % 8;
    const int64_t covered = sfull * bs + slast;  // the blocks' elements
    const int64_t nb = sfull + (slast ? 1 : 0);
    const int64_t Mw = window_blocks(size, bs, window);
    w.bad = (start < 0 || start > size - window) ? 1 : 0;
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

}  // namespace bshuf
