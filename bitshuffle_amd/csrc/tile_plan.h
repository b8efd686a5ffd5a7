// tile_plan.h -- one rows x cols tile of a framed stream as the tile decode sees
// it (bshuf_decompress_lz4_tiles_dev, bshuf_decompress_lz4_tiles_set_dev;
// launch.h, "tile decode").  Pure functions in the style of window_plan.h, run
// on the host (the shape), per (tile, group) by k_tile_plan and per row by
// k_tile_gather on the device, and by the CPU suite through
// libbshuf_hostcheck.so: no HIP but the qualifiers.
//
// Row r of a tile at flat element index `start` is elements [start + r * pitch,
// ... + cols) of its stream; the tile spans (rows - 1) * pitch + cols elements.
// The tile is cut into G = ceil(rows / rg) GROUPS of rg consecutive rows (the
// last may hold fewer).  A group is what a window is to the window decode: the
// (rows_g - 1) * pitch + cols elements from its first row's start on, one Seg of
// Mg consecutive blocks [b0, b0 + Mg) decoded back to back into a staging area
// of its own (window_plan_blocks with Mg forced).  Every row is then one
// contiguous clip of its group's area plus, behind it, a span of the verbatim
// tail.  rg, G and Mg depend on rows, cols, pitch, bs and the stream's block
// count alone: one shape per call, whatever the starts.
#pragma once

#include "window_plan.h"

namespace bshuf {

struct TileShape {
    int64_t rg;  // rows per group
    int64_t G;   // groups per tile
    int64_t Mg;  // work blocks per group
};

// Blocks a run of W >= 1 elements can touch at the worst start.
BSHUF_WINDOW_FN int64_t tile_run_blocks(int64_t W, int64_t bs) { return (W + bs - 2) / bs + 1; }

// The rg in 1..rows with the fewest decoded blocks G * Mg per tile, Mg =
// min(blocks a group's run can touch, nb); of equal costs the larger rg (fewer
// Segs).  Because the bound carries a worst-case +1, an rg between 1 (a window
// per row) and rows (one run) wins for pitches around two blocks.  rows, cols
// >= 1, pitch >= cols; nb: blocks of the stream (of a set's largest stream).
// Once a run can touch every block of the stream the cost ceil(rows / rg) * nb
// only falls with rg, so the search goes straight to rg = rows from there.  With
// pitch <= bs there is nothing to search: a further row adds at most one block
// to a run, a further group at least one, so the one run is the minimum (and the
// largest rg); the search is then over rows that lie more than a block apart,
// fewer than nb steps.
BSHUF_WINDOW_FN void tile_shape(int64_t rows, int64_t cols, int64_t pitch, int64_t bs, int64_t nb,
                                TileShape& t) {
    int64_t best = INT64_MAX;
    t.rg = rows;
    t.G = 1;
    t.Mg = 0;
    for (int64_t rg = pitch <= bs ? rows : 1; rg <= rows; rg++) {
        int64_t M = tile_run_blocks((rg - 1) * pitch + cols, bs);
        if (M >= nb) {
            M = nb;
            rg = rows;
        }
        const int64_t G = (rows + rg - 1) / rg;
        if (G * M <= best) {
            best = G * M;
            t.rg = rg;
            t.G = G;
            t.Mg = M;
        }
    }
}

// A tile of one stream is bad -- status -71, nothing copied -- when its start
// is outside [0, size - span] (span <= size: checked by the caller).
BSHUF_WINDOW_FN bool tile_bad(int64_t size, int64_t span, int64_t start) {
    return start < 0 || start > size - span;
}

// ... and over a set of `count` streams also when id is outside [0, count),
// span is above its stream's `size` (anything when id is outside), or the
// stream has fewer than Mg blocks (the window-set rule, window_set_plan).
BSHUF_WINDOW_FN bool tile_set_bad(int64_t count, int64_t id, int64_t size, int64_t bs, int64_t span,
                                  int64_t start, int64_t Mg) {
    if (id < 0 || id >= count || span > size) return true;
    const int64_t nb = size / bs + (size % bs - size % 8 ? 1 : 0);
    return nb < Mg || tile_bad(size, span, start);
}

// Group g of the tile at `start`: window_plan_blocks of the group's run with Mg
// forced and the TILE's bad flag (a bad tile: blocks [0, Mg), nothing to copy).
// The group's own clip and tail span are not used: rows are copied one by one.
BSHUF_WINDOW_FN void tile_group(int64_t size, int64_t bs, int64_t E, int64_t rows, int64_t cols, int64_t pitch,
                                const TileShape& t, int64_t start, int64_t g, bool bad, WindowPlan& w) {
    const int64_t r0 = g * t.rg;
    const int64_t rows_g = rows - r0 < t.rg ? rows - r0 : t.rg;
    window_plan_blocks(size, bs, E, (rows_g - 1) * pitch + cols, bad ? 0 : start + r0 * pitch, t.Mg, bad, w);
}

struct TileRow {
    int64_t g;        // the row's group
    int64_t lo, n;    // clip: bytes [lo, lo + n) of that group's staging area
    int64_t tail_lo;  // tail span: bytes [tail_lo, tail_lo + tail_n) of the verbatim tail,
    int64_t tail_n;   // behind the clip in the row
    int64_t t0, t1;   // the group's work blocks that hold clip bytes: [t0, t1) of its Mg
};

// The elements of a stream that its blocks hold (the rest: the verbatim tail).
BSHUF_WINDOW_FN int64_t tile_covered(int64_t size, int64_t bs) { return size / bs * bs + (size % bs - size % 8); }

// Row r of a good tile at `start`; b0: first block of the row's group r / rg
// (tile_group); covered: tile_covered of the stream, which a caller of many
// rows computes once.  The fields follow from b0 and covered as
// window_plan_blocks derives a window's.
BSHUF_WINDOW_FN void tile_row(int64_t covered, int64_t bs, int64_t E, int64_t cols, int64_t pitch, int64_t rg,
                              int64_t start, int64_t r, int64_t b0, TileRow& o) {
    const int64_t s = start + r * pitch;
    const int64_t end = s + cols;
    const int64_t e = end < covered ? end : covered;
    o.g = rg == 1 ? r : r / rg;
    o.lo = o.n = o.tail_lo = o.tail_n = 0;
    o.t0 = o.t1 = 0;
    if (e > s) {
        o.lo = (s - b0 * bs) * E;
        o.n = (e - s) * E;
        o.t0 = s / bs - b0;
        o.t1 = (e - 1) / bs - b0 + 1;
    }
    if (end > covered) {
        const int64_t from = s > covered ? s : covered;
        o.tail_lo = (from - covered) * E;
        o.tail_n = (end - from) * E;
    }
}

}  // namespace bshuf
