// cvt_span.h -- how the converting gathers (window_copy.h, span_cvt) cut one
// span of n source elements of S bytes, written as n elements of D bytes: one
// pure function, run by every lane on the device and by the CPU suite through
// libbshuf_hostcheck.so: no HIP but the qualifiers of window_plan.h.
//
// The source starts at a byte address congruent to `src` mod 16 and is
// S-aligned; the destination at one congruent to `dst` mod 16 and D-aligned.
// A span of fewer than 32 source bytes goes element by element.  Otherwise:
//   head   elements before dst's first 16-byte boundary, one by one;
//   nu     UNITS of ue = max(16 / S, 16 / D) elements: ue * S / 16 source
//          granules (1 or 2) become ue * D / 16 whole 16-byte chunks of dst (1,
//          2 or 4), all of them by one lane.  Every unit's source lies r bytes
//          behind a 16-byte boundary; it is read as its aligned granules, one
//          more when r != 0, which then still holds r bytes of the unit;
//   nc     whole chunks behind the units (fewer than a unit has), each by one
//          lane from 16 / D single element loads;
//   tail   elements behind dst's last 16-byte boundary, one by one.
// Single loads and stores are of one element inside the span, so no read
// leaves the 16-byte granules that hold a byte of the span and no write leaves
// the span.
#pragma once

#include <stdint.h>

#include "window_plan.h"

namespace bshuf {

constexpr int64_t kCvtSingleBytes = 32;  // (span_copy's rule)

struct CvtSpan {
    int64_t head, nu, nc, tail;  // elements, units, chunks, elements
    int32_t ue;                  // elements of a unit
    int32_t r;                   // bytes the units' source lies behind a 16-byte boundary
};

BSHUF_WINDOW_FN void cvt_span_plan(uint32_t src, uint32_t dst, int S, int D, int64_t n, CvtSpan& p) {
    const int epc = 16 / D;  // elements of a chunk of dst
    p.ue = 16 / S > epc ? 16 / S : epc;
    p.r = 0;
    if (n * S < kCvtSingleBytes) {
        p.head = n;
        p.nu = p.nc = p.tail = 0;
        return;
    }
    p.head = (int64_t)(((16 - (dst & 15)) & 15) / D);
    const int64_t body = n - p.head;
    p.nu = body / p.ue;
    const int64_t rest = body - p.nu * p.ue;
    p.nc = rest / epc;
    p.tail = rest - p.nc * epc;
    p.r = (int32_t)((src + (uint32_t)p.head * (uint32_t)S) & 15);
}

}  // namespace bshuf
