// inplace.h -- where the in-place decoder (k_lz4_decode<*, VAR & 512>,
// lz4_decode.hip) puts a record inside the decoded block's own LDS buffer, and
// the test that decides whether the block may be decoded from there.  Shared by
// the kernel, its launcher and a host build (scan_host.cpp, loaded only by the
// CPU tests), so the tests search for streams on either side of the test with
// the arithmetic the GPU runs.
//
// The buffer holds the decoded block at [0, cap) and ends at ip_end.  A record
// span (header, payload and, for a stream's last block, whatever follows it up
// to the largest record size) arrives as whole 16-byte granules aligned on its
// global address: `shift` bytes of the first granule precede the header, and
// the granules end at ip_end.  Sequence j writes its output from op_j on and
// reads its token at payload position tp_j, so decoding in place is safe when
// no op_j lies above its token: mx = max_j (op_j - tp_j), which the scan
// records, is at most the payload's LDS offset.
#pragma once
#include <stdint.h>

#ifndef BSHUF_HD
#if defined(__HIPCC__)
#define BSHUF_HD __host__ __device__
#else
#define BSHUF_HD
#endif
#endif

namespace bshuf {

// Bytes behind the decoded block reserved for the in-place record (keeps one
// buffer within 7 LDS granules = 8,960 bytes: 18 waves per CU)
constexpr int kInPlaceMargin = 704;

// The scan's verdict word carries mx + kMxBias in kMxBits bits from bit 32 on
// (the low 32 bits: the sequence count).  -2^14 <= mx <= block bytes <= 160 KiB,
// so 18 bits hold every value: a field that saturates below the true mx (16
// bits did, from 48 KiB on) lets a block pass the test it fails.
constexpr int kMxBias = 1 << 14;
constexpr int kMxBits = 18;
static_assert(160 * 1024 + kMxBias < (1 << kMxBits), "mx of the largest LDS block fits its field");
constexpr int kMxMask = (1 << kMxBits) - 1;

BSHUF_HD inline int64_t inplace_mx_pack(int mx) {
    const int v = mx + kMxBias;
    return (int64_t)(v < 0 ? 0 : (v > kMxMask ? kMxMask : v)) << 32;
}
BSHUF_HD inline int inplace_mx_unpack(int64_t verdict) { return (int)((verdict >> 32) & kMxMask) - kMxBias; }

// LDS offset at which the in-place record region ends (cap: the 16-aligned
// bytes reserved for the decoded block).
BSHUF_HD inline int inplace_end(int cap) { return (cap + kInPlaceMargin + 15) & ~15; }

// 16-byte granules covering span_bytes that start `shift` bytes into a granule.
BSHUF_HD inline int span_granules(int shift, int span_bytes) { return (shift + span_bytes + 15) >> 4; }

// LDS offset of the span's first granule.  (k_lz4_decode writes this one out as
// smem + ip_end - 16 * granules: the other association of the pointer sum
// changes its register allocation.)
BSHUF_HD inline int inplace_span_off(int ip_end, int granules) { return ip_end - 16 * granules; }

// The margin test: span_off + shift + 4 is the payload's LDS offset.
BSHUF_HD inline bool inplace_fits(int mx, int span_off, int shift) { return mx <= span_off + shift + 4; }

}  // namespace bshuf
