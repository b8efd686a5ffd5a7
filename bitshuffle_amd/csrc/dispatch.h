// dispatch.h -- which kernel path a call takes, as plain host functions.
//
// Every device entry point picks its path from three things the caller
// controls: the element size E, the bytes per block (bs * E) and the low four
// bits of the data and output pointers.  The launchers (launch_encode,
// launch_encode_batch, launch_encode_fast, decode_impl, launch_decode,
// launch_decode_batch, launch_transpose) call the functions below and decide
// nothing on their own; the kernels' in-kernel sub-paths read the constants.
// No HIP dependency: a host build (scan_host.cpp, loaded only by the CPU tests)
// exports the same functions, and tests/dispatch_model.py restates them, so
// the table of DESIGN.md "Kernel paths" is pinned by a CPU test and the GPU
// sweep (tests/test_gpu_dispatch.py) derives its cells from these thresholds.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "inplace.h"

namespace bshuf {

// Reference constants of the LZ4 block format (lz4/lz4.c:242-249, 710).
constexpr int kMfLimit = 12;
constexpr int kU16TableLimit = 65536 + kMfLimit - 1;  // LZ4_64Klimit: byU32 from here on
BSHUF_HD inline int lz4_bound(int n) { return n + n / 255 + 16; }

constexpr int64_t kLdsBytes = 160 * 1024;  // LDS of one CU

// ---- alignment ------------------------------------------------------------
// A batch ANDs the flags over all its streams: one odd stream moves them all.
struct Align {
    bool a16 = true;  // every pointer 16-byte aligned
    bool a8 = true;   // every pointer 8-byte aligned
    void add(uintptr_t p) {
        a16 = a16 && (p & 15) == 0;
        a8 = a8 && (p & 7) == 0;
    }
};
inline Align align_of(uintptr_t p) {
    Align a;
    a.add(p);
    return a;
}

// Element sizes with register-transpose kernel instantiations.
inline bool ek_size(int E) { return E == 1 || E == 2 || E == 4 || E == 8; }
// The EK template argument of the LZ4 kernels: E, or 0 for the any-size paths.
inline int pick_ek(int E, bool a16) { return a16 && ek_size(E) ? E : 0; }

// ---- exact encoder (lz4_encode.hip) ----------------------------------------
constexpr int kTableBytes = 16384;  // hash table: byU16 8192 x u16, byU32 4096 x u32
constexpr int kDataPad = 16;        // zeroed read pad behind the block in LDS
constexpr int kDescMax = 256;              // descriptor slots per block
constexpr int kDescBytes = 8 * kDescMax;   // LDS behind the block
// EK == 0: a block of at most kRawBytes from an 8-aligned source is staged
// (8-byte loads into registers, transpose out of LDS); else byte gathers.
constexpr int kRawBytes = 8192;
// EK != 0: groups (of 8 elements) the prefetch registers hold -- one group per
// lane and step (`fits`), or four (`fits4`, group count a multiple of 4);
// larger blocks are loaded chunk by chunk inside the transpose.
constexpr int enc_reg_groups(int EK) { return EK ? (8192 / (64 * 8 * EK)) * 64 : 64; }
constexpr int enc_reg_groups4(int EK) {
    return (EK && 8192 / (64 * 32 * EK) > 0 ? 8192 / (64 * 32 * EK) : 1) * 64 * 4;
}

// Largest block (bytes) the LDS-resident encoder accepts; above it the
// global-memory path (lz4_large.hip).
inline int64_t max_device_block_bytes() { return kLdsBytes - kTableBytes - 64; }
inline int64_t max_lds_encode_bytes() { return max_device_block_bytes(); }

// E = 1 from a source that is 8- but not 16-byte aligned is not staged: the
// staged transpose's 32-bit reciprocal of E has no value for 1.
inline bool enc_raw8(int E, bool a8) { return a8 && E != 1; }
// the byU32 table
inline bool enc_wide(int64_t block_bytes) { return block_bytes >= kU16TableLimit; }
// Sequence descriptors behind the block when the record fits the table's LDS
// as staging (every block of up to ~16 KiB).
inline bool enc_desc(int64_t nmax) { return !enc_wide(nmax) && 4 + lz4_bound((int)nmax) + 15 <= kTableBytes; }
inline int32_t enc_desc_off(int64_t nmax) { return (int32_t)(((nmax + 15) & ~(int64_t)15) + kDataPad); }
inline size_t enc_lds_bytes(int64_t nmax) {
    return kTableBytes + (size_t)enc_desc_off(nmax) + (enc_desc(nmax) ? kDescBytes : 0);
}

// ---- fast encoder (lz4_fast.hip) -------------------------------------------
// fast parse v1 covers blocks up to kFastMaxBlockBytes; above, the exact path
constexpr int64_t kFastMaxBlockBytes = 65536;
inline bool fast_applies(int64_t block_bytes) { return block_bytes <= kFastMaxBlockBytes; }
// The compact LDS layout (SREG) of blocks up to 8 KiB with E = 1, 2, 4: whole
// 32-byte words, the block 16-aligned behind the bitmaps.  A block the
// register transpose does not take is transposed straight from HBM there,
// staged (by 8-byte words or by bytes, on `src & 7`) in the other layout.
constexpr int kSregWords = 4 * 64;
inline bool fast_sreg(int ek, int64_t nmax) {
    const int64_t nw = (nmax + 31) >> 5;
    return ek != 0 && ek != 8 && nmax % 32 == 0 && nw % 4 == 0 && nw <= kSregWords;
}

// ---- decoder (lz4_decode.hip) ----------------------------------------------
// Blocks above this size take the global-memory path: decoded block + 16 +
// record (bound + header + 32 slack, 16-aligned) in 160 KiB.
inline int64_t max_lds_decode_bytes() {
    static const int64_t found = [] {  // (searched once per process, not per call)
        int64_t n = kLdsBytes;
        while (n > 0) {
            const int64_t rec = (lz4_bound((int)n) + 4 + 32 + 15) & ~(int64_t)15;
            if (((n + 15) & ~(int64_t)15) + 16 + rec <= kLdsBytes) break;
            n -= 8;
        }
        return n;
    }();
    return found;
}
// LDS bytes reserved for the decoded block
inline int32_t dec_cap(int64_t nmax) { return (int32_t)((nmax + 15) & ~(int64_t)15); }
// decoded block + record (header, payload, 16-byte alignment slack)
inline size_t dec_rec_bytes(uint32_t maxlen) { return ((size_t)maxlen + 4 + 32 + 15) & ~(size_t)15; }
// LDS of one decode workgroup before any staging block: the record in place
// at the end of the block's own buffer (default), read from global memory
// (grec), or in a buffer of its own.
inline size_t dec_lds_bytes(int32_t cap, uint32_t maxlen, bool inplace, bool grec) {
    return inplace ? (size_t)inplace_end(cap) + 32 : (size_t)cap + 16 + (grec ? 0 : dec_rec_bytes(maxlen));
}
// Blocks of at most this many bytes stage the EK == 0 inverse transpose
// through registers.
constexpr int kStageRegBytes = 8192;
// The EK == 0 store path (DecArgs::stage_off).  When every output is 8-aligned
// the inverse transpose is staged -- through registers for blocks of
// <= kStageRegBytes (-1), else in an LDS block of its own at the returned
// offset, when that still fits the CU's LDS (`lds` grows by it; it does not
// for blocks of some 54 KiB and more with the record in a buffer of its own,
// nor for the largest 168 bytes of block sizes in place: byte stores instead
// of a launch the runtime refuses) -- and leaves as 8-byte stores; else byte
// stores (0).  E = 1 comes here with an output that
// is 8- but not 16-byte aligned: byte stores too, the staged paths' 32-bit
// reciprocal of E has no value for 1 (2^32 wraps to 0, and every item but the
// first took group 0).
inline int32_t dec_stage_off(int ek, int E, int64_t block_bytes, int32_t cap, bool a8, size_t& lds) {
    if (ek != 0 || !a8 || E == 1) return 0;
    if (block_bytes <= kStageRegBytes) return -1;
    if (lds + (size_t)cap <= (size_t)kLdsBytes) {
        const int32_t off = (int32_t)lds;
        lds += (size_t)cap;
        return off;
    }
    return 0;
}

// ---- transposes (transpose.hip) ---------------------------------------------
constexpr int kTileGroups = 256;  // groups per 256-thread workgroup
// the register + LDS tile kernels, or the byte-granular one
inline bool transpose_fast(int E, bool a16) { return a16 && ek_size(E); }
// a tile's rows leave (arrive) as 16-byte stores (loads), or byte by byte (the
// kernels spell the same condition out)
inline bool transpose_rows16(int P, int ng) { return (P & 15) == 0 && (ng & 15) == 0; }

}  // namespace bshuf
