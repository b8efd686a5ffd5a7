// enc_common.h -- what the exact LZ4 encoder (lz4_encode.hip) and the fast one
// (lz4_fast.hip) share: the kernel arguments of one parse launch and the
// fused load + bit transpose of an 8 KiB block into LDS.
#pragma once

#include "launch.h"

namespace bshuf {

struct EncArgs {
    const uint8_t* in;
    uint8_t* scratch;
    uint64_t* foot;
    int64_t slot;
    Layout L;
    int32_t desc_ok;   // LDS holds kDescBytes of sequence descriptors at D + desc_off
    int32_t desc_off;
    const Seg* segs;   // batch: per-stream table (nullptr: the single stream in/L)
    const uint32_t* blk_seg;
    int32_t raw8;      // EK == 0: every block source is 8-aligned (LDS-staged transpose)
    int64_t blk0;      // batch: global index of this launch's block 0 (pipelined segments)
    uint32_t* tickets; // this launch's ticket counters (launch.h); nullptr: static schedule
    int32_t steal;     // a wave whose ticket shard has run out draws from the others
#ifdef BSHUF_DIAG
    int32_t diag_slot; // this launch's slot of the per-shard finish table
#endif
};

// Registers holding one 8 KiB block for EK-byte elements: 8192 / 64 lanes.
template <int EK>
struct BlockRegs {
    static constexpr int kIters = EK ? 8192 / (kWave * 8 * EK) : 1;  // 64-group iterations
    uint32_t w[kIters][2 * (EK ? EK : 1)];
};

template <int EK>
__device__ __forceinline__ void issue_block_loads(BlockRegs<EK>& R, const uint8_t* src, int P,
                                                  int lane) {
#pragma unroll
    for (int it = 0; it < BlockRegs<EK>::kIters; it++) {
        const int g = it * kWave + lane;
        if (g < P) load_group<EK>(src + (int64_t)g * 8 * EK, R.w[it]);
    }
}

template <int EK>
__device__ __forceinline__ void transpose_regs_to_lds(const BlockRegs<EK>& R, lds8* D, int P,
                                                      int g0, int lane) {
#pragma unroll
    for (int it = 0; it < BlockRegs<EK>::kIters; it++) {
        const int g = g0 + it * kWave + lane;
        if (g < P) {
#pragma unroll
            for (int b = 0; b < EK; b++) {
                const uint64_t v = tr8x8(gather_byte_plane<EK>(R.w[it], b));
#pragma unroll
                for (int j = 0; j < 8; j++) D[(8 * b + j) * P + g] = (uint8_t)(v >> (8 * j));
            }
        }
    }
}

// 4-groups-per-lane variant (P % 4 == 0): lane q owns groups 4q..4q+3, i.e.
// 32*EK contiguous input bytes, and writes ONE dword per plane to LDS.
template <int EK>
struct BlockRegs4 {
    static constexpr int kIters = (EK ? 8192 / (kWave * 32 * EK) : 1) > 0
                                      ? (EK ? 8192 / (kWave * 32 * EK) : 1) : 1;
    uint32_t w[kIters][4][2 * (EK ? EK : 1)];
};

template <int EK>
__device__ __forceinline__ void issue_block_loads4(BlockRegs4<EK>& R, const uint8_t* src, int P,
                                                   int lane) {
    const int P4 = P >> 2;
#pragma unroll
    for (int it = 0; it < BlockRegs4<EK>::kIters; it++) {
        const int q = it * kWave + lane;
        if (q < P4) {
#pragma unroll
            for (int k = 0; k < 4; k++) load_group<EK>(src + ((int64_t)q * 4 + k) * 8 * EK, R.w[it][k]);
        }
    }
}

template <int EK>
__device__ __forceinline__ void transpose4_regs_to_lds(const BlockRegs4<EK>& R, lds8* D, int P,
                                                       int lane) {
    const int P4 = P >> 2;
    lds32* D32 = (lds32*)D;
#pragma unroll
    for (int it = 0; it < BlockRegs4<EK>::kIters; it++) {
        const int q = it * kWave + lane;
        if (q < P4) {
            uint32_t pl[8 * EK];
#pragma unroll
            for (int r = 0; r < 8 * EK; r++) pl[r] = 0;
#pragma unroll
            for (int k = 0; k < 4; k++) {
#pragma unroll
                for (int b = 0; b < EK; b++) {
                    const uint64_t v = tr8x8(gather_byte_plane<EK>(R.w[it][k], b));
#pragma unroll
                    for (int j = 0; j < 8; j++)
                        pl[8 * b + j] |= (uint32_t)((v >> (8 * j)) & 0xFFu) << (8 * k);
                }
            }
#pragma unroll
            for (int r = 0; r < 8 * EK; r++) D32[r * P4 + q] = pl[r];
        }
    }
}

// The same, bit-sliced over the lane's four groups at once (A/B variant bit
// 262144): x[8b + i] gathers byte b of element i of all four groups (byte k =
// group k, three v_perm_b32), one 8x8 bit transpose per byte lane across those
// eight registers (untranspose4_rows: the transpose is its own inverse) leaves
// x[8b + j] = plane 8b + j of the four groups -- ONE dword per plane as above.
#ifndef BSHUF_TR_SOFF
#define BSHUF_TR_SOFF 1
#endif
template <int EK>
__device__ __forceinline__ void transpose4s_regs_to_lds(const BlockRegs4<EK>& R, lds8* D, int P,
                                                        int lane) {
    const int P4 = P >> 2;
    lds32* D32 = (lds32*)D;
#pragma unroll
    for (int it = 0; it < BlockRegs4<EK>::kIters; it++) {
        const int q = it * kWave + lane;
        if (q < P4) {
            uint32_t x[8 * EK];
#pragma unroll
            for (int b = 0; b < EK; b++) {
#pragma unroll
                for (int i = 0; i < 8; i++) {
                    const int o = i * EK + b, d = o >> 2;
                    const uint32_t sel = (uint32_t)(o & 3) | ((uint32_t)(4 + (o & 3)) << 8) | 0x0C0C0000u;
                    const uint32_t lo = __builtin_amdgcn_perm(R.w[it][1][d], R.w[it][0][d], sel);
                    const uint32_t hi = __builtin_amdgcn_perm(R.w[it][3][d], R.w[it][2][d], sel);
                    x[8 * b + i] = __builtin_amdgcn_perm(hi, lo, 0x05040100u);
                }
            }
            untranspose4_rows<EK>(x);
            // plane r's dword of this lane at Dq + r * rs: the row offsets are
            // wave-uniform (scalar multiplies), not per-lane 64-bit mads
            lds8* const Dq = D + 4 * q;
            const int rs = 4 * P4;
            int ro = 0;
#pragma unroll
            for (int r = 0; r < 8 * EK; r++) {
                *(lds32*)(Dq + ro) = x[r];
                ro += rs;
                // E >= 4: an opaque scalar (one v_add per row instead of a
                // 64-bit v_mad per row; 1 GiB G2 -2.2 %, E = 2 measured flat or
                // worse beside the pipelined lane_runs, profiles/r06/enc_ab)
                if constexpr (BSHUF_TR_SOFF && EK >= 4) asm volatile("" : "+s"(ro));
            }
        }
    }
}

// Fast parse v1 (lz4_fast.hip) of blocks 0 .. nb-1 of `a` into their scratch
// slots and foot words, in k_lz4_encode's layout.  ek: the element size when
// every block source is 16-aligned and E is 1, 2, 4 or 8, else 0.
hipError_t launch_encode_fast(const EncArgs& a, int64_t nb, int ek, hipStream_t s);

}  // namespace bshuf
