// lz4_fast.hip -- the opt-in fast LZ4 parse ("fast parse v1").
//
// The block's payload is a valid LZ4 block that every bitshuffle/LZ4 reader
// decodes, but not the reference encoder's bytes: matches are looked for only
// at the fixed distances {1, 2, 3, 4, 8, P, 2P} (P = bytes per bit plane of the
// block), where nearly all of a bit-transposed block's redundancy sits.  No
// hash table, no LDS atomics, no lane-ordered exchange:
//
//   A  bit transpose of the block into LDS (as k_lz4_encode);
//   B  per offset d, the bitmap "byte q equals byte q - d" (q >= d, q < n - 5:
//      the cap of LZ4's last-literals rule), 32 positions per lane and step:
//      XOR against the shifted window, zero-byte test;
//   C  the bitmap of positions where some offset runs >= 4 bytes
//      (m & m>>1 & m>>2 & m>>3, OR over the offsets), cut to 1 <= p <= n - 12
//      (in registers for 8 KiB blocks of E = 1, 2, 4, else an eighth LDS bitmap);
//   D  the serial selection, wave-uniform: next set bit of C at or after ip
//      (a window of 64 words per step), then per offset the first
//      zero bit of its bitmap at or after p -- offset j on lanes 8j .. 8j+7, one
//      word each, so 256 positions per round trip -- the longest run wins, ties
//      to the smaller offset; the sequence's bytes leave at once with wave-wide
//      copies, so there is no descriptor buffer to flush.  The measure step's
//      first window is read together with the search's, and the literals'
//      first 64 bytes together with the measure step's: two LDS round trips per
//      sequence, often one.
//
// One wave per block; the record [BE32 c][payload] and its foot word land in
// k_lz4_encode's scratch-slot layout, so the offset scan, k_compact and
// k_encode_finish[_batch] run unchanged behind it.
#include <hip/hip_runtime.h>

#include "enc_common.h"
#include "launch.h"

namespace bshuf {

namespace {

constexpr int kFrontPad = 16;  // LDS in front of the block: the windows of q - d < 0
constexpr int kBackPad = 16;
constexpr int kOffsets = 7;    // bitmap slots 0..6: d = 1, 2, 3, 4, 8, P, 2P; slot 7: match starts

__device__ __forceinline__ uint32_t bits_from(int lo) {
    return lo >= 32 ? 0u : (lo <= 0 ? ~0u : ~0u << lo);
}
// bits [lo, hi) of a word (any lo, hi)
__device__ __forceinline__ uint32_t bit_range(int lo, int hi) { return bits_from(lo) & ~bits_from(hi); }

// 0x80 in every non-zero byte of x
__device__ __forceinline__ uint32_t nz_flags(uint32_t x) {
    return (((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x) & 0x80808080u;
}
// bits 0..3: bytes 0..3 of xa are non-zero, bits 4..7: those of xb.  One
// (quarter-rate) multiply gathers both dwords' flags: flag 8i (xa) and 8i + 4
// (xb) times 2^(21 - 7i) land on bits 21 + i and 25 + i, and no other partial
// product falls on bits 21..28 or on one another (no carries).
__device__ __forceinline__ uint32_t nz8(uint32_t xa, uint32_t xb) {
    const uint32_t c = (nz_flags(xa) >> 7) | (nz_flags(xb) >> 3);
    return ((c * 0x00204081u) >> 21) & 0xFFu;
}

// x[2 + k] = dword k of a 32-byte word of the block, x[0], x[1] the 8 bytes in front
template <int d>
__device__ __forceinline__ uint32_t eq_near(const uint32_t (&x)[10]) {
    uint32_t df[8];
#pragma unroll
    for (int k = 0; k < 8; k++) {
        uint32_t sh;
        if constexpr (d < 4)
            sh = __builtin_amdgcn_alignbyte(x[2 + k], x[1 + k], (uint32_t)(4 - d));
        else if constexpr (d == 4)
            sh = x[1 + k];
        else
            sh = x[k];
        df[k] = x[2 + k] ^ sh;
    }
    return ~(nz8(df[0], df[1]) | (nz8(df[2], df[3]) << 8) | (nz8(df[4], df[5]) << 16) |
             (nz8(df[6], df[7]) << 24));
}

__device__ __forceinline__ uint32_t eq_far(const lds8* D, int base, const uint32_t (&x)[10], int d) {
    uint32_t df[8];
#pragma unroll
    for (int k = 0; k < 8; k++) {
        const int a = base + 4 * k;
        // always loaded (a branch per window would wait for each load alone);
        // windows wholly below d read the bytes in front of the block and are
        // masked by the caller
        df[k] = x[2 + k] ^ lds_rd32(D, max(a - d, -4));
    }
    return ~(nz8(df[0], df[1]) | (nz8(df[2], df[3]) << 8) | (nz8(df[4], df[5]) << 16) |
             (nz8(df[6], df[7]) << 24));
}

// LDS written by some lanes, read by others: the workgroup is ONE wave, whose
// LDS accesses execute in order, so the compiler's ordering is all it takes.
// (__syncthreads() would also wait for every outstanding global access: the
// record's stores and the next block's prefetch.)
__device__ __forceinline__ void lds_handoff() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// minimum over the lane's group of 8 (lanes 8j .. 8j+7), in every lane of it
__device__ __forceinline__ int group_min8(int v) {
    v = min(v, __builtin_amdgcn_update_dpp(v, v, 0xB1, 0xF, 0xF, false));   // quad_perm [1,0,3,2]
    v = min(v, __builtin_amdgcn_update_dpp(v, v, 0x4E, 0xF, 0xF, false));   // quad_perm [2,3,0,1]
    v = min(v, __builtin_amdgcn_update_dpp(v, v, 0x141, 0xF, 0xF, false));  // row_half_mirror
    return v;
}

// The emitters' loops step the whole wave (uniform trip count, lanes past the
// end masked) and stay rolled: they sit on the selection's serial chain, where
// the set-up of an unrolled per-lane loop costs more than it saves.

// the length bytes behind a 15 nibble: v / 255 bytes of 255, then v % 255
__device__ __forceinline__ void put_len(gbl8* o, int& op, int v, int lane) {
    const int nfull = (int)((uint32_t)v / 255u);
#pragma nounroll
    for (int i0 = 0; i0 <= nfull; i0 += kWave) {
        const int i = i0 + lane;
        if (i <= nfull) o[op + i] = (uint8_t)(i < nfull ? 255 : v - 255 * nfull);
    }
    op += nfull + 1;
}

// literals [from + first, from + ll) (the bytes before `first` are the caller's)
__device__ __forceinline__ void put_literals(gbl8* o, int& op, const lds8* D, int from, int ll, int first,
                                             int lane) {
    // four bytes per lane and LDS round trip (loads clamped into the run)
#pragma nounroll
    for (int i0 = first; i0 < ll; i0 += 4 * kWave) {
        const int i = i0 + lane;
        uint8_t v[4];
#pragma unroll
        for (int u = 0; u < 4; u++) v[u] = D[from + min(i + u * kWave, ll - 1)];
#pragma unroll
        for (int u = 0; u < 4; u++)
            if (i + u * kWave < ll) o[op + i + u * kWave] = v[u];
    }
    op += ll;
}

// SREG: the compact LDS layout of blocks up to 8 KiB with E = 1, 2, 4 -- the
// seven equality bitmaps, then the block, nothing else (15,360 B at 8 KiB: 10
// blocks per CU instead of 9).  The match-start bitmap lives in registers (word
// w in lane w % 64, register w / 64), reads below the block fall into the
// bitmaps' tail (their bits are masked), and a block the register transpose
// does not take (a partial last block) is transposed straight from HBM.
static_assert(kSregWords == 4 * kWave, "dispatch.h: the match-start bitmap's four registers");
template <int EK, bool SREG>
__global__ __launch_bounds__(64) void k_lz4_encode_fast(EncArgs a, int64_t nb, int nw_max) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const int lane = threadIdx.x;
    const int E = EK ? EK : a.L.E;
    lds8* const D = to_lds(smem) + (SREG ? 4 * kOffsets * nw_max : kFrontPad);
    // (not SREG: raw bytes of a staged transpose, then the bitmaps)
    lds8* const U = SREG ? to_lds(smem) : D + 32 * nw_max + kBackPad;
    lds32* const U32 = (lds32*)U;
    const bool batch = a.segs != nullptr;

    for (int64_t blk = blockIdx.x; blk < nb; blk += gridDim.x) {
        // block -> (elements, source): one stream, or a batch of streams
        int m;
        const uint8_t* src;
        if (!batch) {
            m = blk < a.L.nfull ? a.L.bs : a.L.last;
            src = a.in + blk * (int64_t)a.L.bs * E;
        } else {
            const Seg& g = a.segs[a.blk_seg[blk + a.blk0]];
            const int64_t k = blk + a.blk0 - g.first;
            m = k < g.nfull ? a.L.bs : g.last;
            src = g.in + k * (int64_t)a.L.bs * E;
        }
        const int n = m * E;
        const int P = m / 8;
        const int nw = (n + 31) >> 5;
        lds_handoff();  // the previous block's LDS is dead

        // ---- A: bit transpose into LDS (bshuf_trans_bit_elem)
        bool done = false;
        if constexpr (EK != 0) {
            constexpr int kRegGroups4 = BlockRegs4<EK>::kIters * kWave * 4;
            static_assert(kRegGroups4 == enc_reg_groups4(EK), "dispatch.h names the registers' capacity");
            if (P % 4 == 0 && P <= kRegGroups4) {
                BlockRegs4<EK> R4;
                issue_block_loads4<EK>(R4, src, P, lane);
                transpose4s_regs_to_lds<EK>(R4, D, P, lane);
                done = true;
            }
        }
        if (!done && SREG) {
            for (int i = lane; i < P * E; i += kWave) {
                const int g = i / E, b = i - g * E;
                uint64_t v = 0;
#pragma unroll
                for (int k = 0; k < 8; k++) v |= (uint64_t)src[(int64_t)(8 * g + k) * E + b] << (8 * k);
                v = tr8x8(v);
#pragma unroll
                for (int j = 0; j < 8; j++) D[(8 * b + j) * P + g] = (uint8_t)(v >> (8 * j));
            }
        } else if (!done) {
            if (((uintptr_t)src & 7) == 0) {
                for (int i = lane; i < n / 8; i += kWave) ((lds64v*)U)[i] = ((const gbl64c*)src)[i];
            } else {
                for (int i = lane; i < n; i += kWave) U[i] = src[i];
            }
            lds_handoff();
            // lane = (group g, byte b) with b fastest
            const uint32_t magic = (uint32_t)((0x100000000ull + (uint64_t)E - 1) / (uint64_t)E);
            for (int i = lane; i < P * E; i += kWave) {
                // (E = 1: the magic does not fit 32 bits)
                const int g = E == 1 ? i : (int)__umulhi((uint32_t)i, magic), b = i - g * E;
                const lds8* x = U + 8 * g * E + b;
                uint64_t v = 0;
#pragma unroll
                for (int k = 0; k < 8; k++) v |= (uint64_t)x[k * E] << (8 * k);
                v = tr8x8(v);
#pragma unroll
                for (int j = 0; j < 8; j++) D[(8 * b + j) * P + g] = (uint8_t)(v >> (8 * j));
            }
        }
        lds_handoff();

        gbl8* const rec = (gbl8*)(a.scratch + blk * a.slot);
        gbl8* const o = rec + 4;
        int op = 0, anchor = 0;

        if (n >= kLz4MinLength) {
            // offsets P and 2P when they are not among 1, 2, 3, 4, 8 already
            const int dP = (P <= 4 || P == 8) ? 0 : P;
            const int d2P = (P == 1 || P == 2 || P == 4) ? 0 : 2 * P;
            const int cap = n - kLastLiterals;  // equality bits end here

            // ---- B: capped equality bitmaps, one 32-position word per lane and step
            for (int w = lane; w < nw; w += kWave) {
                const int base = 32 * w;
                const lds8* B = D + base;
                // Word 0 reads the 8 bytes in FRONT of the block here (and eq_far
                // up to 4): the front pad, or in the SREG layout the tail of bitmap
                // slot 6, which other lanes are writing in this very phase.  Those
                // bytes are undefined.  They only ever stand for s[q - d] with
                // q < d, and every such bit is cleared by bit_range(d - base, ..)
                // below: keep that lower bound if the masks ever change.
                const u32x2 pv = *(const lds64v*)(B - 8);
                const u32x4 c0 = *(const lds128*)B, c1 = *(const lds128*)(B + 16);
                const uint32_t x[10] = {pv.x, pv.y, c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, c1.z, c1.w};
                const int hi = cap - base;
                U32[0 * nw + w] = eq_near<1>(x) & bit_range(1 - base, hi);
                U32[1 * nw + w] = eq_near<2>(x) & bit_range(2 - base, hi);
                U32[2 * nw + w] = eq_near<3>(x) & bit_range(3 - base, hi);
                U32[3 * nw + w] = eq_near<4>(x) & bit_range(4 - base, hi);
                U32[4 * nw + w] = eq_near<8>(x) & bit_range(8 - base, hi);
                U32[5 * nw + w] = dP ? eq_far(D, base, x, dP) & bit_range(dP - base, hi) : 0u;
                U32[6 * nw + w] = d2P ? eq_far(D, base, x, d2P) & bit_range(d2P - base, hi) : 0u;
            }
            lds_handoff();
            // ---- C: positions 1 .. n - 12 where some offset runs >= 4 bytes
            auto starts = [&](int w) {
                uint32_t s = 0;
                const uint32_t more = w + 1 < nw ? ~0u : 0u;  // (the last slot's last word + 1: valid LDS, masked)
#pragma unroll
                for (int j = 0; j < kOffsets; j++) {
                    const uint32_t c = U32[j * nw + w];
                    const uint32_t nx = U32[j * nw + w + 1] & more;
                    const uint64_t v = (uint64_t)c | ((uint64_t)nx << 32);
                    s |= (uint32_t)(v & (v >> 1) & (v >> 2) & (v >> 3));
                }
                return s & bit_range(1 - 32 * w, n - kMfLimit + 1 - 32 * w);
            };
            uint32_t sreg[4] = {0u, 0u, 0u, 0u};
            if constexpr (SREG) {
#pragma unroll
                for (int i = 0; i < 4; i++)
                    if (lane + kWave * i < nw) sreg[i] = starts(lane + kWave * i);
            } else {
                for (int w = lane; w < nw; w += kWave) U32[kOffsets * nw + w] = starts(w);
                lds_handoff();
            }

            // ---- D: serial selection (everything but the lanes' words is wave-uniform)
            const int j = lane >> 3, k = lane & 7;
            const int dj = j == 0 ? 1 : j == 1 ? 2 : j == 2 ? 3 : j == 3 ? 4 : j == 4 ? 8 : j == 5 ? dP : j == 6 ? d2P : 0;
            const lds32* const Cj = U32 + (j < kOffsets ? j : 0) * nw;
            const lds32* const S = U32 + kOffsets * nw;
            int ip = 1;
            for (;;) {
                // next match start at or after ip
                int p = -1;
                const int wip = ip >> 5;
                // the measure step's first window, read beside the search's: it
                // is the right one when the match starts within 8 words of ip
                const uint32_t cw = Cj[min(wip + k, nw - 1)];
                // (SREG: windows aligned to the registers' 64 words)
                for (int w0 = SREG ? wip & ~(kWave - 1) : wip; w0 < nw; w0 += kWave) {
                    const int w = w0 + lane;
                    uint32_t s;
                    if constexpr (SREG) {
                        const int t = w0 >> 6;
                        s = t == 0 ? sreg[0] : t == 1 ? sreg[1] : t == 2 ? sreg[2] : sreg[3];
                        if (w < wip) s = 0;
                    } else {
                        s = S[min(w, nw - 1)];
                        if (w >= nw) s = 0;
                    }
                    if (w == wip) s &= ~0u << (ip & 31);
                    const uint64_t bal = ballot(s != 0);
                    if (bal) {
                        const int fl = ffs64(bal);
                        const uint32_t word = (uint32_t)__builtin_amdgcn_readlane((int)s, fl);
                        p = 32 * (w0 + fl) + (__ffs(word) - 1);
                        break;
                    }
                }
                if (p < 0) break;
                p = uni(p);
                // the first 64 literals: read now, stored behind the measure step
                const int ll = p - anchor;
                const uint32_t lit0 = D[anchor + min(lane, max(ll - 1, 0))];
                // per offset (lane group), the end of its run from p
                int run = 0;
                bool found = false;
                const int wp = p >> 5;
                bool have = wp < wip + 8;
                for (int wb = have ? wip : wp;; wb += 8) {
                    const int w = wb + k;
                    uint32_t c = have ? cw : Cj[min(w, nw - 1)];
                    have = false;
                    if (dj == 0 || w >= nw) c = 0;
                    uint32_t inv = w < wp ? 0u : ~c;
                    if (w == wp) inv &= ~0u << (p & 31);
                    const int e = group_min8(inv ? 32 * w + (__ffs(inv) - 1) : 0x7FFFFFFF);
                    if (!found && e != 0x7FFFFFFF) {
                        run = e - p;
                        found = true;
                    }
                    if (ballot(!found) == 0) break;
                }
                // longest run, ties to the smaller offset (run < 65536, d < 65536)
                const uint32_t key = ((uint32_t)run << 16) | (0xFFFFu - (uint32_t)dj);
                uint32_t best = 0;
#pragma unroll
                for (int g = 0; g < kOffsets; g++)
                    best = max(best, (uint32_t)__builtin_amdgcn_readlane((int)key, 8 * g));
                const int len = (int)(best >> 16);
                const int d = (int)(0xFFFFu - (best & 0xFFFFu));
                if (len < kMinMatch) break;  // cannot happen (p has a run >= 4); keeps ip moving

                // the sequence: token, literal length, literals, offset, match length
                const int ml = len - kMinMatch;
                if (lane == 0) o[op] = (uint8_t)((min(ll, 15) << 4) | min(ml, 15));
                op += 1;
                if (ll >= 15) put_len(o, op, ll - 15, lane);
                if (lane < ll) o[op + lane] = (uint8_t)lit0;
                put_literals(o, op, D, anchor, ll, kWave, lane);
                if (lane < 2) o[op + lane] = (uint8_t)(d >> (8 * lane));
                op += 2;
                if (ml >= 15) put_len(o, op, ml - 15, lane);
                anchor = ip = p + len;
            }
        }
        // last sequence: literals [anchor, n)
        {
            const int ll = n - anchor;
            if (lane == 0) o[op] = (uint8_t)(min(ll, 15) << 4);
            op += 1;
            if (ll >= 15) put_len(o, op, ll - 15, lane);
            put_literals(o, op, D, anchor, ll, 0, lane);
        }
        if (lane < 4) rec[lane] = (uint8_t)((uint32_t)op >> (24 - 8 * lane));
        if (lane == 0) a.foot[blk] = 4 + (uint64_t)op;
    }
}

template <int EK, bool SREG>
hipError_t launch_fast_t(const EncArgs& a, int64_t nb, hipStream_t s) {
    const int64_t nmax = (int64_t)a.L.bs * a.L.E;
    if (!fast_applies(nmax)) return hipErrorInvalidValue;
    const int nw_max = (int)((nmax + 31) >> 5);
    // (E = 8 stays in the 8-slot layout: its SREG instance compiled to 170
    // VGPRs = 2 waves per SIMD = 8 blocks per CU by the compiler's report, below
    // the 9 the 8-slot layout's LDS allows at its 160 VGPRs / 3 waves per SIMD;
    // read from the report, not timed)
    if constexpr (EK != 0 && EK != 8 && !SREG) {
        // whole words, the block 16-aligned behind the bitmaps
        if (fast_sreg(EK, nmax)) return launch_fast_t<EK, true>(a, nb, s);
    }
    // SREG: 7 bitmap slots + block; else front pad + block (whole words) + back
    // pad + 8 bitmap slots
    const size_t lds = SREG ? (size_t)(4 * kOffsets + 32) * nw_max
                            : kFrontPad + 32 * (size_t)nw_max + kBackPad + 32 * (size_t)nw_max;
    auto fn = k_lz4_encode_fast<EK, SREG>;
    if (lds > 65536) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(fn),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    const int64_t grid = std::min<int64_t>(nb, (int64_t)1 << 22);
    ProfScope prof("k_lz4_encode_fast", s);
    hipLaunchKernelGGL(fn, dim3((unsigned)grid), dim3(kWave), lds, s, a, nb, nw_max);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_encode_fast(const EncArgs& a, int64_t nb, int ek, hipStream_t s) {
    if (nb <= 0) return hipSuccess;
    switch (ek) {
        case 1: return launch_fast_t<1, false>(a, nb, s);
        case 2: return launch_fast_t<2, false>(a, nb, s);
        case 4: return launch_fast_t<4, false>(a, nb, s);
        case 8: return launch_fast_t<8, false>(a, nb, s);
        default: return launch_fast_t<0, false>(a, nb, s);
    }
}

}  // namespace bshuf
