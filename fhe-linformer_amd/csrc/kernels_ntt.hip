// K1 — batched negacyclic NTT / INTT over RNS limbs, hand-written for gfx950 (CDNA4).
//
// Replaces (reference side): every DCRTPoly::SetFormat(EVALUATION/COEFFICIENT) executed inside
// OpenFHE underneath context->EvalMult / EvalRotate / rescale (reference call sites
// src/FHEController.cpp:423-435, :833, :843).  SURVEY.md §8(a) row K1.
//
// Function computed (bit-exact contract, same as oracle/fhe_oracle.c orc_ntt_forward):
//   forward:  out[j] = sum_i a[i] * psi^{(2*bitrev(j)+1) * i}  mod q        (natural in, bit-reversed out)
//   inverse:  the inverse map, including the N^{-1} factor               (bit-reversed in, natural out)
//
// Decomposition: N = 2^A x 256.  One transform = two kernels ("passes"), each a coalesced tile read,
// up to nine radix-2 stages done in registers/LDS, and a coalesced tile write:
//   forward : pass A (column transforms over the high A index bits, all 256 columns share 2^A-1 twiddles)
//             pass B (row transforms over the low 8 index bits, one 256-entry twiddle slice per row)
//   inverse : pass B' then pass A' (Gentleman-Sande order), N^{-1} folded into the last stage.
// A workgroup (256 threads = 4 wavefronts) owns a tile of 4096 residues; each thread keeps 16 residues
// in VGPRs and runs 4 stages on them between LDS exchanges ("rounds").  Butterflies use Shoup twiddles with an
// approximate quotient (product in [0,5q), 11 VALU instructions) and carry NO conditional subtraction for primes
// below 2^53 (value bounds proven per stage, one reduction before the final store), one mask-form conditional
// subtraction per butterfly for the 55/60-bit primes.  This is 64-bit modular-integer work: no MFMA.
//
// Memory behaviour: every global access of a wave instruction is a run of whole 128-byte lines (column pass:
// 4 row segments of 128 B; row pass: 512 B contiguous, reached through one extra LDS exchange).  The first pass can
// read out of place and strided (LimbBatch::src / src_group), which is how key switching and rescale avoid staging
// copies.  The row pass maps workgroups to (limb, tile, repetition) in XCD-contiguous order so that the 4 KiB
// twiddle slice of a (limb, tile) is shared by the vectors of a batch in one L2.
// Addressing: every global access is a workgroup-uniform 64-bit base held in SGPRs (a raw buffer descriptor per stream), one 32-bit
// lane offset per register window and a per-slot constant in the instruction's immediate / scalar offset; the LDS exchanges form one
// lane address per window and take the slot from the instruction's offset; limb, tile and vector bookkeeping runs on the scalar unit.
// Measured (profiles/): 2.11-2.17 M limb-NTT/s at N=2^16 (1.97-2.02 M before the addressing above).  A lazy
// forward pass issues 935 (columns) / 1123 (rows) VALU instructions per thread, 576 / 626 of them the butterflies' multiplies and
// 320 their other arithmetic (14 per butterfly, 9 of them 32x32 multiplies); the vector pipe is busy 79 % (columns) and 74 % (rows)
// of the time with 4 waves per SIMD - it was 88 % and 82 % - and the launches of a forward pass that fill the GPU move their tiles
// at about 5 TB/s.  2.07x algorithmic HBM traffic (two passes + twiddles).
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdlib>
#include "kernels.h"
#include "kernels_elem.h"

namespace fhelin {

namespace {

struct NttArgs {
    u64* data;
    const u64* src;     // input of this pass (== data when in place)
    const u64* tw;      // [n_limbs][2N]
    const u64* tw_rows; // [n_limbs][N/4096][15][256][2]  row-pass layout of the per-thread stages
    const u64* moduli;  // [n_limbs]
    const u64* ninv;    // [n_limbs][8]: N^-1 constants (4), lazy-reduction shift and ratio (2), spare (2)
    const int* limb_tab;
    int tab_len;
    int limb_first;
    int limb_count;
    int log_n;
    int nvec;
    int period;  // > 0: vectors v and v + period use the same limb (twiddles); used to co-schedule them
    int lazy_out;             // forward: lazy-path limbs below 2^53 skip the final reduction (LimbBatch::lazy_out)
    int src_group;            // > 0: strided first-pass input (see LimbBatch)
    size_t src_group_stride;
    int src_group2;
    size_t src_group2_stride;
    const u64* lift_qlm;      // rescale: first-pass input = centred lift of src[vec / limb_count] (LimbBatch::lift_qlm)
    int lift_limb;
    int vec0;                 // first vector of this launch: a large transform runs as chunks of vectors, both passes per chunk (launch_ntt_impl)
};

__device__ __forceinline__ size_t src_offset(const NttArgs& a, int vec, int log_n) {
    if (a.src_group > 0) {
        const int g = vec / a.src_group;
        const size_t in = (size_t)(vec % a.src_group) << log_n;
        if (a.src_group2 > 0) return (size_t)(g / a.src_group2) * a.src_group2_stride + (size_t)(g % a.src_group2) * a.src_group_stride + in;
        return (size_t)g * a.src_group_stride + in;
    }
    return (size_t)vec << log_n;
}

constexpr int TILE = 4096;
constexpr int LDS_WORDS = TILE + TILE / 16;

// tile-local element index held by thread tau in register slot k when the 4-bit register window
// sits at bit p of the index
__device__ __forceinline__ constexpr int tile_index(int tau, int k, int p) {
    return ((tau >> p) << (p + 4)) | (k << p) | (tau & ((1 << p) - 1));
}
// one pad word per 16 residues keeps every exchange pattern used below bank-conflict free
__device__ __forceinline__ constexpr int lds_slot(int e) { return e + (e >> 4); }

__device__ __forceinline__ int limb_of(const NttArgs& a, int vec) {
    return a.limb_tab ? a.limb_tab[a.tab_len ? vec % a.tab_len : vec] : a.limb_first + (vec % a.limb_count);
}

typedef u64 u64x2 __attribute__((ext_vector_type(2)));

// ---- addressing: uniform base + 32-bit lane offset + immediate -------------------------------------------
// Every global access of the tile passes is  base(vector, tile, limb, ...) + lane(tau) + K(k)  in bytes.  The base is the same
// for the whole workgroup: it is computed once as a 64-bit value, pinned to SGPRs and wrapped in a raw buffer descriptor (Stream:
// stride 0, no bound, so an access is plain base + offset).  The lane part is one unsigned byte offset (tile-local, or below
// N * 8 <= 2^20 for the automorphism scatter), formed once per window.  K depends only on the register slot k: a compile-time
// constant whose low 12 bits are the instruction's immediate and whose rest, with any further workgroup-uniform offset, is the
// instruction's scalar offset.  The result is  buffer_load/store v_lane, s[desc], s_off offen offset:imm : no vector
// instruction per access.  Only tile-local quantities go into the 32-bit parts: vec << log_n (bytes) passes 2^32 from 8192
// vectors at N = 2^16 and stays in the 64-bit base.  (Plain global accesses do not get there: with constants beyond the 13-bit
// immediate the compiler goes back to one 64-bit vector address per access.)
__device__ __forceinline__ int uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }
typedef u32 u32x2 __attribute__((ext_vector_type(2)));
typedef u32 u32x4 __attribute__((ext_vector_type(4)));
struct Stream {
    __amdgpu_buffer_rsrc_t r;
};
__device__ __forceinline__ Stream stream(const void* ubase) {
    const u64 v = reinterpret_cast<u64>(ubase);
    const u32 lo = __builtin_amdgcn_readfirstlane((u32)v), hi = __builtin_amdgcn_readfirstlane((u32)(v >> 32));
    Stream s;
    s.r = __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<void*>(((u64)hi << 32) | lo), 0, 0xffffffff, 0x00020000);
    return s;
}
// K >= 0 constant, soff >= 0 workgroup-uniform; lane + soff + K < 2^32
__device__ __forceinline__ u32 ld32(const Stream& s, u32 lane, int K, int soff = 0) {
    return __builtin_amdgcn_raw_buffer_load_b32(s.r, lane + (K & 4095), soff + (K & ~4095), 0);
}
__device__ __forceinline__ u64 ld64(const Stream& s, u32 lane, int K, int soff = 0) {
    const u32x2 v = __builtin_amdgcn_raw_buffer_load_b64(s.r, lane + (K & 4095), soff + (K & ~4095), 0);
    return ((u64)v.y << 32) | v.x;
}
__device__ __forceinline__ u64x2 ld128(const Stream& s, u32 lane, int K, int soff = 0) {
    const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(s.r, lane + (K & 4095), soff + (K & ~4095), 0);
    u64x2 r;
    r.x = ((u64)v.y << 32) | v.x;
    r.y = ((u64)v.w << 32) | v.z;
    return r;
}
__device__ __forceinline__ void st64(const Stream& s, u32 lane, int K, u64 x, int soff = 0) {
    u32x2 v;
    v.x = (u32)x;
    v.y = (u32)(x >> 32);
    __builtin_amdgcn_raw_buffer_store_b64(v, s.r, lane + (K & 4095), soff + (K & ~4095), 0);
}

// Per-limb constants of a block.
struct LimbConst {
    u64 q;
    u64 nq;   // 2^64 - q
    u64 q5;   // 5q   (lazy path: upper bound of mul_shoup_lazy5)
    u32 sh;   // lazy path: reduce_lazy_2q shift and ratio
    u32 rr;
};

// Lazy path (q < 2^53).  No conditional subtraction inside the transform: the approximate-quotient Shoup product
// returns T in [0,5q) for any 64-bit input, a forward butterfly maps (X, Y) -> (X + T, X + 5q - T), so the value bound
// grows by 5q per stage: canonical input -> < (1 + 5*17)q = 86q < 2^60 after the 17 stages of N = 2^17.  The column
// pass stores these lazy values; the row pass reduces once before its final store.
//
// Forward (Cooley-Tukey) stages for register-index bits KB_HI-1 .. KB_LO (descending).
//   gbase : global index bit that register bit 0 of the window corresponds to
//   hi    : the thread's global index bits above the window (index >> (gbase+4))
// The (up to) 15 twiddles of one round, fetched as a block so that a kernel can issue the loads of its NEXT round before
// the LDS exchange (their L2 latency then hides behind the barrier instead of sitting on the critical path).
// Stage KB uses 8 >> KB twiddles, stored at t[(8 >> KB) - 1 ...].
struct RoundTw {
    u64x2 t[15];
};
// hi = hi_u | hi_lane: its workgroup-uniform bits (the tile, row pass) and the thread's own.  One address per stage: the uniform
// part of m + (hi << (3 - kb)) is the scalar offset, the lane part is one shift, the 8 >> kb entries of a group are immediates 16 j.
template <int KB_LO, int KB_HI>
__device__ __forceinline__ void load_round_tw(RoundTw& r, const Stream& tw, int log_n, int gbase, int hi_u, u32 hi_lane) {
#pragma unroll
    for (int kb = KB_LO; kb < KB_HI; ++kb) {
        const int m = 1 << (log_n - (gbase + kb) - 1);
        const int soff = 16 * (m + (hi_u << (3 - kb)));
        const u32 lane = hi_lane << (7 - kb);   // 16 bytes x (hi_lane << (3 - kb))
#pragma unroll
        for (int j = 0; j < (8 >> kb); ++j) r.t[(8 >> kb) - 1 + j] = ld128(tw, lane, 16 * j, soff);
    }
}

// the per-thread twiddles of the row pass (global stage bits 0..3) from the transposed table: lanes read consecutive pairs;
// the 4 KiB stage stride is stepped in the scalar offset
__device__ __forceinline__ void load_round_tw_rows(RoundTw& r, const Stream& trows, int tau) {
    const u32 lane = 16u * (u32)tau;
#pragma unroll
    for (int s = 0; s < 15; ++s) r.t[s] = ld128(trows, lane, 4096 * s);
}

template <int KB, bool LAZY>
__device__ __forceinline__ void fwd_stage(u64 (&x)[16], const RoundTw& tw, const LimbConst& c) {
#pragma unroll
    for (int k0 = 0; k0 < 16; ++k0) {
        if (k0 & (1 << KB)) continue;
        const int k1 = k0 | (1 << KB);
        const u64x2 w = tw.t[(8 >> KB) - 1 + (k0 >> (KB + 1))];
        const u64 X = LAZY ? x[k0] : csub_mask(x[k0], c.q5);
#if defined(FHELIN_BFLY15)  // A/B measurement builds only (tools/build_variant.sh): the 15-instruction form
        const u64 T = mul_shoup_lazy5(x[k1], w.x, w.y, c.nq);
        x[k0] = X + T;
        x[k1] = X + c.q5 - T;
#else
        // A = X + T comes out of the multiply-add chain itself; B = X + 5q - T = (2X + 5q) - A
        const u64 A = mul_shoup_lazy5_add(x[k1], w.x, w.y, c.nq, X);
        x[k0] = A;
        x[k1] = shl1_add(X, c.q5) - A;
#endif
    }
}
template <int KB_LO, int KB_HI, bool LAZY>
__device__ __forceinline__ void fwd_round(u64 (&x)[16], const RoundTw& tw, const LimbConst& c) {
    if constexpr (KB_LO < KB_HI) {
        fwd_stage<KB_HI - 1, LAZY>(x, tw, c);
        fwd_round<KB_LO, KB_HI - 1, LAZY>(x, tw, c);
    }
}

// Lazy inverse stages: (X, Y) -> (X + Y, (X + B_s - Y) * w) with the product in [0,5q) and no conditional subtraction.
// With inputs below c_s*q at stage s of a kernel, sums stay below 2*c_s*q, so c_{s+1} = max(2*c_s, 5) and B_s = c_s*q.
// A kernel runs at most 9 stages from c_0 <= 2: c_8 = 640, every intermediate < 1280q < 2^64 for q < 2^53.
constexpr int lazy_coef(int s, int c0) { return s == 0 ? c0 : 5 << (s - 1); }  // c0 <= 2

// Inverse (Gentleman-Sande) stages for register-index bits KB_LO .. KB_HI-1 (ascending).
// If LAST, the stage at bit KB_HI-1 is the final stage of the whole transform and carries N^{-1}.
// Lazy path: S0 = stages of this kernel already done, C0 = bound coefficient of the kernel's input (see lazy_coef).
template <int KB, bool FINAL, bool LAZY, int S, int C0>
__device__ __forceinline__ void inv_stage(u64 (&x)[16], const RoundTw& tw, const LimbConst& c, const u64* __restrict__ ninv) {
    const u64 B = c.q * (u64)lazy_coef(S, C0);  // lazy path only
    if constexpr (FINAL) {
        const u64 ni = ninv[0], nis = ninv[1], wn = ninv[2], wns = ninv[3];
#pragma unroll
        for (int k0 = 0; k0 < 16; ++k0) {
            if (k0 & (1 << KB)) continue;
            const int k1 = k0 | (1 << KB);
            const u64 X = x[k0], Y = x[k1];
            if (LAZY) {
                x[k0] = csub_mask(reduce_lazy_2q(mul_shoup_lazy5(X + Y, ni, nis, c.nq), c.q, c.sh, c.rr), c.q);
                x[k1] = csub_mask(reduce_lazy_2q(mul_shoup_lazy5(X + B - Y, wn, wns, c.nq), c.q, c.sh, c.rr), c.q);
            } else {
                x[k0] = csub_mask(reduce_lazy_2q(mul_shoup_lazy5(X + Y, ni, nis, c.nq), c.q, c.sh, c.rr), c.q);
                x[k1] = csub_mask(reduce_lazy_2q(mul_shoup_lazy5(X + c.q5 - Y, wn, wns, c.nq), c.q, c.sh, c.rr), c.q);
            }
        }
    } else {
#pragma unroll
        for (int k0 = 0; k0 < 16; ++k0) {
            if (k0 & (1 << KB)) continue;
            const int k1 = k0 | (1 << KB);
            const u64x2 w = tw.t[(8 >> KB) - 1 + (k0 >> (KB + 1))];
            const u64 X = x[k0], Y = x[k1];
            if (LAZY) {
                x[k0] = X + Y;
                x[k1] = mul_shoup_lazy5(X + B - Y, w.x, w.y, c.nq);
            } else {
                x[k0] = csub_mask(X + Y, c.q5);
                x[k1] = mul_shoup_lazy5(X + c.q5 - Y, w.x, w.y, c.nq);
            }
        }
    }
}
template <int KB_LO, int KB_HI, bool LAST, bool LAZY, int S0 = 0, int C0 = 1>
__device__ __forceinline__ void inv_round(u64 (&x)[16], const RoundTw& tw, const LimbConst& c, const u64* __restrict__ ninv) {
    if constexpr (KB_LO < KB_HI) {
        inv_stage<KB_LO, (LAST && KB_LO == KB_HI - 1), LAZY, S0, C0>(x, tw, c, ninv);
        inv_round<KB_LO + 1, KB_HI, LAST, LAZY, S0 + 1, C0>(x, tw, c, ninv);
    }
}

// The slot of (tau, k) is the slot of (tau, 0) plus the slot of (0, k): the two indices share no bit, so neither the sum nor its
// pad term e >> 4 carries.  One lane address per window, the slot of (0, k) is the instruction's offset.
// the first half of an exchange: the registers of window p_from to their LDS slots, visible to the workgroup on return
__device__ __forceinline__ void park(const u64 (&x)[16], u64* lds, int tau, int p_from, bool sync_first) {
    if (sync_first) __syncthreads();
    u64* const from = lds + lds_slot(tile_index(tau, 0, p_from));
#pragma unroll
    for (int k = 0; k < 16; ++k) from[lds_slot(tile_index(0, k, p_from))] = x[k];
    __syncthreads();
}
__device__ __forceinline__ void exchange(u64 (&x)[16], u64* lds, int tau, int p_from, int p_to, bool sync_first) {
    park(x, lds, tau, p_from, sync_first);
    const u64* const to = lds + lds_slot(tile_index(tau, 0, p_to));
#pragma unroll
    for (int k = 0; k < 16; ++k) x[k] = to[lds_slot(tile_index(0, k, p_to))];
}

__device__ __forceinline__ LimbConst limb_const(const NttArgs& a, int limb) {
    LimbConst c;
    c.q = a.moduli[limb];
    c.nq = 0 - c.q;
    c.q5 = 5 * c.q;
    c.sh = (u32)a.ninv[8 * limb + 4];
    c.rr = (u32)a.ninv[8 * limb + 5];
    return c;
}
// the 52-bit scaling primes (most limbs) take the lazy path, the 60-bit special primes the semi-lazy path (one
// conditional subtraction per butterfly), the 55-bit first prime lazy forward / semi-lazy inverse; uniform per workgroup
#if defined(FHELIN_NTT_FORCE_PATH)  // ISA inspection builds only (tools/isa_count.py): 1 = lazy, 0 = classic
template <bool INVERSE> __device__ __forceinline__ bool lazy_prime(u64) { return FHELIN_NTT_FORCE_PATH; }
#else
// forward: bound 86q must fit 64 bits -> q < 2^57 (covers the 55-bit first prime too); inverse: 1280q -> q < 2^53
template <bool INVERSE> __device__ __forceinline__ bool lazy_prime(u64 q) { return q < (1ull << (INVERSE ? 53 : 57)); }
#endif

// ------------------------------------------------------------------------------------------------
// pass A: column transforms over the high A bits of the index.  Tile = 2^A rows x CW columns.
// tile-local index e = (row << LOGCW) | col ; global index j = (row << 8) | (tile*CW + col).
// ------------------------------------------------------------------------------------------------
template <int A, bool INVERSE, bool LAZY, bool LIFT>
__device__ __forceinline__ void cols_body(const NttArgs& a, u64* lds, int vec, int tile, int limb, const LimbConst& c) {
    constexpr int LOGCW = 12 - A;
    constexpr int CW = 1 << LOGCW;
    constexpr int LOGN = A + 8;
    constexpr int NFULL = A / 4;
    constexpr int REM = A % 4;
    const Stream tw = stream(reinterpret_cast<const u64x2*>(a.tw) + ((size_t)limb << LOGN));
    const Stream base = stream(a.data + ((size_t)vec << LOGN) + tile * CW);
    const Stream sbase = stream((LIFT ? a.src + ((size_t)(vec / a.limb_count) << LOGN) : a.src + src_offset(a, vec, LOGN)) + tile * CW);
    const int tau = threadIdx.x;
    u64 x[16];

    // global byte offset (relative to base) of tile-local index e.  It moves index bits, so for the window at bit p
    // goff(tile_index(tau, k, p)) = goff(tile_index(tau, 0, p)) + goff(tile_index(0, k, p)): a lane offset plus a constant
    auto goff = [](int e) constexpr { return 8 * (((e >> LOGCW) << 8) | (e & (CW - 1))); };

    if (!INVERSE) {
        // windows (in tile-index bits), top down: LOGCW+A-4, LOGCW+A-8, ..., then the remainder at LOGCW
        constexpr int P0 = LOGCW + A - 4;
        const u32 lane_in = goff(tile_index(tau, 0, P0));
#pragma unroll
        for (int k = 0; k < 16; ++k) x[k] = ld64(sbase, lane_in, goff(tile_index(0, k, P0)));
        if constexpr (LIFT) {
            // rescale: x is a coefficient modulo q_lift < 2 q (checked by the host): x mod q is one conditional subtraction,
            // the centred representative subtracts q_lift mod q where x > q_lift / 2  (== rescale_lift_kernel)
            const u64 half = a.moduli[a.lift_limb] >> 1, qlm = a.lift_qlm[limb];
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                const u64 r = csub_mask(x[k], c.q);
                x[k] = x[k] > half ? sub_mod(r, qlm, c.q) : r;
            }
        }
        RoundTw rt, rn;
        load_round_tw<0, 4>(rt, tw, LOGN, 8 + P0 - LOGCW, 0, tau >> P0);
        fwd_round<0, 4, LAZY>(x, rt, c);
        int p_prev = P0;
        if constexpr (NFULL >= 2) {
            constexpr int P1 = LOGCW + A - 8;
            load_round_tw<0, 4>(rn, tw, LOGN, 8 + P1 - LOGCW, 0, tau >> P1);
            exchange(x, lds, tau, p_prev, P1, false);
            fwd_round<0, 4, LAZY>(x, rn, c);
            p_prev = P1;
        }
        if constexpr (REM > 0) {
            constexpr int PR = LOGCW;
            load_round_tw<0, REM>(rt, tw, LOGN, 8, 0, tau >> PR);
            exchange(x, lds, tau, p_prev, PR, NFULL >= 2);
            fwd_round<0, REM, LAZY>(x, rt, c);
            p_prev = PR;
        }
        // lazy path: values up to (1 + 5A)q go to memory as they are; the row pass bounds and reduces them
        constexpr int PL = REM > 0 ? LOGCW : (NFULL >= 2 ? LOGCW + A - 8 : P0);
        (void)p_prev;
        const u32 lane_out = goff(tile_index(tau, 0, PL));
#pragma unroll
        for (int k = 0; k < 16; ++k) st64(base, lane_out, goff(tile_index(0, k, PL)), x[k]);
    } else {
        // inverse: bottom up.  full rounds at LOGCW, LOGCW+4, ...; remainder = top REM bits of the window at 8.
        // lazy path: the row pass hands over values below 2q (C0 = 2)
        const u64* ninv = a.ninv + 8 * limb;
        constexpr int P0 = LOGCW;
        const u32 lane_in = goff(tile_index(tau, 0, P0));
#pragma unroll
        for (int k = 0; k < 16; ++k) x[k] = ld64(sbase, lane_in, goff(tile_index(0, k, P0)));
        RoundTw rt, rn;
        load_round_tw<0, 4>(rt, tw, LOGN, 8, 0, tau >> P0);
        inv_round<0, 4, (NFULL == 1 && REM == 0), LAZY, 0, 2>(x, rt, c, ninv);
        int p_prev = P0;
        if constexpr (NFULL >= 2) {
            constexpr int P1 = LOGCW + 4;
            load_round_tw<0, 4>(rn, tw, LOGN, 8 + 4, 0, tau >> P1);
            exchange(x, lds, tau, p_prev, P1, false);
            inv_round<0, 4, (REM == 0), LAZY, 4, 2>(x, rn, c, ninv);
            p_prev = P1;
        }
        if constexpr (REM > 0) {
            constexpr int PR = 8;  // window covers tile bits 8..11; its top REM bits are still to do
            load_round_tw<4 - REM, 4>(rt, tw, LOGN, 8 + PR - LOGCW, 0, tau >> PR);
            exchange(x, lds, tau, p_prev, PR, NFULL >= 2);
            inv_round<4 - REM, 4, true, LAZY, 4 * NFULL, 2>(x, rt, c, ninv);
            p_prev = PR;
        }
        constexpr int PL = REM > 0 ? 8 : (NFULL >= 2 ? LOGCW + 4 : P0);
        (void)p_prev;
        const u32 lane_out = goff(tile_index(tau, 0, PL));
#pragma unroll
        for (int k = 0; k < 16; ++k) st64(base, lane_out, goff(tile_index(0, k, PL)), x[k]);
    }
}

template <int A, bool INVERSE, bool LIFT = false>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(LIFT ? 3 : 4))) void ntt_cols_kernel(NttArgs a) {
    constexpr int LOGTILES = A - 4;
    __shared__ u64 lds[LDS_WORDS];
    const int vec = a.vec0 + (blockIdx.x >> LOGTILES);
    const int tile = blockIdx.x & ((1 << LOGTILES) - 1);
    const int limb = uniform(limb_of(a, vec));   // per-workgroup values: pinned to SGPRs, never recomputed per lane
    if (limb < 0) return;
    const LimbConst c = limb_const(a, limb);
    if (lazy_prime<INVERSE>(c.q))
        cols_body<A, INVERSE, true, LIFT>(a, lds, vec, tile, limb, c);
    else
        cols_body<A, INVERSE, false, LIFT>(a, lds, vec, tile, limb, c);
}

// ------------------------------------------------------------------------------------------------
// pass B: row transforms over the low 8 bits of the index.  Tile = 16 consecutive rows of 256
// (4096 contiguous residues); tile-local index e == global index - tile*4096.
// ------------------------------------------------------------------------------------------------
// ---- product stages (NttProduct, kernels_elem.h): a key switch's inner product formed where a row pass would load it from memory - the
// special limbs as the input of the inverse row pass (product_to_lds), the Q limbs as the accumulator operand of the forward row pass's
// epilogue (epilogue_products).
// The operands of one (row, component, target limb) of a product stage, all workgroup-uniform: resolved once per workgroup by product_row
// and product_limb, read by product_sums.  OWN (the Q limbs, launch_ntt_epilogue_product): digit `own` is the ciphertext's own limb and
// component 0 may take the c0 addend; a special limb has neither.
struct ProdOperands {
    const u64* ext;     // digits of the row's input (rotation 0)
    const u64* key0;    // single key of the row (multi: sh.evk_rot)
    const u32* map0;    // its gather map, or nullptr
    int n_rot;
    int khi;            // shift that yields a key word's high half: pre-split keys (EvalKey::d_perm, folded keys) 32, keys as stored 30
    int tt, limb, comp; // digit slot, limb of modulus / key, component
    Barrett br;
    u64 qi;
    int own;            // OWN: the digit that holds limb tt
    const u64* own_src; // OWN: the own limb's vector
    u64 mont, monts;    // OWN: 2^64 mod q and its Shoup companion, applied to the own limb where own_mont
    bool own_mont;
    const u64* gsrc;    // OWN: c0's limb vector (component 0 of a gathered rotation) or nullptr; enters times (pw, pws) = P mod q
    u64 pw, pws;
};
__device__ __forceinline__ void product_row(ProdOperands& o, const NttArgs& a, const NttProduct& pr, int bi, int& in) {
    const KsShape& sh = pr.sh;
    const size_t N = (size_t)1 << a.log_n;
    const int nt = sh.ell + sh.k;
    o.ext = pr.ext;
    o.key0 = pr.evk;
    o.map0 = nullptr;
    o.n_rot = 1;
    in = bi;   // the input of batch row bi
    if (pr.multi) {
        o.ext += (size_t)bi * (sh.ext_batch_stride ? sh.ext_batch_stride : (size_t)sh.beta * nt * N);
        o.n_rot = sh.n_rot;
    } else {
        int ri = 0;
        if (sh.row_mod) {
            ri = bi % sh.row_mod;
            in = bi / sh.row_mod;
            o.ext += (size_t)in * sh.ext_batch_stride;
            o.key0 = sh.evk_row[ri];
        } else {
            if (!sh.shared_input) o.ext += (size_t)bi * sh.beta * nt * N;
            if (sh.per_row) {
                ri = bi;
                o.key0 = sh.evk_row[bi];
            }
        }
        if (sh.gather) o.map0 = sh.map_row[ri];
    }
    o.khi = pr.multi || sh.gather ? 32 : 30;
}
__device__ __forceinline__ void product_limb(ProdOperands& o, int tt, int limb, int comp, u64 q, const u64* __restrict__ barrett,
                                             const u64* __restrict__ qinv) {
    o.tt = tt;
    o.limb = limb;
    o.comp = comp;
    o.br.q = q;
    o.br.r0 = barrett[2 * limb];
    o.br.r1 = barrett[2 * limb + 1];
    o.qi = qinv[limb];
}

// byte offsets (below N * 8 <= 2^20) of the PG positions e = tau + 256 (g + i) of a tile in a limb vector, through the map where there is one
template <int PG>
__device__ __forceinline__ void product_offsets(u32 (&off)[PG], const u32* map, int tile, int g, int tau) {
    if (map) {
        const Stream ms = stream(map + ((size_t)tile << 12));
#pragma unroll
        for (int i = 0; i < PG; ++i) off[i] = 8u * ld32(ms, 4u * (u32)tau, 1024 * i, 1024 * g);
    } else {
#pragma unroll
        for (int i = 0; i < PG; ++i) off[i] = ((u32)tile << 15) + 8u * (u32)tau + 2048u * (u32)(g + i);
    }
}

// The term loop of both product stages: res[i] = the canonical residue of the inner product at tile-local position e = tau + 256 (g + i)
// (the bit-8 window: every key load of a wave is 512 contiguous bytes, every digit gather moves with whole 128-byte lines as the maps do).
// PG slots at a time carry their sums (an Acc30 and a 128-bit pair each) through the (rotation, digit) terms, with 2 PG independent loads per
// term.  Limb, row, component, key and map bookkeeping is workgroup-uniform: scalar loads, scalar branches.
// Bounds: as ks_inner_multi_kernel - keys canonical, digits canonical or below 86q (q < 2^53): a flush every 8 terms, a fold every 16.
// SHORT: at most 8 terms in all (one rotation of up to 8 digits - every plain key switch of the default chain): no flush inside the
// loops, the 128-bit pairs exist only at the end, and PG = 8 slots fit; else PG = 4.
template <int PG, bool SHORT, bool OWN>
__device__ __forceinline__ void product_sums(u64 (&res)[PG], const NttArgs& a, const NttProduct& pr, const ProdOperands& o, int tile, int g,
                                             int tau) {
    const KsShape& sh = pr.sh;
    const int log_n = a.log_n;
    const int nt = sh.ell + sh.k;
    const size_t kstride = (size_t)(sh.L1 + sh.k) << log_n;   // one evk component
    const size_t klimb = ((size_t)o.limb << log_n) + ((size_t)tile << 12);
    const u32 lane8 = 8u * (u32)tau;
    u64 lo[PG], hi[PG];
    Acc30 acc[PG];
#pragma unroll
    for (int i = 0; i < PG; ++i) {
        lo[i] = hi[i] = 0;
        acc[i] = Acc30{0, 0, 0};
    }
    int pending = 0, folded = 0;
#pragma unroll 1
    for (int r = 0; r < o.n_rot; ++r) {
        const u32* map = pr.multi ? sh.map_rot[r] : o.map0;
        const u64* key = pr.multi ? sh.evk_rot[r] : o.key0;
        const u64* dig = o.ext + (size_t)r * sh.rot_ext_stride + ((size_t)o.tt << log_n);
        u32 off[PG];
        product_offsets<PG>(off, map, tile, g, tau);
#pragma unroll 1
        for (int j = 0; j < sh.beta; ++j) {
            const bool is_own = OWN && j == o.own;
            const Stream ds = stream(is_own ? o.own_src : dig + ((size_t)j * nt << log_n));
            const Stream ks = stream(key + (size_t)(2 * j + o.comp) * kstride + klimb);
            u64 d[PG], kw[PG];
#pragma unroll
            for (int i = 0; i < PG; ++i) {
                d[i] = ld64(ds, off[i], 0);
                kw[i] = ld64(ks, lane8, 2048 * i, 2048 * g);
            }
            if constexpr (OWN) {
                if (is_own && o.own_mont) {   // the digits of this form come times 2^64 (up_hatmod_r2); the ciphertext's own limb gets the factor here
#pragma unroll
                    for (int i = 0; i < PG; ++i) d[i] = mul_shoup(d[i], o.mont, o.monts, o.br.q);
                }
            }
#pragma unroll
            for (int i = 0; i < PG; ++i) {
                u32 d0, d1;
                split30(d[i], d0, d1);
                // the key's halves without a branch: pack30 keeps the low half (below 2^30) in the low dword and the high half in
                // the high dword, a key as stored is split here
                mac30(acc[i], d0, d1, (u32)kw[i] & 0x3FFFFFFFu, (u32)(kw[i] >> o.khi));
            }
            if (!SHORT && ++pending == 8) {
                pending = 0;
                const bool fold = ++folded == 2;
                if (fold) folded = 0;
#pragma unroll
                for (int i = 0; i < PG; ++i) {
                    acc30_flush(acc[i], lo[i], hi[i]);
                    acc[i] = Acc30{0, 0, 0};
                    if (fold) {   // reduces, does not divide: the factor 2^64 stays
                        lo[i] = barrett_reduce128(lo[i], hi[i], o.br);
                        hi[i] = 0;
                    }
                }
            }
        }
    }
#pragma unroll
    for (int i = 0; i < PG; ++i) {
        acc30_flush(acc[i], lo[i], hi[i]);
        // every term carries 2^64 once: the canonical residue of the plain sum
        res[i] = redc128(lo[i], hi[i], o.br.q, o.qi);
    }
    if constexpr (OWN) {
        if (o.gsrc) {   // + P * sigma_g(c0), as ks_inner_kernel<true> adds it: the addend passes through the ModDown with the rest
            u32 off[PG];
            product_offsets<PG>(off, o.map0, tile, g, tau);
            const Stream gs = stream(o.gsrc);
#pragma unroll
            for (int i = 0; i < PG; ++i) res[i] = add_mod(res[i], mul_shoup(ld64(gs, off[i], 0), o.pw, o.pws, o.br.q), o.br.q);
        }
    }
}

// The product load stage of the inverse row pass (NttProduct, kernels_elem.h): the residue at tile-local position e = tau + 256 k becomes
// the canonical residue of the special-limb inner product at e (product_sums) and goes straight to the LDS slot that exchange(8 -> 0) would
// have written it to: the transform's sixteen registers are not live yet, and the slot groups are a real loop.
template <int PG, bool SHORT>
__device__ __forceinline__ void product_to_lds(u64* lds, const NttArgs& a, const NttProduct& pr, const u64* __restrict__ barrett,
                                               const u64* __restrict__ qinv, int vec, int tile, int limb, u64 q, int tau) {
    const KsShape& sh = pr.sh;
    const int K = sh.k;
    const int poly = uniform(vec / K), p = vec - poly * K;
    ProdOperands o;
    int in;
    product_row(o, a, pr, poly >> 1, in);
    product_limb(o, sh.ell + p, limb, poly & 1, q, barrett, qinv);
    u64* const from = lds + lds_slot(tile_index(tau, 0, 8));
#pragma unroll 1
    for (int g = 0; g < 16; g += PG) {
        u64 res[PG];
        product_sums<PG, SHORT, false>(res, a, pr, o, tile, g, tau);
        u64* const fg = from + lds_slot(tile_index(0, 1, 8)) * g;   // the slot of (0, k) is k times the slot of (0, 1) in this window
#pragma unroll
        for (int i = 0; i < PG; ++i) fg[lds_slot(tile_index(0, i, 8))] = res[i];
    }
}

// The epilogue's arithmetic and store on NK slots of the bit-8 window, slots g .. g + NK - 1 (g workgroup-uniform; all sixteen at g = 0):
// x = the transform, av = the accumulator operand at the same positions; vector = (poly, limb t) of ell limbs per poly.
template <int NK>
__device__ __forceinline__ void epilogue_finish(u64 (&x)[NK], const u64 (&av)[NK], int g, const NttEpilogue* ep, const LimbConst& c, u64 epi_b,
                                                int log_n, int tile, int tau, int poly, int t, int ell) {
    const u32 lane8 = 8u * (u32)tile_index(tau, 0, 8);
    auto koff = [](int k) constexpr { return 8 * tile_index(0, k, 8); };
    const int goff = koff(1) * g;   // slot k of this window lies k times the offset of slot 1 away
    const int bi = poly >> 1, comp = poly & 1;
    const size_t n = (size_t)1 << log_n;
    const u64 w = ep->w[2 * t], ws = ep->w[2 * t + 1];
    // av + B - x in (0, B + q): the same residue as av - x, and mul_shoup returns it canonical
#pragma unroll
    for (int k = 0; k < NK; ++k) x[k] = mul_shoup(av[k] + epi_b - x[k], w, ws, c.q);
    const u64* add = comp == 0 ? ep->add0 : ep->add1;
    if (add) {
        const Stream adds = stream(add + (size_t)bi * ep->add_stride + (size_t)t * n + ((size_t)tile << 12));
#pragma unroll
        for (int k = 0; k < NK; ++k) x[k] = add_mod(x[k], ld64(adds, lane8, koff(k), goff), c.q);
    }
    const size_t row_off = (size_t)(comp * ell + t) * n;
    const bool has_post = ep->post != nullptr;
    const Stream post = stream(ep->post + (has_post ? (size_t)bi * ep->post_stride + row_off : 0));   // read only if has_post
    const Stream out = stream(ep->out + (size_t)bi * ep->out_stride + row_off);
    const int toff = (tile << 15) + goff;   // the slots' byte offset in a row of post / out
    const u32* im = ep->per_row ? ep->invmap_row[bi] : ep->invmap;
    if (im) {   // rotation: through the inverse automorphism map; a target index is below N, its byte offset below 2^20
        const Stream ims = stream(im + ((size_t)tile << 12));
#pragma unroll
        for (int k = 0; k < NK; ++k) {
            const u32 j8 = 8u * ld32(ims, 4u * (u32)tau, 4 * tile_index(0, k, 8), goff >> 1);
            u64 r = x[k];
            if (has_post) r = add_mod(r, ld64(post, j8, 0), c.q);
            st64(out, j8, 0, r);
        }
    } else {
        if (has_post) {
#pragma unroll
            for (int k = 0; k < NK; ++k) x[k] = add_mod(x[k], ld64(post, lane8, koff(k), toff), c.q);
        }
#pragma unroll
        for (int k = 0; k < NK; ++k) st64(out, lane8, koff(k), x[k], toff);
    }
}

// what a forward row pass whose epilogue forms its own accumulator operand needs besides the epilogue (launch_ntt_epilogue_product)
struct ProdTabs {
    const NttProduct* pr;
    const u64* barrett;
    const u64* qinv;
    const u64* mont;
};

// The epilogue over a product stage: the transform x sits in LDS (park(x, 0): the layout exchange(0 -> 8) reads), and per group of PG slots the
// Q-limb sums of the key switch are formed (product_sums, operands as ks_inner_kernel<GATHER> takes them), the group's x comes back from LDS in
// the bit-8 window and the epilogue finishes and stores the group.  Nothing of the transform is live in registers during the sums.
template <int PG, bool SHORT>
__device__ __forceinline__ void epilogue_products(const u64* lds, const NttArgs& a, const NttEpilogue* ep, const ProdTabs& pt, const LimbConst& c,
                                                  u64 epi_b, bool reduce_x, int tile, int tau, int poly, int t, int ell) {
    const NttProduct& pr = *pt.pr;
    const KsShape& sh = pr.sh;
    const int log_n = a.log_n;
    const int bi = poly >> 1, comp = poly & 1;
    ProdOperands o;
    int in;
    product_row(o, a, pr, bi, in);
    product_limb(o, t, t, comp, c.q, pt.barrett, pt.qinv);   // Q limb t: digit slot t, key and modulus limb t
    o.own = t / sh.alpha;
    // the polynomial of the row's input: as ks_inner_kernel offsets c_ntt
    const int cin = sh.row_mod ? in : sh.shared_input ? 0 : bi;
    o.own_src = pr.c_ntt + (size_t)cin * sh.c_stride + ((size_t)t << log_n);
    o.own_mont = !sh.gather;
    o.mont = pt.mont[2 * t];
    o.monts = pt.mont[2 * t + 1];
    o.gsrc = nullptr;
    o.pw = o.pws = 0;
    if (sh.gather && sh.gsrc_pmod && comp == 0) {
        o.gsrc = sh.gsrc + (size_t)in * sh.gsrc_stride + ((size_t)t << log_n);
        o.pw = sh.gsrc_pmod[2 * t];
        o.pws = sh.gsrc_pmod[2 * t + 1];
    }
    const u64* const to = lds + lds_slot(tile_index(tau, 0, 8));
#pragma unroll 1
    for (int g = 0; g < 16; g += PG) {
        u64 av[PG], x[PG];
        product_sums<PG, SHORT, true>(av, a, pr, o, tile, g, tau);
        const u64* const tg = to + lds_slot(tile_index(0, 1, 8)) * g;   // the slot of (0, k) is k times the slot of (0, 1) in this window
#pragma unroll
        for (int i = 0; i < PG; ++i) x[i] = tg[lds_slot(tile_index(0, i, 8))];
        if (reduce_x) {
#pragma unroll
            for (int i = 0; i < PG; ++i) x[i] = reduce_lazy_2q(x[i], c.q, c.sh, c.rr);
        }
        epilogue_finish<PG>(x, av, g, ep, c, epi_b, log_n, tile, tau, poly, t, ell);
    }
}

// PROD: an operand is not loaded but formed by a product stage.  Inverse: the input - product_to_lds has left it in LDS, as the first half of
// exchange(8 -> 0) would have.  Forward (with EPI): the epilogue's accumulator operand (epilogue_products, pt).
template <bool INVERSE, bool LAZY, bool EPI, bool PROD = false>
__device__ __forceinline__ void rows_body(const NttArgs& a, u64* lds, int vec, int tile, int limb, const LimbConst& c,
                                          const NttEpilogue* ep, const ProdTabs* pt = nullptr) {
    const int log_n = a.log_n;
    const Stream tw = stream(reinterpret_cast<const u64x2*>(a.tw) + ((size_t)limb << log_n));
    const Stream trows = stream(reinterpret_cast<const u64x2*>(a.tw_rows) + (((size_t)limb << (log_n - 12)) + tile) * (15 * 256));
    [[maybe_unused]] u64* const vbase = a.data + ((size_t)vec << log_n) + ((size_t)tile << 12);
    const Stream base = stream(vbase);
    const Stream sbase = stream(a.src + src_offset(a, vec, log_n) + ((size_t)tile << 12));
    const int tau = threadIdx.x;
    // lane byte offsets of the bit-4 and bit-8 windows; slot k adds the constant 8 * (k << p): 128 k and 2048 k
    const u32 lane4 = 8u * (u32)tile_index(tau, 0, 4), lane8 = 8u * (u32)tile_index(tau, 0, 8);
    auto koff = [](int k, int p) constexpr { return 8 * tile_index(0, k, p); };
    u64 x[16];

    if (!INVERSE) {
#pragma unroll
        for (int k = 0; k < 16; ++k) x[k] = ld64(sbase, lane4, koff(k, 4));
        RoundTw rt, rn;
        load_round_tw<0, 4>(rt, tw, log_n, 4, tile << 4, tau >> 4);
        fwd_round<0, 4, LAZY>(x, rt, c);
        load_round_tw_rows(rn, trows, tau);                          // per-thread twiddles of the last four stages
        exchange(x, lds, tau, 4, 0, false);
        fwd_round<0, 4, LAZY>(x, rn, c);
        // epilogue operand, read at the store offsets (bit-8 window) now so that its latency hides behind the reduction and
        // the exchange below
        [[maybe_unused]] u64 av[16];
        [[maybe_unused]] int ell = 0, t = 0, poly = 0;
        if constexpr (EPI) {
            ell = ep->ell;
            poly = uniform(vec / ell);
            t = vec - poly * ell;
        }
        if constexpr (EPI && !PROD) {
            const Stream acc = stream(ep->acc + (size_t)poly * ep->acc_poly_stride + ((size_t)t << log_n) + ((size_t)tile << 12));
#pragma unroll
            for (int k = 0; k < 16; ++k) av[k] = ld64(acc, lane8, koff(k, 8));
        }
        // Epilogue: x only feeds av + B - x into mul_shoup, which takes ANY 64-bit input and returns the canonical residue.  So x
        // needs no reduction of its own where a multiple B = cq of q bounds it and av + B < 2^64 (av < q): from a canonical input
        // (every epilogue transform takes the canonical output of a basis conversion or of the lift) the lazy path proves x < 86q
        // and runs for q < 2^57 (87q < 2^64); the semi-lazy path proves x < 10q, and 11q < 2^64 for q < 2^60.  Same residue class,
        // hence the same canonical bytes.  Any larger prime keeps the reduction to [0, 2q).
        [[maybe_unused]] u64 epi_b = 0;
        if constexpr (EPI) {
            if (LAZY) {
                epi_b = 86 * c.q;
            } else if (c.q < (1ull << 60)) {
                epi_b = 10 * c.q;
            } else {
                epi_b = 2 * c.q;
                if constexpr (!PROD) {   // PROD: per slot group, where x comes back from LDS
#pragma unroll
                    for (int k = 0; k < 16; ++k) x[k] = reduce_lazy_2q(x[k], c.q, c.sh, c.rr);
                }
            }
        } else if (!(LAZY && a.lazy_out && c.q < (1ull << 53))) {
#pragma unroll
            for (int k = 0; k < 16; ++k)
                x[k] = csub_mask(reduce_lazy_2q(x[k], c.q, c.sh, c.rr), c.q);   // from < 86q (lazy) or < 10q (semi-lazy)
        }
#if defined(FHELIN_ROWS_DIRECT_STORE)   // A/B builds only: 16-byte stores straight from the bit-0 window (128-byte lane stride), no exchange
        if constexpr (!EPI) {
#pragma unroll
            for (int k = 0; k < 16; k += 2) {
                u64x2 v;
                v.x = x[k];
                v.y = x[k + 1];
                reinterpret_cast<u64x2*>(vbase + 16 * tau)[k >> 1] = v;
            }
            return;
        }
#endif
        // window at bit 0 leaves 16 consecutive residues per thread (128-byte lane stride); one more LDS exchange
        // to the bit-8 window makes every store instruction a contiguous 512-byte wave access
        if constexpr (EPI && PROD) {
            park(x, lds, tau, 0, true);
            const bool reduce_x = !LAZY && c.q >= (1ull << 60);
            if (pt->pr->sh.beta <= 8)
                epilogue_products<8, true>(lds, a, ep, *pt, c, epi_b, reduce_x, tile, tau, poly, t, ell);
            else
                epilogue_products<4, false>(lds, a, ep, *pt, c, epi_b, reduce_x, tile, tau, poly, t, ell);
        } else {
            exchange(x, lds, tau, 0, 8, true);
            if constexpr (EPI) {
                epilogue_finish<16>(x, av, 0, ep, c, epi_b, log_n, tile, tau, poly, t, ell);
            } else {
#pragma unroll
                for (int k = 0; k < 16; ++k) st64(base, lane8, koff(k, 8), x[k]);
            }
        }
    } else {
        // coalesced load through the bit-8 window, then an LDS exchange to the bit-0 window of the first GS round
        RoundTw rt, rn;
        if constexpr (PROD) {
            load_round_tw_rows(rt, trows, tau);
            __syncthreads();
            const u64* const to = lds + lds_slot(tile_index(tau, 0, 0));
#pragma unroll
            for (int k = 0; k < 16; ++k) x[k] = to[lds_slot(tile_index(0, k, 0))];
        } else {
#pragma unroll
            for (int k = 0; k < 16; ++k) x[k] = ld64(sbase, lane8, koff(k, 8));
            load_round_tw_rows(rt, trows, tau);                      // per-thread twiddles of the first four stages
            exchange(x, lds, tau, 8, 0, false);
        }
        inv_round<0, 4, false, LAZY, 0, 1>(x, rt, c, nullptr);
        load_round_tw<0, 4>(rn, tw, log_n, 4, tile << 4, tau >> 4);
        exchange(x, lds, tau, 0, 4, true);
        inv_round<0, 4, false, LAZY, 4, 1>(x, rn, c, nullptr);
        if (LAZY) {  // sums have grown to < 640q: hand values below 2q to the column pass
#pragma unroll
            for (int k = 0; k < 16; ++k) x[k] = reduce_lazy_2q(x[k], c.q, c.sh, c.rr);
        }
#pragma unroll
        for (int k = 0; k < 16; ++k) st64(base, lane4, koff(k, 4), x[k]);
    }
}

// Block -> (vector, tile) map of the row pass.  A row tile needs its own 4 KiB twiddle slice per (limb, tile); vectors of the same
// limb (the two polys of a ciphertext, the rows of a batch) reuse it.  Blocks b and b+8 share an XCD (L2), so
// each XCD gets a contiguous range of logical ids, ordered (limb, tile, repetition): the slice is fetched once
// per XCD instead of once per block.  Placement affects speed only.
__device__ __forceinline__ void rows_block(const NttArgs& a, int& vec, int& tile) {
    const int logtiles = a.log_n - 12;
    int lid = blockIdx.x;
    const int nblk = gridDim.x;
    if ((nblk & 7) == 0) lid = (lid & 7) * (nblk >> 3) + (lid >> 3);
    if (a.period > 0) {
        const int nper = a.nvec / a.period;
        const int rep = lid % nper, r = lid / nper;
        tile = r & ((1 << logtiles) - 1);
        vec = a.vec0 + rep * a.period + (r >> logtiles);
    } else {
        vec = a.vec0 + (lid >> logtiles);
        tile = lid & ((1 << logtiles) - 1);
    }
    vec = uniform(vec);   // per-workgroup values: pinned to SGPRs, never recomputed per lane
    tile = uniform(tile);
}

template <bool INVERSE, bool EPI = false>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4))) void ntt_rows_kernel(NttArgs a, NttEpilogue ep) {
    __shared__ u64 lds[LDS_WORDS];
    int vec, tile;
    rows_block(a, vec, tile);
    const int limb = uniform(limb_of(a, vec));
    if (limb < 0) return;
    const LimbConst c = limb_const(a, limb);
    if (lazy_prime<INVERSE>(c.q))
        rows_body<INVERSE, true, EPI>(a, lds, vec, tile, limb, c, &ep);
    else
        rows_body<INVERSE, false, EPI>(a, lds, vec, tile, limb, c, &ep);
}

// The inverse row pass over the special-limb products of a key switch (NttProduct).  Vectors are (row, component, special limb) with
// the limb fastest, so the period of the block map is k and its repetitions are (row, component): component b and component a of one
// (row, limb, tile), which gather the same digit tile, are neighbours in one XCD's share.
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4))) void ntt_rows_product_kernel(NttArgs a, NttProduct pr, const u64* barrett,
                                                                                                        const u64* qinv) {
    __shared__ u64 lds[LDS_WORDS];
    int vec, tile;
    rows_block(a, vec, tile);
    const int limb = uniform(limb_of(a, vec));
    const LimbConst c = limb_const(a, limb);
    if ((pr.multi ? pr.sh.n_rot : 1) * pr.sh.beta <= 8)
        product_to_lds<8, true>(lds, a, pr, barrett, qinv, vec, tile, limb, c.q, threadIdx.x);
    else
        product_to_lds<4, false>(lds, a, pr, barrett, qinv, vec, tile, limb, c.q, threadIdx.x);
    if (lazy_prime<true>(c.q))
        rows_body<true, true, false, true>(a, lds, vec, tile, limb, c, nullptr);
    else
        rows_body<true, false, false, true>(a, lds, vec, tile, limb, c, nullptr);
}

// The epilogue row pass of a ModDown's NTT(conv) over the Q-limb products of its key switch (launch_ntt_epilogue_product): ntt_rows_kernel<false,
// true> with the accumulator operand formed in place of loaded.  Vectors are (row, component, Q limb) with the limb fastest: as above, the two
// components of one (row, limb, tile) are neighbours in one XCD's share.
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4))) void ntt_rows_epilogue_product_kernel(NttArgs a, NttEpilogue ep, NttProduct pr,
                                                                                                                 const u64* barrett, const u64* qinv,
                                                                                                                 const u64* mont) {
    __shared__ u64 lds[LDS_WORDS];
    int vec, tile;
    rows_block(a, vec, tile);
    const int limb = uniform(limb_of(a, vec));
    const LimbConst c = limb_const(a, limb);
    const ProdTabs pt{&pr, barrett, qinv, mont};
    if (lazy_prime<false>(c.q))
        rows_body<false, true, true, true>(a, lds, vec, tile, limb, c, &ep, &pt);
    else
        rows_body<false, false, true, true>(a, lds, vec, tile, limb, c, &ep, &pt);
}

template <int A>
void launch_cols(const NttArgs& a, bool inverse, int blocks, hipStream_t s) {
    if (inverse)
        hipLaunchKernelGGL((ntt_cols_kernel<A, true>), dim3(blocks), dim3(256), 0, s, a);
    else if (a.lift_qlm)
        hipLaunchKernelGGL((ntt_cols_kernel<A, false, true>), dim3(blocks), dim3(256), 0, s, a);
    else
        hipLaunchKernelGGL((ntt_cols_kernel<A, false>), dim3(blocks), dim3(256), 0, s, a);
}

}  // namespace

// which = ROWS_PRODUCT: only the inverse row pass, its input formed from *prod; COLS_ONLY: only the inverse column pass;
// forward with ep and prod: the epilogue's accumulator operand formed from *prod
enum NttPasses { BOTH_PASSES, ROWS_PRODUCT, COLS_ONLY };
static void launch_ntt_impl(const DeviceTables& t, const LimbBatch& b, bool inverse, const NttEpilogue* ep, hipStream_t s,
                            NttPasses which = BOTH_PASSES, const NttProduct* prod = nullptr);

void launch_ntt(const DeviceTables& t, const LimbBatch& b, bool inverse, hipStream_t s) { launch_ntt_impl(t, b, inverse, nullptr, s); }
void launch_ntt_epilogue(const DeviceTables& t, const LimbBatch& b, const NttEpilogue& ep, hipStream_t s) {
    launch_ntt_impl(t, b, false, &ep, s);
}
void launch_ntt_rows_product(const DeviceTables& t, const LimbBatch& b, const NttProduct& p, hipStream_t s) {
    launch_ntt_impl(t, b, true, nullptr, s, ROWS_PRODUCT, &p);
}
void launch_ntt_cols_inverse(const DeviceTables& t, const LimbBatch& b, hipStream_t s) { launch_ntt_impl(t, b, true, nullptr, s, COLS_ONLY); }
void launch_ntt_epilogue_product(const DeviceTables& t, const LimbBatch& b, const NttEpilogue& ep, const NttProduct& p, hipStream_t s) {
    // the product stage takes Q limb t for vector (poly, t): b is the dense [poly][ell] batch of a ModDown (Evaluator::moddown checks)
    launch_ntt_impl(t, b, false, &ep, s, BOTH_PASSES, &p);
}

static void launch_ntt_impl(const DeviceTables& t, const LimbBatch& b, bool inverse, const NttEpilogue* ep, hipStream_t s, NttPasses which,
                            const NttProduct* prod) {
    if (b.nvec <= 0) return;
    NttArgs a;
    a.data = b.data;
    a.src = b.src ? b.src : b.data;
    a.src_group = b.src ? b.src_group : 0;
    a.src_group_stride = b.src_group_stride;
    a.src_group2 = (b.src && b.src_group > 0) ? b.src_group2 : 0;
    a.src_group2_stride = b.src_group2_stride;
    a.lazy_out = (!inverse && b.lazy_out) ? 1 : 0;
    a.lift_qlm = (!inverse && b.src && b.lift_limb >= 0) ? b.lift_qlm : nullptr;
    a.lift_limb = b.lift_limb;
    a.tw = inverse ? t.tw_inv : t.tw_fwd;
    a.tw_rows = inverse ? t.tw_rows_inv : t.tw_rows_fwd;
    a.moduli = t.moduli;
    a.ninv = t.ninv;
    a.limb_tab = b.limb_tab;
    a.tab_len = b.tab_len;
    a.limb_first = b.limb_first;
    a.limb_count = b.limb_count > 0 ? b.limb_count : 1;
    a.log_n = t.log_n;
    a.nvec = b.nvec;
    const int per = b.limb_tab ? b.tab_len : a.limb_count;
    a.period = (per > 0 && per < b.nvec && b.nvec % per == 0) ? per : 0;
    const int A = t.log_n - 8;
    a.vec0 = 0;
    // FHELIN_NTT_CHUNK_MB=<m> (experiment, default off): a large transform as CHUNKS of about m MiB of vectors, both tile passes per chunk,
    // so that the intermediate a chunk's first pass writes is still in the 256 MiB Infinity Cache when its second pass reads it.
    // Measured in round 4 (profiles/r04_q_*): SLOWER - 274 -> 284 / 293 / 316 ms per pass at 96 / 64 / 32 MiB, micro-benchmark 1.97 -> 1.69 M
    // limb-NTT/s: the extra launch boundaries (every launch drains before the next starts) cost more than HBM round trips of the
    // intermediate do, i.e. the tile passes are not waiting on HBM.  Chunks are multiples of the twiddle period (vectors v and
    // v + period share a limb) so that the block order of the row pass keeps working inside a chunk.
    static const int chunk_mb = [] {
        const char* e = std::getenv("FHELIN_NTT_CHUNK_MB");
        return e ? std::atoi(e) : 0;
    }();
    int chunk = b.nvec;
    if (chunk_mb > 0 && !ep && which == BOTH_PASSES) {
        const size_t vec_bytes = (size_t)8 << t.log_n;
        const int want = (int)std::max<size_t>(1, ((size_t)chunk_mb << 20) / vec_bytes);
        if (b.nvec > want + want / 2) {
            const int per = a.period > 0 ? a.period : 1;
            chunk = std::max(per, want / per * per);
        }
    }
    const int nvec_all = b.nvec, period_all = a.period;
    const u64* src_all = a.src;
    const int sg = a.src_group, sg2 = a.src_group2;
    for (int v0 = 0; v0 < nvec_all; v0 += chunk) {
        a.vec0 = v0;
        a.nvec = std::min(chunk, nvec_all - v0);
        a.period = (period_all > 0 && a.nvec % period_all == 0 && a.nvec > period_all) ? period_all : 0;
        a.src = src_all;
        a.src_group = sg;
        a.src_group2 = sg2;
        const int blocks = a.nvec << (t.log_n - 12);
        auto cols = [&]() {
            switch (A) {
                case 4: launch_cols<4>(a, inverse, blocks, s); break;
                case 5: launch_cols<5>(a, inverse, blocks, s); break;
                case 6: launch_cols<6>(a, inverse, blocks, s); break;
                case 7: launch_cols<7>(a, inverse, blocks, s); break;
                case 8: launch_cols<8>(a, inverse, blocks, s); break;
                case 9: launch_cols<9>(a, inverse, blocks, s); break;
                default: break;
            }
        };
        // the first pass may read out of place; the second always works in place on `data`
        if (!inverse) {
            cols();
            a.src = a.data;
            a.src_group = 0;
            a.src_group2 = 0;
            if (ep && prod)
                hipLaunchKernelGGL(ntt_rows_epilogue_product_kernel, dim3(blocks), dim3(256), 0, s, a, *ep, *prod, t.barrett, t.qinv, t.mont);
            else if (ep)
                hipLaunchKernelGGL((ntt_rows_kernel<false, true>), dim3(blocks), dim3(256), 0, s, a, *ep);
            else
                hipLaunchKernelGGL((ntt_rows_kernel<false, false>), dim3(blocks), dim3(256), 0, s, a, NttEpilogue());
        } else {
            if (which == ROWS_PRODUCT) {
                hipLaunchKernelGGL(ntt_rows_product_kernel, dim3(blocks), dim3(256), 0, s, a, *prod, t.barrett, t.qinv);
                continue;
            }
            if (which != COLS_ONLY) hipLaunchKernelGGL((ntt_rows_kernel<true, false>), dim3(blocks), dim3(256), 0, s, a, NttEpilogue());
            a.src = a.data;
            a.src_group = 0;
            a.src_group2 = 0;
            cols();
        }
    }
}

}  // namespace fhelin
