// Client-side work on the GPU: CKKS encoding and public-key encryption of whole batches.
//
// Reference side: FHEController::encode / encrypt / read_expanded_input (reference src/FHEController.cpp:348-385,
// :623-650) run one MakeCKKSPackedPlaintext + Encrypt per input on the host; a sample of the Linformer driver has 194
// inputs (src/main.cpp:159-173).  Here the inverse special FFT (fp64), the scaling / rounding to integers, the sampling of
// the encryption randomness and the final dyadic combination run as batched kernels over [vectors][...] arrays.
//
//  * fft_special_inv_stage_kernel : one radix-2 stage of the inverse special FFT (canonical embedding restricted to <5>),
//    bit-identical to the host loop in client.cpp ckks_fft_special(inverse): IEEE double operations in the same order,
//    contraction to FMA switched off.
//  * encode_round_reduce_kernel   : bit-reversal, 1/n scaling, (long double)v * Delta exactly as the x87 host code rounds
//    it (64-bit significand, round-to-nearest-even), round-half-away to an integer, residues modulo every limb.
//  * sample_small_kernel          : ChaCha20 (RFC 8439 block function) keyed per call; ternary {-1,0,1} or rounded
//    Gaussian (sigma 3.19, Box-Muller) coefficients written as residues of every limb.
//  * encrypt_combine_kernel       : c0 = b*u + e0 + m, c1 = a*u + e1 (NTT form) for a batch.
//  * sample_flood_kernel          : uniform coefficients on [-2^B, 2^B) (noise flooding), optionally plus the rounded Gaussian,
//    as residues of every limb (|f| may exceed q_l: reduced with the limb's Barrett constants).
//  * rerandomize_combine_kernel   : out = in + (b*u + w, a*u + e1) on the first out_ell limbs of a batch of ciphertexts of any limb
//    counts (a fresh encryption of zero added, the level drop part of the same pass).
//  * phase_batch_kernel, decode_lift_kernel, fft_special_fwd_tile_kernel / _stage_kernel, decode_gather_kernel : batched decryption
//    (Client::decrypt_batch): the phase of a batch of any shapes, the centred CRT lift and the division by the scale in integer code
//    (decode_lift.h), the forward special FFT bit-identical to the host loop, and the slots that were asked for in one buffer.
// All HBM-bound or trivially small; no MFMA.
#include <hip/hip_runtime.h>
#include "kernels.h"
#include "kernels_client.h"
#include "kernels_chacha.h"
#include "decode_lift.h"

namespace fhelin {
namespace {

typedef u64 u64x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ Barrett load_barrett(const DeviceTables& t, int limb) {
    Barrett b;
    b.q = t.moduli[limb];
    b.r0 = t.barrett[2 * limb];
    b.r1 = t.barrett[2 * limb + 1];
    return b;
}

// the same for a limb index that is uniform but a loop counter, in a kernel that stores between the loads: the constants are vector
// loads then, and this brings them back to scalar registers
__device__ __forceinline__ u64 uniform64(u64 x) {
    return ((u64)(u32)__builtin_amdgcn_readfirstlane((int)(u32)(x >> 32)) << 32) | (u32)__builtin_amdgcn_readfirstlane((int)(u32)x);
}
__device__ __forceinline__ Barrett load_barrett_uniform(const DeviceTables& t, int limb) {
    Barrett b = load_barrett(t, limb);
    b.q = uniform64(b.q);
    b.r0 = uniform64(b.r0);
    b.r1 = uniform64(b.r1);
    return b;
}

// ---- interleaved samples (include/fhelin.h "Interleaved samples"): the PHYSICAL slot vectors of a chunk from staged logical ones, in
// front of the inverse special FFT.  out [n_vec][slots << log_stride]: physical slot p holds logical slot p >> log_stride of lane
// p & (stride - 1); in [n_vec][lanes][slots] with lanes = stride (one vector per sample) or 1 (one vector replicated into every lane:
// model plaintexts, masks).  grid ((slots << log_stride) / 256 rounded up, n_vec): consecutive threads write consecutive physical slots.
__global__ __launch_bounds__(256) void interleave_slots_kernel(double2* __restrict__ out, const double2* __restrict__ in, int slots,
                                                               int log_stride, int lanes) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    const int phys = slots << log_stride;
    if (p >= phys) return;
    const int lane = lanes == 1 ? 0 : p & ((1 << log_stride) - 1);
    out[(size_t)blockIdx.y * phys + p] = in[((size_t)blockIdx.y * lanes + lane) * slots + (p >> log_stride)];
}

// ---- inverse special FFT, one stage.  data [n_vec][size] (re, im) pairs; grid (size/2 / 256, n_vec)
#pragma clang fp contract(off)
__global__ __launch_bounds__(256) void fft_special_inv_stage_kernel(double2* data, const u32* rot, const double2* ksi, int size, int len) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= size / 2) return;
    double2* v = data + (size_t)blockIdx.y * size;
    const int lenh = len >> 1, lenq = len << 2, gap = (4 * size) / lenq;
    const int j = t % lenh, i = (t / lenh) * len;
    const int idx = (lenq - (int)(rot[j] % (u32)lenq)) * gap;
    const double2 a = v[i + j], b = v[i + j + lenh], k = ksi[idx];
    const double dr = a.x - b.x, di = a.y - b.y;
    double2 u, w;
    u.x = a.x + b.x;
    u.y = a.y + b.y;
    w.x = dr * k.x - di * k.y;   // (dr + i di)(k.x + i k.y), each product and sum rounded separately like the host code
    w.y = dr * k.y + di * k.x;
    v[i + j] = u;
    v[i + j + lenh] = w;
}

// |v| * s with v a double and s = ms * 2^es a positive long double (64-bit significand): the product rounded to a 64-bit
// significand (round to nearest even), then rounded half away from zero to an integer -> magnitude as (lo, hi)
__device__ __forceinline__ void x87_mul_round(double v, u64 ms, int es, u64& lo, u64& hi, bool& neg) {
    const u64 bits = (u64)__double_as_longlong(v);
    neg = (bits >> 63) != 0;
    const int ex = (int)((bits >> 52) & 0x7FF);
    u64 mv = bits & 0xFFFFFFFFFFFFFull;
    lo = hi = 0;
    if (ex == 0 && mv == 0) return;             // +-0
    int ev;
    if (ex == 0) ev = -1074;                     // subnormal
    else {
        mv |= 1ull << 52;
        ev = ex - 1075;
    }
    // P = mv * ms < 2^117
    u64 plo = mv * ms, phi = __umul64hi(mv, ms);
    // significant bits of P
    const int nb = phi ? 128 - __clzll((long long)phi) : 64 - __clzll((long long)plo);
    int E = ev + es;                             // value = P * 2^E
    u64 q;                                       // 64-bit significand after the first rounding
    if (nb > 64) {
        const int sh = nb - 64;                  // 1..53
        q = (plo >> sh) | (phi << (64 - sh));
        const u64 rem = plo & ((1ull << sh) - 1), half = 1ull << (sh - 1);
        if (rem > half || (rem == half && (q & 1))) {
            ++q;
            if (q == 0) {                        // carried out of 64 bits
                q = 1ull << 63;
                ++E;
            }
        }
        E += sh;
    } else {
        q = plo;                                 // exact in 64 bits
    }
    // round q * 2^E half away from zero to an integer (|result| < 2^127 for every scale this library uses)
    if (E >= 0) {
        if (E >= 64) {
            hi = q << (E - 64);
            lo = 0;
        } else if (E == 0) {
            lo = q;
        } else {
            lo = q << E;
            hi = q >> (64 - E);
        }
    } else {
        const int t = -E;
        if (t > 64) return;                      // below 1/2
        if (t == 64) {
            lo = q >> 63;                        // >= 1/2 rounds to 1
            return;
        }
        lo = q >> t;
        if ((q >> (t - 1)) & 1) {
            ++lo;
            if (lo == 0) hi = 1;
        }
    }
}

// grid (N/256, n_vec): thread = coefficient position n of vector b.  fftdata [n_vec][slots] is the output of the stage
// kernels (before bit reversal and 1/n scaling); out [n_vec][ell][N] residues (coefficient form).  Row l is reduced modulo limb
// l < ell_q ? l : L1 + (l - ell_q): the first ell_q rows are chain limbs, the rest follow from limb id L1 (the special limbs of a
// limb-sliced encoding, launch_encode_round_reduce_split); ell_q == ell: row l is limb l
__global__ __launch_bounds__(256) void encode_round_reduce_kernel(DeviceTables t, u64* out, const double2* fftdata, int slots, int log_slots,
                                                                  int ell, int ell_q, int L1, u64 ms, int es, double inv_n) {
    const size_t N = (size_t)1 << t.log_n;
    const size_t n = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t gapc = (N / 2) / slots;
    u64* o = out + (size_t)blockIdx.y * ell * N + n;
    const size_t half = N / 2;
    const size_t pos = n < half ? n : n - half;
    if (pos % gapc != 0) {
        for (int l = 0; l < ell; ++l) o[(size_t)l * N] = 0;
        return;
    }
    const u32 i = (u32)(pos / gapc);
    const u32 src = __brev(i) >> (32 - log_slots);     // bit_reverse(v): element i comes from position bitrev(i)
    const double2 c = fftdata[(size_t)blockIdx.y * slots + src];
    double val;
    {
#pragma clang fp contract(off)
        val = (n < half ? c.x : c.y) * inv_n;
    }
    u64 lo, hi;
    bool neg;
    x87_mul_round(val, ms, es, lo, hi, neg);
    for (int l = 0; l < ell; ++l) {
        const Barrett br = load_barrett(t, l < ell_q ? l : L1 + (l - ell_q));
        const u64 h = barrett_reduce128(hi, 0, br);
        u64 r = barrett_reduce128(lo, h, br);
        if (neg) r = neg_mod(r, br.q);
        o[(size_t)l * N] = r;
    }
}

// grid (N/8/256, n_poly): one ChaCha20 block = 8 coefficients per thread.  out [n_poly][ell][N] residues (coefficient form)
// kind 0: rounded Gaussian sigma 3.19 (Box-Muller on 53-bit uniforms); kind 1: uniform ternary
__global__ __launch_bounds__(256) void sample_small_kernel(DeviceTables t, u64* out, SamplerKey key, u64 stream_base, int kind, int ell) {
    const size_t N = (size_t)1 << t.log_n;
    const size_t blk = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (blk >= N / 8) return;
    u64 r[8];
    chacha20_block(key, blk, stream_base + blockIdx.y, r);
    int v[8];
    if (kind == 1) {
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = (int)__umul64hi(r[i], 3) - 1;
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const double u1 = ((double)(r[2 * i] >> 11) + 1.0) * (1.0 / 9007199254740992.0);   // (0, 1]
            const double u2 = (double)(r[2 * i + 1] >> 11) * (1.0 / 9007199254740992.0);       // [0, 1)
            const double rad = sqrt(-2.0 * log(u1)) * 3.19, th = 6.283185307179586476925 * u2;
            double sn, cs;
            sincos(th, &sn, &cs);
            v[2 * i] = (int)llrint(rad * cs);
            v[2 * i + 1] = (int)llrint(rad * sn);
        }
    }
    u64* o = out + (size_t)blockIdx.y * ell * N + blk * 8;
    for (int l = 0; l < ell; ++l) {
        const u64 q = t.moduli[l];
        u64x2* dst = reinterpret_cast<u64x2*>(o + (size_t)l * N);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            u64x2 w;
            w.x = v[2 * i] < 0 ? q - (u64)(-v[2 * i]) : (u64)v[2 * i];
            w.y = v[2 * i + 1] < 0 ? q - (u64)(-v[2 * i + 1]) : (u64)v[2 * i + 1];
            dst[i] = w;
        }
    }
}

// grid (N/512, n_vec * ell): ct [n_vec][2][ell][N] <- (pk_b * u + e0 + m, pk_a * u + e1); pk [2][L1][N]
__global__ __launch_bounds__(256) void encrypt_combine_kernel(DeviceTables t, u64* ct, const u64* pk, const u64* u, const u64* e0, const u64* e1,
                                                              const u64* m, int ell, int L1, size_t m_stride) {
    const int b = blockIdx.y / ell, l = blockIdx.y % ell;
    const Barrett br = load_barrett(t, l);
    const size_t row = ((size_t)1 << t.log_n) >> 1;
    const size_t n2 = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t in = ((size_t)b * ell + l) * row + n2;
    const u64x2 uu = reinterpret_cast<const u64x2*>(u)[in];
    const u64x2 a0 = reinterpret_cast<const u64x2*>(e0)[in], a1 = reinterpret_cast<const u64x2*>(e1)[in];
    const u64x2 mm = reinterpret_cast<const u64x2*>(m + (size_t)b * m_stride)[(size_t)l * row + n2];
    const u64x2 kb = reinterpret_cast<const u64x2*>(pk)[(size_t)l * row + n2];
    const u64x2 ka = reinterpret_cast<const u64x2*>(pk)[((size_t)L1 + l) * row + n2];
    u64x2 c0, c1;
    c0.x = add_mod(add_mod(mul_mod(kb.x, uu.x, br), a0.x, br.q), mm.x, br.q);
    c0.y = add_mod(add_mod(mul_mod(kb.y, uu.y, br), a0.y, br.q), mm.y, br.q);
    c1.x = add_mod(mul_mod(ka.x, uu.x, br), a1.x, br.q);
    c1.y = add_mod(mul_mod(ka.y, uu.y, br), a1.y, br.q);
    u64x2* C = reinterpret_cast<u64x2*>(ct);
    C[((size_t)(2 * b) * ell + l) * row + n2] = c0;
    C[((size_t)(2 * b + 1) * ell + l) * row + n2] = c1;
}

// grid (N/8/256, n_poly): one ChaCha20 block = 8 coefficients per thread, as sample_small_kernel.  Coefficient i of polynomial p is
// f_i = (W >> (63 - B)) - 2^B with W word i % 8 of block i / 8 of stream stream_base + p: uniform on [-2^B, 2^B), 1 <= B <= 62.
// gauss: plus the rounded Gaussian of sample_small_kernel kind 0 drawn from the block of stream gauss_stream_base + p (e0 + f as one
// polynomial).  out [n_poly][ell][N] residues f_i mod q_l in [0, q_l) (coefficient form)
__global__ __launch_bounds__(256, 8) void sample_flood_kernel(DeviceTables t, u64* __restrict__ out, SamplerKey key, u64 stream_base,
                                                           u64 gauss_stream_base, int flood_bits, int gauss, int ell) {
    const size_t N = (size_t)1 << t.log_n;
    const size_t blk = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (blk >= N / 8) return;
    u64 r[8];
    u32 g[2] = {0, 0};   // the Gaussian terms (|e| <= 28: sigma 3.19 times the radius of a 53-bit uniform) packed as eight int8
    if (gauss) {   // first, and one pair at a time: the double-precision pairs are what the register count is made of
        chacha20_block(key, blk, gauss_stream_base + blockIdx.y, r);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const double u1 = ((double)(r[2 * i] >> 11) + 1.0) * (1.0 / 9007199254740992.0);   // (0, 1]
            const double u2 = (double)(r[2 * i + 1] >> 11) * (1.0 / 9007199254740992.0);       // [0, 1)
            const double rad = sqrt(-2.0 * log(u1)) * 3.19, th = 6.283185307179586476925 * u2;
            double sn, cs;
            sincos(th, &sn, &cs);
            g[i >> 1] |= (((u32)(int)llrint(rad * cs) & 0xFFu) | (((u32)(int)llrint(rad * sn) & 0xFFu) << 8)) << (16 * (i & 1));
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    // the thread's position formed again from an opaque copy of its index: nothing but the packed Gaussian terms lives across the
    // double-precision code above (what the compiler otherwise keeps there, it spills)
    u32 tid = threadIdx.x;
    asm volatile("" : "+v"(tid));
    const size_t pos = (size_t)blockIdx.x * 256 + tid;
    chacha20_block(key, pos, stream_base + blockIdx.y, r);
    const int sh = 63 - flood_bits;
    const long long off = 1ll << flood_bits;
    u32 neg = 0;   // bit i: coefficient i is negative; r[i] becomes its magnitude (|f + e| < 2^62 + 2^5)
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const long long v = (long long)(r[i] >> sh) - off + (int)(signed char)(g[i >> 2] >> (8 * (i & 3)));
        neg |= (v < 0 ? 1u : 0u) << i;
        r[i] = v < 0 ? (u64)(-v) : (u64)v;
    }
    u64* o = out + (size_t)blockIdx.y * ell * N + pos * 8;
    for (int l = 0; l < ell; ++l) {
        const Barrett br = load_barrett_uniform(t, l);
        u64x2* dst = reinterpret_cast<u64x2*>(o + (size_t)l * N);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            // one reduction at a time: interleaved, the eight cost 128 registers
            const u64 ra = barrett_reduce128(r[2 * i], 0, br);
            u64x2 w;
            w.x = (neg >> (2 * i)) & 1 ? neg_mod(ra, br.q) : ra;
            __builtin_amdgcn_sched_barrier(0);
            const u64 rb = barrett_reduce128(r[2 * i + 1], 0, br);
            w.y = (neg >> (2 * i + 1)) & 1 ? neg_mod(rb, br.q) : rb;
            dst[i] = w;
            __builtin_amdgcn_sched_barrier(0);
        }
    }
}

// grid (N/512, out_ell, n_ct): item b = tab[blockIdx.z] is a ciphertext in [2][in_ell][N] with in_ell >= out_ell; its first out_ell
// limbs plus a fresh public-key encryption of zero go to out [2][out_ell][N]:
//   out0[l] = in0[l] + pk_b[l] u + w,  out1[l] = in1[l] + pk_a[l] u + e1      u, w, e1 [n_ct][out_ell][N], pk [2][L1][N], all NTT form
__global__ __launch_bounds__(256) void rerandomize_combine_kernel(DeviceTables t, const RerandItem* __restrict__ tab, const u64* __restrict__ pk,
                                                                  const u64* __restrict__ u, const u64* __restrict__ w,
                                                                  const u64* __restrict__ e1, int out_ell, int L1) {
    const int b = blockIdx.z, l = blockIdx.y;
    const RerandItem it = tab[b];
    const Barrett br = load_barrett(t, l);
    const size_t row = ((size_t)1 << t.log_n) >> 1;
    const size_t n2 = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t rnd = ((size_t)b * out_ell + l) * row + n2;
    const u64x2 uu = reinterpret_cast<const u64x2*>(u)[rnd];
    const u64x2 a0 = reinterpret_cast<const u64x2*>(w)[rnd], a1 = reinterpret_cast<const u64x2*>(e1)[rnd];
    const u64x2 kb = reinterpret_cast<const u64x2*>(pk)[(size_t)l * row + n2];
    const u64x2 ka = reinterpret_cast<const u64x2*>(pk)[((size_t)L1 + l) * row + n2];
    const u64x2* I = reinterpret_cast<const u64x2*>(it.in);
    const u64x2 i0 = I[(size_t)l * row + n2], i1 = I[((size_t)it.in_ell + l) * row + n2];
    u64x2 c0, c1;
    c0.x = add_mod(add_mod(mul_mod(kb.x, uu.x, br), a0.x, br.q), i0.x, br.q);
    c0.y = add_mod(add_mod(mul_mod(kb.y, uu.y, br), a0.y, br.q), i0.y, br.q);
    c1.x = add_mod(add_mod(mul_mod(ka.x, uu.x, br), a1.x, br.q), i1.x, br.q);
    c1.y = add_mod(add_mod(mul_mod(ka.y, uu.y, br), a1.y, br.q), i1.y, br.q);
    u64x2* O = reinterpret_cast<u64x2*>(it.out);
    O[(size_t)l * row + n2] = c0;
    O[((size_t)out_ell + l) * row + n2] = c1;
}

// ---- batched decryption (kernels_client.h): everything between the ciphertexts and the slots that were asked for
// grid (N/512, nl_max, n): item b = tab[blockIdx.z], limb l = blockIdx.y.  out [n][nl_max][N] <- c0 + c1 s (+ c2 s^2) on the item's first
// nl limbs (Client::phase for a batch of any limb counts and degrees); the rows an item does not read are zeroed
__global__ __launch_bounds__(256) void phase_batch_kernel(DeviceTables t, u64* __restrict__ out, const DecodeItem* __restrict__ tab,
                                                          const u64* __restrict__ s, int nl_max) {
    const int b = blockIdx.z, l = blockIdx.y;
    const DecodeItem it = tab[b];
    const size_t row = ((size_t)1 << t.log_n) >> 1;
    const size_t n2 = (size_t)blockIdx.x * 256 + threadIdx.x;
    u64x2* O = reinterpret_cast<u64x2*>(out) + ((size_t)b * nl_max + l) * row + n2;
    u64x2 m;
    if (l >= it.nl) {
        m.x = m.y = 0;
        *O = m;
        return;
    }
    const Barrett br = load_barrett(t, l);
    const size_t at = (size_t)l * ((size_t)it.limb_stride >> 1) + n2;
    const u64x2 a0 = reinterpret_cast<const u64x2*>(it.c0)[at], a1 = reinterpret_cast<const u64x2*>(it.c1)[at];
    const u64x2 ss = reinterpret_cast<const u64x2*>(s)[(size_t)l * row + n2];
    m.x = add_mod(a0.x, mul_mod(a1.x, ss.x, br), br.q);
    m.y = add_mod(a0.y, mul_mod(a1.y, ss.y, br), br.q);
    if (it.deg > 1) {
        const u64x2 a2 = reinterpret_cast<const u64x2*>(it.c2)[at];
        m.x = add_mod(m.x, mul_mod(a2.x, mul_mod(ss.x, ss.x, br), br), br.q);
        m.y = add_mod(m.y, mul_mod(a2.y, mul_mod(ss.y, ss.y, br), br), br.q);
    }
    *O = m;
}

// grid (slots/256 rounded up, n): thread i of item b reads coefficients i * gap and i * gap + N/2 of phase [n][nl_max][N] (coefficient
// form), lifts each (decode_lift.h: integer code, the host decoder's double bit for bit) and stores the pair at position bitrev(i) of
// v [n][slots]: the forward FFT begins with a bit reversal, done here so that the stages run in place
__global__ __launch_bounds__(256) void decode_lift_kernel(DeviceTables t, double2* __restrict__ v, const u64* __restrict__ phase,
                                                          const DecodeItem* __restrict__ tab, u64 q0inv, u64 q0inv_shoup, int nl_max, int slots,
                                                          int log_slots) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= slots) return;
    const DecodeItem it = tab[blockIdx.y];
    const size_t N = (size_t)1 << t.log_n;
    const size_t gap = (N / 2) / slots;
    DecodeLift p;
    p.q0 = t.moduli[0];
    p.q1 = it.nl > 1 ? t.moduli[1] : 1;
    p.inv = q0inv;
    p.inv_shoup = q0inv_shoup;
    p.ms = it.ms;
    p.es = it.es;
    p.nl = it.nl;
    const u64* m = phase + (size_t)blockIdx.y * nl_max * N;
    const size_t ca = (size_t)i * gap, cb = ca + N / 2;
    double2 o;
    o.x = decode_lift(m[ca], it.nl > 1 ? m[N + ca] : 0, p);
    o.y = decode_lift(m[cb], it.nl > 1 ? m[N + cb] : 0, p);
    const u32 dst = log_slots ? __brev((u32)i) >> (32 - log_slots) : 0;
    v[(size_t)blockIdx.y * slots + dst] = o;
}

// one butterfly of the forward special FFT exactly as the host loop in client.cpp ckks_fft_special(forward) does it: w = b * ksi with each
// product and each sum rounded on its own, then u + w and u - w
__device__ __forceinline__ void fft_fwd_butterfly(double2& u, double2& b, const double2 k) {
#pragma clang fp contract(off)
    double2 w;
    w.x = b.x * k.x - b.y * k.y;
    w.y = b.x * k.y + b.y * k.x;
    const double2 a = u;
    u.x = a.x + w.x;
    u.y = a.y + w.y;
    b.x = a.x - w.x;
    b.y = a.y - w.y;
}

// ---- forward special FFT, the stages with len <= 512: they touch only aligned blocks of 512 elements, so one workgroup runs them all
// on a tile held in LDS (8 KiB, two elements per thread, a barrier per stage).  data [n_vec][size], bit-reversed input;
// grid (size/512 rounded up, n_vec).  size < 512: one tile of `size` elements and all of the transform
__global__ __launch_bounds__(256) void fft_special_fwd_tile_kernel(double2* data, const u32* __restrict__ rot, const double2* __restrict__ ksi,
                                                                   int size) {
    __shared__ double2 tile[512];
    const int tsz = size < 512 ? size : 512;
    double2* v = data + (size_t)blockIdx.y * size + (size_t)blockIdx.x * 512;
    const int t = threadIdx.x;
    if (t < tsz) tile[t] = v[t];
    if (t + 256 < tsz) tile[t + 256] = v[t + 256];
    for (int len = 2; len <= tsz; len <<= 1) {
        __syncthreads();
        if (t < tsz / 2) {
            const int lenh = len >> 1, lenq = len << 2, gap = (4 * size) / lenq;
            const int j = t % lenh, i = (t / lenh) * len;
            const int idx = (int)(rot[j] % (u32)lenq) * gap;
            double2 u = tile[i + j], b = tile[i + j + lenh];
            fft_fwd_butterfly(u, b, ksi[idx]);
            tile[i + j] = u;
            tile[i + j + lenh] = b;
        }
    }
    __syncthreads();
    if (t < tsz) v[t] = tile[t];
    if (t + 256 < tsz) v[t + 256] = tile[t + 256];
}

// ---- forward special FFT, one later stage (len > 512): the mirror of fft_special_inv_stage_kernel.  grid (size/2 / 256, n_vec)
__global__ __launch_bounds__(256) void fft_special_fwd_stage_kernel(double2* data, const u32* __restrict__ rot, const double2* __restrict__ ksi,
                                                                    int size, int len) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= size / 2) return;
    double2* v = data + (size_t)blockIdx.y * size;
    const int lenh = len >> 1, lenq = len << 2, gap = (4 * size) / lenq;
    const int j = t % lenh, i = (t / lenh) * len;
    const int idx = (int)(rot[j] % (u32)lenq) * gap;
    double2 u = v[i + j], b = v[i + j + lenh];
    fft_fwd_butterfly(u, b, ksi[idx]);
    v[i + j] = u;
    v[i + j + lenh] = b;
}

// grid (lanes * width / 256 rounded up, n): out [n][lanes][width] <- the real parts asked for of v [n][slots * stride]: physical slot
// stride * k + lane holds logical slot k of lane `lane` (interleaved samples); k = idx[e] when a list is given, else e
__global__ __launch_bounds__(256) void decode_gather_kernel(double* __restrict__ out, const double2* __restrict__ v, const int* __restrict__ idx,
                                                            int slots, int stride, int lanes, int width) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= lanes * width) return;
    const int lane = e / width, k = e % width;
    const int src = idx ? idx[k] : k;
    out[(size_t)blockIdx.y * lanes * width + e] = v[(size_t)blockIdx.y * slots * stride + (size_t)src * stride + lane].x;
}

}  // namespace

void launch_phase_batch(const DeviceTables& t, u64* out, const DecodeItem* tab, const u64* s, int nl_max, int n, hipStream_t st) {
    if (n < 1) return;
    hipLaunchKernelGGL(phase_batch_kernel, dim3((1u << t.log_n) / 512, (unsigned)nl_max, (unsigned)n), dim3(256), 0, st, t, out, tab, s, nl_max);
}
void launch_decode_lift(const DeviceTables& t, double* v, const u64* phase, const DecodeItem* tab, u64 q0inv, u64 q0inv_shoup, int nl_max,
                        int slots, int n, hipStream_t st) {
    if (n < 1) return;
    int log_slots = 0;
    while ((1 << log_slots) < slots) ++log_slots;
    hipLaunchKernelGGL(decode_lift_kernel, dim3((unsigned)((slots + 255) / 256), (unsigned)n), dim3(256), 0, st, t, reinterpret_cast<double2*>(v),
                       phase, tab, q0inv, q0inv_shoup, nl_max, slots, log_slots);
}
void launch_fft_special_fwd(double* data, const u32* rot, const double* ksi, int slots, int n_vec, hipStream_t st) {
    if (n_vec < 1 || slots < 2) return;
    hipLaunchKernelGGL(fft_special_fwd_tile_kernel, dim3((unsigned)((slots + 511) / 512), (unsigned)n_vec), dim3(256), 0, st,
                       reinterpret_cast<double2*>(data), rot, reinterpret_cast<const double2*>(ksi), slots);
    const dim3 g((unsigned)((slots / 2 + 255) / 256), (unsigned)n_vec);
    for (int len = 1024; len <= slots; len <<= 1)
        hipLaunchKernelGGL(fft_special_fwd_stage_kernel, g, dim3(256), 0, st, reinterpret_cast<double2*>(data), rot,
                           reinterpret_cast<const double2*>(ksi), slots, len);
}
void launch_decode_gather(double* out, const double* v, const int* idx, int slots, int stride, int lanes, int width, int n, hipStream_t st) {
    if (n < 1) return;
    hipLaunchKernelGGL(decode_gather_kernel, dim3((unsigned)((lanes * width + 255) / 256), (unsigned)n), dim3(256), 0, st, out,
                       reinterpret_cast<const double2*>(v), idx, slots, stride, lanes, width);
}

void launch_interleave_slots(double* out, const double* in, int slots, int stride, int lanes, int n_vec, hipStream_t s) {
    if (n_vec < 1) return;
    int log_stride = 0;
    while ((1 << log_stride) < stride) ++log_stride;
    hipLaunchKernelGGL(interleave_slots_kernel, dim3((unsigned)((((size_t)slots << log_stride) + 255) / 256), (unsigned)n_vec), dim3(256), 0, s,
                       reinterpret_cast<double2*>(out), reinterpret_cast<const double2*>(in), slots, log_stride, lanes);
}
void launch_fft_special_inv(double* data, const u32* rot, const double* ksi, int slots, int n_vec, hipStream_t s) {
    const dim3 g((unsigned)((slots / 2 + 255) / 256), (unsigned)n_vec);
    for (int len = slots; len >= 2; len >>= 1)
        hipLaunchKernelGGL(fft_special_inv_stage_kernel, g, dim3(256), 0, s, reinterpret_cast<double2*>(data), rot,
                           reinterpret_cast<const double2*>(ksi), slots, len);
}
void launch_encode_round_reduce(const DeviceTables& t, u64* out, const double* fftdata, int slots, int ell, u64 scale_mant, int scale_exp,
                                int n_vec, hipStream_t s) {
    int log_slots = 0;
    while ((1 << log_slots) < slots) ++log_slots;
    hipLaunchKernelGGL(encode_round_reduce_kernel, dim3((1u << t.log_n) / 256, (unsigned)n_vec), dim3(256), 0, s, t, out,
                       reinterpret_cast<const double2*>(fftdata), slots, log_slots, ell, ell, 0, scale_mant, scale_exp, 1.0 / slots);
}
void launch_encode_round_reduce_split(const DeviceTables& t, u64* out, const double* fftdata, int slots, int ell_q, int k, int L1, u64 scale_mant,
                                      int scale_exp, int n_vec, hipStream_t s) {
    int log_slots = 0;
    while ((1 << log_slots) < slots) ++log_slots;
    hipLaunchKernelGGL(encode_round_reduce_kernel, dim3((1u << t.log_n) / 256, (unsigned)n_vec), dim3(256), 0, s, t, out,
                       reinterpret_cast<const double2*>(fftdata), slots, log_slots, ell_q + k, ell_q, L1, scale_mant, scale_exp, 1.0 / slots);
}
void launch_sample_small(const DeviceTables& t, u64* out, const SamplerKey& key, u64 stream_base, int kind, int ell, int n_poly, hipStream_t s) {
    const unsigned bx = (unsigned)(((1u << t.log_n) / 8 + 255) / 256);
    hipLaunchKernelGGL(sample_small_kernel, dim3(bx, (unsigned)n_poly), dim3(256), 0, s, t, out, key, stream_base, kind, ell);
}
void launch_encrypt_combine(const DeviceTables& t, u64* ct, const u64* pk, const u64* u, const u64* e0, const u64* e1, const u64* m, int ell,
                            int L1, size_t m_stride, int n_vec, hipStream_t s) {
    hipLaunchKernelGGL(encrypt_combine_kernel, dim3((1u << t.log_n) / 512, (unsigned)(n_vec * ell)), dim3(256), 0, s, t, ct, pk, u, e0, e1, m,
                       ell, L1, m_stride);
}
void launch_sample_flood(const DeviceTables& t, u64* out, const SamplerKey& key, u64 stream_base, u64 gauss_stream_base, int flood_bits,
                         bool gauss, int ell, int n_poly, hipStream_t s) {
    const unsigned bx = (unsigned)(((1u << t.log_n) / 8 + 255) / 256);
    hipLaunchKernelGGL(sample_flood_kernel, dim3(bx, (unsigned)n_poly), dim3(256), 0, s, t, out, key, stream_base, gauss_stream_base, flood_bits,
                       gauss ? 1 : 0, ell);
}
void launch_rerandomize_combine(const DeviceTables& t, const RerandItem* tab, const u64* pk, const u64* u, const u64* w, const u64* e1,
                                int out_ell, int L1, int n_ct, hipStream_t s) {
    hipLaunchKernelGGL(rerandomize_combine_kernel, dim3((1u << t.log_n) / 512, (unsigned)out_ell, (unsigned)n_ct), dim3(256), 0, s, t, tab, pk,
                       u, w, e1, out_ell, L1);
}


// ---- sample ingestion (kernels_client.h) ------------------------------------------------------------------------------
namespace {
__global__ void ingest_xin_kernel(double* __restrict__ x_in, const double* __restrict__ emb, const int* __restrict__ tokens,
                                  const double* __restrict__ table, const double* __restrict__ cls, const double* __restrict__ pos, int S) {
    const int t = blockIdx.x, j = threadIdx.x;           // row t of x_in (0 = CLS), feature j < 128
    if (t == 0) {
        x_in[j] = cls[j];
        return;
    }
    const double e = tokens ? table[(size_t)tokens[t - 1] * 128 + j] : emb[(size_t)(t - 1) * 128 + j];
    {
#pragma clang fp contract(off)
        const double p3 = pos[(size_t)(t - 1) * 128 + j] / 3.0;
        x_in[(size_t)t * 128 + j] = e + p3;
    }
}
__global__ void ingest_project_kernel(double* __restrict__ proj, const double* __restrict__ x_in, const double* __restrict__ E_w,
                                      const double* __restrict__ E_b, const double* __restrict__ F_w, const double* __restrict__ F_b,
                                      int w_cols, int S1) {
    const int r = blockIdx.x, j = threadIdx.x;           // r < 64: rows of E then rows of F
    const double* w = (r < 32 ? E_w : F_w) + (size_t)(r & 31) * w_cols;
    // every product and every sum rounded on its own, in this order (the header's __dmul_rn / __dadd_rn are plain operators that
    // the compiler is free to contract into FMAs; the pragma below is what forbids it)
    {
#pragma clang fp contract(off)
        double acc = w[0] * x_in[j];
        for (int t = 1; t < S1; ++t) {
            const double p = w[t] * x_in[(size_t)t * 128 + j];
            acc = acc + p;
        }
        proj[(size_t)r * 128 + j] = acc + (r < 32 ? E_b : F_b)[r & 31];
    }
}
__global__ void ingest_expand_kernel(double* __restrict__ out, const double* __restrict__ proj, const double* __restrict__ x_in, int S1, int slots) {
    const int v = blockIdx.y;
    const int slot = blockIdx.x * blockDim.x + threadIdx.x;
    if (slot >= slots) return;
    const double* src = v < 64 ? proj + (size_t)v * 128 : x_in + (size_t)(v - 64) * 128;
    const int j = slot >> 7;
    double2 o;
    o.x = j < 128 ? src[j] : 0.0;
    o.y = 0.0;
    reinterpret_cast<double2*>(out)[(size_t)v * slots + slot] = o;
}
// The expanded layout of `stride` samples of one length interleaved: physical slot p of vector v holds slot p >> log_stride of sample
// p & (stride - 1), whose rows are proj + sample * 64 * 128 and x_in + sample * S1 * 128.  Same sources and values as
// ingest_expand_kernel per sample; consecutive threads write consecutive physical slots.
__global__ void ingest_expand_interleaved_kernel(double* __restrict__ out, const double* __restrict__ proj, const double* __restrict__ x_in,
                                                 int S1, int slots, int log_stride) {
    const int v = blockIdx.y;
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    const int phys = slots << log_stride;
    if (p >= phys) return;
    const int sample = p & ((1 << log_stride) - 1), slot = p >> log_stride;
    const double* src = v < 64 ? proj + ((size_t)sample * 64 + v) * 128 : x_in + ((size_t)sample * S1 + (v - 64)) * 128;
    const int j = slot >> 7;
    double2 o;
    o.x = j < 128 ? src[j] : 0.0;
    o.y = 0.0;
    reinterpret_cast<double2*>(out)[(size_t)v * phys + p] = o;
}
// Wrapped layout (include/fhelin.h "Wrapped inputs"): vector w holds up to 128 inputs, slot j*128 + t = row pos[w][t] [j];
// pos [n_w][128] (-1: no input, the slot column stays 0).  Same sources and order as ingest_expand_kernel.
__global__ void ingest_wrap_kernel(double* __restrict__ out, const double* __restrict__ proj, const double* __restrict__ x_in,
                                   const int* __restrict__ pos, int slots) {
    const int w = blockIdx.y;
    const int slot = blockIdx.x * blockDim.x + threadIdx.x;
    if (slot >= slots) return;
    const int j = slot >> 7, t = slot & 127;
    const int v = pos[w * 128 + t];
    double2 o;
    o.x = 0.0;
    o.y = 0.0;
    if (v >= 0 && j < 128) o.x = (v < 64 ? proj + (size_t)v * 128 : x_in + (size_t)(v - 64) * 128)[j];
    reinterpret_cast<double2*>(out)[(size_t)w * slots + slot] = o;
}
// The wrapped layout of `stride` samples of one length interleaved: physical slot p of vector w holds slot p >> log_stride of sample
// p & (stride - 1) in ingest_wrap_kernel's layout; pos is shared by the samples (the same inputs in every lane), the sources are those of
// ingest_expand_interleaved_kernel.  Consecutive threads write consecutive physical slots, one 16-byte store each.
__global__ void ingest_wrap_interleaved_kernel(double* __restrict__ out, const double* __restrict__ proj, const double* __restrict__ x_in,
                                               const int* __restrict__ pos, int S1, int slots, int log_stride) {
    const int w = blockIdx.y;
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    const int phys = slots << log_stride;
    if (p >= phys) return;
    const int sample = p & ((1 << log_stride) - 1), slot = p >> log_stride;
    const int j = slot >> 7, t = slot & 127;
    const int v = pos[w * 128 + t];
    double2 o;
    o.x = 0.0;
    o.y = 0.0;
    if (v >= 0 && j < 128) o.x = (v < 64 ? proj + ((size_t)sample * 64 + v) * 128 : x_in + ((size_t)sample * S1 + (v - 64)) * 128)[j];
    reinterpret_cast<double2*>(out)[(size_t)w * phys + p] = o;
}
}  // namespace
void launch_ingest_expand_interleaved(double* out, const double* proj, const double* x_in, int S1, int slots, int stride, hipStream_t s) {
    int log_stride = 0;
    while ((1 << log_stride) < stride) ++log_stride;
    hipLaunchKernelGGL(ingest_expand_interleaved_kernel, dim3((unsigned)((((size_t)slots << log_stride) + 255) / 256), 64 + S1), dim3(256), 0, s,
                       out, proj, x_in, S1, slots, log_stride);
}
void launch_ingest_wrap(double* out, const double* proj, const double* x_in, const int* pos, int n_w, int slots, hipStream_t s) {
    if (n_w < 1) return;
    hipLaunchKernelGGL(ingest_wrap_kernel, dim3((slots + 255) / 256, n_w), dim3(256), 0, s, out, proj, x_in, pos, slots);
}
void launch_ingest_wrap_interleaved(double* out, const double* proj, const double* x_in, const int* pos, int n_w, int S1, int slots, int stride,
                                    hipStream_t s) {
    if (n_w < 1) return;
    int log_stride = 0;
    while ((1 << log_stride) < stride) ++log_stride;
    hipLaunchKernelGGL(ingest_wrap_interleaved_kernel, dim3((unsigned)((((size_t)slots << log_stride) + 255) / 256), n_w), dim3(256), 0, s, out,
                       proj, x_in, pos, S1, slots, log_stride);
}
void launch_ingest_xin(double* x_in, const double* emb, const int* tokens, const double* table, const double* cls, const double* pos,
                       int S, hipStream_t s) {
    hipLaunchKernelGGL(ingest_xin_kernel, dim3(S + 1), dim3(128), 0, s, x_in, emb, tokens, table, cls, pos, S);
}
void launch_ingest_project(double* proj, const double* x_in, const double* E_w, const double* E_b, const double* F_w, const double* F_b,
                           int w_cols, int S1, hipStream_t s) {
    hipLaunchKernelGGL(ingest_project_kernel, dim3(64), dim3(128), 0, s, proj, x_in, E_w, E_b, F_w, F_b, w_cols, S1);
}
void launch_ingest_expand(double* out, const double* proj, const double* x_in, int S1, int slots, hipStream_t s) {
    hipLaunchKernelGGL(ingest_expand_kernel, dim3((slots + 255) / 256, 64 + S1), dim3(256), 0, s, out, proj, x_in, S1, slots);
}

}  // namespace fhelin
