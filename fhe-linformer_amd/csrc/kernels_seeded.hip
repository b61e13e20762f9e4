// Seeded ciphertexts (include/fhelin.h "Compact ciphertexts"): c1 = a is not random data but the expansion of a public 32-byte seed
// and a nonce, so a compact ciphertext carries c0 alone.  Residue j of limb l (storage order, NTT form) is
//     (W[2k+1] * 2^64 + W[2k]) mod q_l,   b = j / 4, k = j % 4,   W = ChaCha20(seed, counter (l << 32) | b, stream nonce)
// One thread produces one ChaCha20 block, i.e. the four residues 4b .. 4b+3 of one limb, and writes them as two 16-byte stores
// (consecutive threads: consecutive 32-byte chunks).  Both kernels below call the same __device__ expansion (seeded_residues4),
// which is what makes the client's resident c1 equal a server's expansion bit for bit.
//
//  * seeded_expand_kernel      : c1 of a batch of ciphertexts of mixed levels, one launch; per-ciphertext seed, nonce, ell and
//                                destination from a device table.  grid (N/4/256, max ell, n_ct)
//  * sk_encrypt_combine_kernel : secret-key encryption, c0 = m - a s + e and c1 = a, with a produced in registers.
//                                grid (N/4/256, ell, n_vec)
//  * seeded_keygen_combine_kernel : one key of seeded key generation (include/fhelin.h "Seeded evaluation keys"), every digit in
//                                one launch: b = e - a s_to (+ (P mod q_l) s_from on the digit's limbs), a in registers.
//                                grid (N/4/256, ell, digits); the capped form: grid (N/4/256, max_ell + n_p, digits')
// Cost: the 20 ChaCha rounds are ~1,000 32-bit VALU operations per 64-byte block against 32 bytes of c1 written per block (plus
// the 128-bit Barrett reductions): both kernels are bound by the VALU, not by HBM.  No LDS, no MFMA.
#include <hip/hip_runtime.h>
#include "kernels.h"
#include "kernels_chacha.h"
#include "kernels_seeded.h"

namespace fhelin {
namespace {

typedef u64 u64x2 __attribute__((ext_vector_type(2)));
constexpr int SE_THREADS = 256;
constexpr int SK_BATCH = 32;   // nonces passed by value per sk_encrypt_combine launch

struct NonceSet {
    u64 v[SK_BATCH];
};
struct PModSet {   // P mod q_l for the Q limbs
    u64 v[KEYGEN_MAX_Q];
};

__device__ __forceinline__ Barrett seeded_barrett(const DeviceTables& t, int limb) {
    Barrett b;
    b.q = t.moduli[limb];
    b.r0 = t.barrett[2 * limb];
    b.r1 = t.barrett[2 * limb + 1];
    return b;
}

// residues 4b .. 4b+3 of limb l.  The 128-bit value W[2k+1]:W[2k] is reduced in one Barrett step: with r = floor(2^128 / q) the
// quotient estimate is at most 2 short for ANY 128-bit input, and 3q < 2^64 for every modulus of the library (q < 2^62).
__device__ __forceinline__ void seeded_residues4(const SamplerKey& key, u64 nonce, int l, u32 b, const Barrett& br, u64 (&r)[4]) {
    u64 w[8];
    chacha20_block(key, ((u64)(u32)l << 32) | (u64)b, nonce, w);
#pragma unroll
    for (int k = 0; k < 4; ++k) r[k] = barrett_reduce128(w[2 * k], w[2 * k + 1], br);
}

__global__ __launch_bounds__(SE_THREADS) void seeded_expand_kernel(DeviceTables t, const SeededEntry* __restrict__ tab) {
    const SeededEntry& e = tab[blockIdx.z];
    if ((int)blockIdx.y >= e.ell) return;
    const int l = e.split > 0 && (int)blockIdx.y >= e.split ? (int)blockIdx.y + e.skip : (int)blockIdx.y;   // block-uniform
    const size_t N = (size_t)1 << t.log_n;
    const u32 b = blockIdx.x * SE_THREADS + threadIdx.x;
    if (b >= N / 4) return;
    u64 r[4];
    seeded_residues4(e.key, e.nonce, l, b, seeded_barrett(t, l), r);
    u64x2* o = reinterpret_cast<u64x2*>(e.dst + (size_t)l * N + 4 * (size_t)b);
    o[0] = u64x2{r[0], r[1]};
    o[1] = u64x2{r[2], r[3]};
}

__global__ __launch_bounds__(SE_THREADS) void sk_encrypt_combine_kernel(DeviceTables t, u64* __restrict__ ct, const u64* __restrict__ s,
                                                                         const u64* __restrict__ e, const u64* __restrict__ m, size_t m_stride,
                                                                         int ell, SamplerKey key, NonceSet nonces) {
    const size_t N = (size_t)1 << t.log_n;
    const u32 b = blockIdx.x * SE_THREADS + threadIdx.x;
    if (b >= N / 4) return;
    const int v = blockIdx.z, l = blockIdx.y;
    const Barrett br = seeded_barrett(t, l);
    u64 a[4];
    seeded_residues4(key, nonces.v[v], l, b, br, a);
    const size_t at = (size_t)l * N + 4 * (size_t)b;
    const u64x2* sp = reinterpret_cast<const u64x2*>(s + at);
    const u64x2* ep = reinterpret_cast<const u64x2*>(e + (size_t)v * ell * N + at);
    const u64x2* mp = reinterpret_cast<const u64x2*>(m + (size_t)v * m_stride + at);
    const u64x2 s0 = sp[0], s1 = sp[1], e0 = ep[0], e1 = ep[1], m0 = mp[0], m1 = mp[1];
    const u64 sv[4] = {s0.x, s0.y, s1.x, s1.y}, ev[4] = {e0.x, e0.y, e1.x, e1.y}, mv[4] = {m0.x, m0.y, m1.x, m1.y};
    u64 c[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) c[k] = add_mod(sub_mod(mv[k], mul_mod(a[k], sv[k], br), br.q), ev[k], br.q);
    u64x2* c0 = reinterpret_cast<u64x2*>(ct + ((size_t)(2 * v) * ell) * N + at);
    u64x2* c1 = reinterpret_cast<u64x2*>(ct + ((size_t)(2 * v + 1) * ell) * N + at);
    c0[0] = u64x2{c[0], c[1]};
    c0[1] = u64x2{c[2], c[3]};
    c1[0] = u64x2{a[0], a[1]};
    c1[1] = u64x2{a[2], a[3]};
}

// The limb index l = blockIdx.y is over Q then P (the key basis); digit j = blockIdx.z.  The s_from term, on limbs
// [lo, hi) of digit j only, is a wave-uniform branch.
// CAPPED (include/fhelin.h "Level-capped keys"): blockIdx.y runs over the present_q + n_p PRESENT rows of a key capped at present_q limbs
// and is mapped to the absolute limb l - Q limb y, or special limb n_q + (y - present_q), a block-uniform select - which the ChaCha counter,
// the modulus and every address below take: the rows written are, residue for residue, the uncapped key's, at the same full-stride places.
template <bool CAPPED>
__global__ __launch_bounds__(SE_THREADS) void seeded_keygen_combine_kernel(DeviceTables t, u64* __restrict__ key, const u64* __restrict__ s_to,
                                                                            const u64* __restrict__ s_from, const u64* __restrict__ e, int ell,
                                                                            int alpha, int n_q, int present_q, SamplerKey seed, u64 nonce0, PModSet pm) {
    const size_t N = (size_t)1 << t.log_n;
    const u32 b = blockIdx.x * SE_THREADS + threadIdx.x;
    if (b >= N / 4) return;
    const int j = blockIdx.z;
    const int l = CAPPED && (int)blockIdx.y >= present_q ? n_q + ((int)blockIdx.y - present_q) : (int)blockIdx.y;
    const Barrett br = seeded_barrett(t, l);
    u64 a[4];
    seeded_residues4(seed, nonce0 | ((u64)j << 40), l, b, br, a);
    const size_t at = (size_t)l * N + 4 * (size_t)b;
    const u64x2* sp = reinterpret_cast<const u64x2*>(s_to + at);
    const u64x2* ep = reinterpret_cast<const u64x2*>(e + (size_t)j * ell * N + at);
    const u64x2 s0 = sp[0], s1 = sp[1], e0 = ep[0], e1 = ep[1];
    const u64 sv[4] = {s0.x, s0.y, s1.x, s1.y}, ev[4] = {e0.x, e0.y, e1.x, e1.y};
    u64 r[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) r[k] = sub_mod(ev[k], mul_mod(a[k], sv[k], br), br.q);
    const int lo = j * alpha, hi = min((j + 1) * alpha, n_q);
    if (s_from && l >= lo && l < hi) {
        const u64x2* fp = reinterpret_cast<const u64x2*>(s_from + at);
        const u64x2 f0 = fp[0], f1 = fp[1];
        const u64 fv[4] = {f0.x, f0.y, f1.x, f1.y};
        const u64 pml = pm.v[l];
#pragma unroll
        for (int k = 0; k < 4; ++k) r[k] = add_mod(r[k], mul_mod(pml, fv[k], br), br.q);
    }
    u64x2* kb = reinterpret_cast<u64x2*>(key + ((size_t)(2 * j) * ell) * N + at);
    u64x2* ka = reinterpret_cast<u64x2*>(key + ((size_t)(2 * j + 1) * ell) * N + at);
    kb[0] = u64x2{r[0], r[1]};
    kb[1] = u64x2{r[2], r[3]};
    ka[0] = u64x2{a[0], a[1]};
    ka[1] = u64x2{a[2], a[3]};
}

}  // namespace

void launch_seeded_expand(const DeviceTables& t, const SeededEntry* tab, int n_ct, int max_ell, hipStream_t s) {
    if (n_ct < 1 || max_ell < 1 || n_ct > 65535 || max_ell > t.n_limbs) return;   // callers check (capi_compact.cpp)
    const unsigned bx = (unsigned)(((1u << t.log_n) / 4 + SE_THREADS - 1) / SE_THREADS);
    hipLaunchKernelGGL(seeded_expand_kernel, dim3(bx, (unsigned)max_ell, (unsigned)n_ct), dim3(SE_THREADS), 0, s, t, tab);
}

void launch_sk_encrypt_combine(const DeviceTables& t, u64* ct, const u64* s, const u64* e, const u64* m, size_t m_stride, int ell,
                               const SamplerKey& key, const u64* nonces, int n_vec, hipStream_t st) {
    const size_t N = (size_t)1 << t.log_n;
    const unsigned bx = (unsigned)((N / 4 + SE_THREADS - 1) / SE_THREADS);
    for (int lo = 0; lo < n_vec; lo += SK_BATCH) {
        const int n = n_vec - lo < SK_BATCH ? n_vec - lo : SK_BATCH;
        NonceSet ns{};
        for (int i = 0; i < n; ++i) ns.v[i] = nonces[lo + i];
        hipLaunchKernelGGL(sk_encrypt_combine_kernel, dim3(bx, (unsigned)ell, (unsigned)n), dim3(SE_THREADS), 0, st, t,
                           ct + (size_t)lo * 2 * ell * N, s, e + (size_t)lo * ell * N, m + (size_t)lo * m_stride, m_stride, ell, key, ns);
    }
}

void launch_seeded_keygen_combine(const DeviceTables& t, u64* key, const u64* s_to, const u64* s_from, const u64* e, int ell, int digits,
                                  int alpha, int n_q, const u64* p_mod_q, const SamplerKey& seed, u64 kind, u64 galois, hipStream_t st) {
    if (ell < 1 || ell > t.n_limbs || digits < 1 || digits > 65535 || n_q < 1 || n_q > KEYGEN_MAX_Q || alpha < 1) return;   // callers check (client.cpp)
    PModSet pm{};
    if (s_from)
        for (int l = 0; l < n_q; ++l) pm.v[l] = p_mod_q[l];
    const unsigned bx = (unsigned)((((size_t)1 << t.log_n) / 4 + SE_THREADS - 1) / SE_THREADS);
    hipLaunchKernelGGL(seeded_keygen_combine_kernel<false>, dim3(bx, (unsigned)ell, (unsigned)digits), dim3(SE_THREADS), 0, st, t, key, s_to,
                       s_from, e, ell, alpha, n_q, n_q, seed, key_nonce(kind, 0, galois), pm);
}

void launch_seeded_keygen_combine_capped(const DeviceTables& t, u64* key, const u64* s_to, const u64* s_from, const u64* e, int ell, int digits,
                                         int alpha, int n_q, int max_ell, const u64* p_mod_q, const SamplerKey& seed, u64 kind, u64 galois,
                                         hipStream_t st) {
    if (ell != t.n_limbs || ell <= n_q || digits < 1 || digits > 65535 || n_q < 1 || n_q > KEYGEN_MAX_Q || alpha < 1 || max_ell < 1 ||
        max_ell > n_q || !s_from || (size_t)(digits - 1) * alpha >= (size_t)max_ell)
        return;   // callers check (client.cpp): a switching key over Q and P, its digits those of a switch at max_ell limbs
    PModSet pm{};
    for (int l = 0; l < n_q; ++l) pm.v[l] = p_mod_q[l];
    const unsigned bx = (unsigned)((((size_t)1 << t.log_n) / 4 + SE_THREADS - 1) / SE_THREADS);
    const unsigned rows = (unsigned)(max_ell + (ell - n_q));
    hipLaunchKernelGGL(seeded_keygen_combine_kernel<true>, dim3(bx, rows, (unsigned)digits), dim3(SE_THREADS), 0, st, t, key, s_to, s_from, e,
                       ell, alpha, n_q, max_ell, seed, key_nonce(kind, 0, galois), pm);
}

}  // namespace fhelin
