// Launchers of the seeded-ciphertext kernels (kernels_seeded.hip): secret-key encryption with c1 expanded from a public seed,
// the expansion of c1 on import (include/fhelin.h "Compact ciphertexts" defines the expansion), and seeded key generation
// (include/fhelin.h "Seeded evaluation keys": a key's a half is the expansion of the key-set seed and a per-digit nonce).
#pragma once
#include "kernels.h"
#include "kernels_client.h"

namespace fhelin {

// One ciphertext of a batched expansion: c1 limb l (l < ell) is written to dst + l * N.
// split > 0 (the a half of a level-capped key, include/fhelin.h "Level-capped keys"): ell counts PRESENT rows; row y below split is limb
// y, row y >= split is limb y + skip (the special limbs: skip = n_q - split), expanded and written at its absolute limb.
struct SeededEntry {
    SamplerKey key;   // the 32-byte seed as 8 little-endian u32 words
    u64 nonce;
    u64* dst;
    int32_t ell;
    int32_t split = 0;
    int32_t skip = 0;
    int32_t pad_ = 0;    // 64 bytes
};
static_assert(sizeof(SeededEntry) == 64, "SeededEntry is 64 bytes");

// c1 of n_ct ciphertexts in one launch, grid (N/4/256, max_ell, n_ct); tab [n_ct] is a device table
void launch_seeded_expand(const DeviceTables& t, const SeededEntry* tab, int n_ct, int max_ell, hipStream_t s);

// ct [n_vec][2][ell][N] <- (m - a s + e, a) with a the expansion of (key, nonces[b]) on limbs 0..ell-1; s the secret [>= ell][N],
// e [n_vec][ell][N], m at m + b * m_stride (all NTT form).  nonces: host array of n_vec values (passed as kernel arguments).
void launch_sk_encrypt_combine(const DeviceTables& t, u64* ct, const u64* s, const u64* e, const u64* m, size_t m_stride, int ell,
                               const SamplerKey& key, const u64* nonces, int n_vec, hipStream_t st);

// nonce of digit `digit` of a key (include/fhelin.h "Seeded evaluation keys"): kind 0 public, 1 relinearisation, 2 rotation,
// 3 conjugation key
inline u64 key_nonce(u64 kind, u64 digit, u64 galois) { return (kind << 56) | (digit << 40) | galois; }
constexpr int KEYGEN_MAX_Q = 64;   // Q limbs of the P mod q_l table passed by value

// key [digits][2][ell][N] <- per digit j: b = e_j - a_j s_to (+ (P mod q_l) s_from on the limbs [j alpha, min((j+1) alpha, n_q))),
// a_j = the expansion of (seed, key_nonce(kind, j, galois)) on limbs 0..ell-1.  s_to, s_from [>= ell][N], e [digits][ell][N], all
// NTT form; s_from null: no s_from term (the public key: ell = n_q, digits = 1).  p_mod_q: host array of n_q values.
// grid (N/4/256, ell, digits)
void launch_seeded_keygen_combine(const DeviceTables& t, u64* key, const u64* s_to, const u64* s_from, const u64* e, int ell, int digits,
                                  int alpha, int n_q, const u64* p_mod_q, const SamplerKey& seed, u64 kind, u64 galois, hipStream_t st);
// The same for a switching key capped at max_ell < n_q limbs (include/fhelin.h "Level-capped keys"): only the PRESENT rows - Q limbs
// 0..max_ell-1 and the ell - n_q special limbs - of the `digits` = digits_at(max_ell) digits held are formed, by the same expansion, and
// written where the uncapped launch writes them (limb stride ell; the absent rows are not touched).  e: the noise of the UNCAPPED shape,
// [>= digits][ell][N], of which the present rows are read (the others need not be in NTT form).  ell = the key basis (all n_limbs).
// grid (N/4/256, max_ell + ell - n_q, digits)
void launch_seeded_keygen_combine_capped(const DeviceTables& t, u64* key, const u64* s_to, const u64* s_from, const u64* e, int ell, int digits,
                                         int alpha, int n_q, int max_ell, const u64* p_mod_q, const SamplerKey& seed, u64 kind, u64 galois,
                                         hipStream_t st);

}  // namespace fhelin
