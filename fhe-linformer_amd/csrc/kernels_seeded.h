// Launchers of the seeded-ciphertext kernels (kernels_seeded.hip): secret-key encryption with c1 expanded from a public seed,
// and the expansion of c1 on import (include/fhelin.h "Compact ciphertexts" defines the expansion).
#pragma once
#include "kernels.h"
#include "kernels_client.h"

namespace fhelin {

// One ciphertext of a batched expansion: c1 limb l (l < ell) is written to dst + l * N
struct SeededEntry {
    SamplerKey key;   // the 32-byte seed as 8 little-endian u32 words
    u64 nonce;
    u64* dst;
    int32_t ell;
    int32_t pad_ = 0;
    u64 pad2_ = 0;    // 64 bytes
};
static_assert(sizeof(SeededEntry) == 64, "SeededEntry is 64 bytes");

// c1 of n_ct ciphertexts in one launch, grid (N/4/256, max_ell, n_ct); tab [n_ct] is a device table
void launch_seeded_expand(const DeviceTables& t, const SeededEntry* tab, int n_ct, int max_ell, hipStream_t s);

// ct [n_vec][2][ell][N] <- (m - a s + e, a) with a the expansion of (key, nonces[b]) on limbs 0..ell-1; s the secret [>= ell][N],
// e [n_vec][ell][N], m at m + b * m_stride (all NTT form).  nonces: host array of n_vec values (passed as kernel arguments).
void launch_sk_encrypt_combine(const DeviceTables& t, u64* ct, const u64* s, const u64* e, const u64* m, size_t m_stride, int ell,
                               const SamplerKey& key, const u64* nonces, int n_vec, hipStream_t st);

}  // namespace fhelin
