// Launch interface of the key-integrity kernel (kernels_keys.hip): the evaluation-key set's range check and digest.
#pragma once
#include "kernels.h"

namespace fhelin {

// Digest of the evaluation-key set (include/fhelin.h, "Evaluation-key sets"): arithmetic modulo the Mersenne prime 2^61 - 1
// on positional weights from a 32-bit counter-based mixer (lowbias32).  Host and device share these definitions.
constexpr u64 KEY_DIGEST_P = (1ull << 61) - 1;
FHE_HD u32 key_mix32(u32 x) {
    x ^= x >> 16;
    x *= 0x7feb352du;
    x ^= x >> 15;
    x *= 0x846ca68bu;
    x ^= x >> 16;
    return x;
}
FHE_HD u64 key_weight_pos(u32 i) { return key_mix32(i ^ 0x9E3779B9u); }      // word i of a limb vector
FHE_HD u64 key_weight_vec(u32 j) { return key_mix32(j | 0x80000000u); }      // limb vector j of a key
// a mod (2^61 - 1), fully reduced, for any 64-bit a
FHE_HD u64 key_red61(u64 a) {
    a = (a & KEY_DIGEST_P) + (a >> 61);
    return a >= KEY_DIGEST_P ? a - KEY_DIGEST_P : a;
}

// Per limb vector v (modulus of limb limb_first + v % limb_count): d_out[2 v] = sum_i (x_i mod P) k_i mod P,
// d_out[2 v + 1] = 1 if every x_i < q, else 0.  d_part: key_digest_scratch_words(N, n_vec) words of device scratch.
size_t key_digest_scratch_words(int N, int n_vec);
// The vectors come in groups of limb_count, group_stride vectors apart: vector v is read from
// data + ((v / limb_count) * group_stride + v % limb_count) * N (the c0 limbs of a batch of ciphertexts [n][2][ell][N]:
// limb_count = ell, group_stride = 2 ell; data[n_vec][N] back to back: group_stride = limb_count)
void launch_key_digest_strided(const DeviceTables& dt, const u64* data, int n_vec, int limb_first, int limb_count, int group_stride,
                               u64* d_part, u64* d_out, hipStream_t s);

}  // namespace fhelin
