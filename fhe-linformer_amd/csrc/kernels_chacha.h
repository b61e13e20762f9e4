// Device ChaCha20 (RFC 8439 block function, 20 rounds), shared by the client kernels (kernels_client.hip: the encryption
// randomness) and the seeded-ciphertext kernels (kernels_seeded.hip: the expansion of c1).  State layout as the host generator
// (client.h Prng, fhelin_prng_block): key in words 4-11, 64-bit block counter in words 12-13, 64-bit stream id in words 14-15.
// Device code only: include from .hip files.
#pragma once
#include <hip/hip_runtime.h>
#include "kernels_client.h"

namespace fhelin {

__device__ __forceinline__ u32 rotl32(u32 x, int k) { return (x << k) | (x >> (32 - k)); }
#define FHELIN_QR(a, b, c, d) \
    a += b; d ^= a; d = rotl32(d, 16); c += d; b ^= c; b = rotl32(b, 12); a += b; d ^= a; d = rotl32(d, 8); c += d; b ^= c; b = rotl32(b, 7);
// out: the 64-byte block as 8 little-endian u64 words
__device__ __forceinline__ void chacha20_block(const SamplerKey& k, u64 counter, u64 stream, u64 (&out)[8]) {
    u32 x[16], in[16];
    in[0] = 0x61707865u; in[1] = 0x3320646eu; in[2] = 0x79622d32u; in[3] = 0x6b206574u;
#pragma unroll
    for (int i = 0; i < 8; ++i) in[4 + i] = k.w[i];
    in[12] = (u32)counter; in[13] = (u32)(counter >> 32); in[14] = (u32)stream; in[15] = (u32)(stream >> 32);
#pragma unroll
    for (int i = 0; i < 16; ++i) x[i] = in[i];
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        FHELIN_QR(x[0], x[4], x[8], x[12]) FHELIN_QR(x[1], x[5], x[9], x[13]) FHELIN_QR(x[2], x[6], x[10], x[14]) FHELIN_QR(x[3], x[7], x[11], x[15])
        FHELIN_QR(x[0], x[5], x[10], x[15]) FHELIN_QR(x[1], x[6], x[11], x[12]) FHELIN_QR(x[2], x[7], x[8], x[13]) FHELIN_QR(x[3], x[4], x[9], x[14])
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) out[i] = (u64)(x[2 * i] + in[2 * i]) | ((u64)(x[2 * i + 1] + in[2 * i + 1]) << 32);
}
#undef FHELIN_QR

}  // namespace fhelin
