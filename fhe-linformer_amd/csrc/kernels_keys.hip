// Integrity of imported / exported key material (include/fhelin.h "Evaluation-key sets").
//
//  * key_digest_partial_kernel : one streaming pass over limb vectors data[v][N].  Every lane reads 16 B per load
//    (coalesced: a wave covers 1 KiB contiguous), checks each residue against its limb's modulus (one scalar per block,
//    read from the context's moduli table) and accumulates sum x_i k_i modulo 2^61 - 1 with k_i = lowbias32(i ^ C): a
//    32x64-bit product and a Mersenne fold per word, small next to the 8 bytes it streams.  Reduction: wave64 butterflies
//    through __shfl_xor, then the block's four waves through LDS; one partial per (block, vector).
//  * key_digest_final_kernel   : one thread per limb vector folds its N / 4096 partials.
// Lazy residues: the running sums stay below 2^61 + 3 (one fold after every addition); only the final value is canonical.
#include <hip/hip_runtime.h>
#include "kernels_keys.h"

namespace fhelin {
namespace {

typedef u64 u64x2 __attribute__((ext_vector_type(2)));

constexpr int DG_THREADS = 256;
constexpr int DG_CHUNK = 4096;                            // words per block
constexpr int DG_ITER = DG_CHUNK / (2 * DG_THREADS);      // 16-byte loads per lane

// a < 2^61 + 3, b < 2^62  ->  a + b folded: < 2^61 + 3
__device__ __forceinline__ u64 dg_add(u64 a, u64 b) {
    const u64 s = a + b;
    return (s & KEY_DIGEST_P) + (s >> 61);
}
// x < 2^61, k < 2^32: x k folded once: < 2^61 + 2^32 < 2^62
__device__ __forceinline__ u64 dg_mul(u64 x, u64 k) {
    const u64 lo = x * k, hi = __umul64hi(x, k);
    return (lo & KEY_DIGEST_P) + ((lo >> 61) | (hi << 3));
}

__global__ __launch_bounds__(DG_THREADS) void key_digest_partial_kernel(const u64* __restrict__ data, int log_n,
                                                                          const u64* __restrict__ moduli, int limb_first,
                                                                          int limb_count, int group_stride, u64* __restrict__ part) {
    const int v = blockIdx.y;
    const size_t N = (size_t)1 << log_n;
    const u64 q = moduli[limb_first + v % limb_count];
    const u32 base = blockIdx.x * DG_CHUNK;
    const size_t row = (size_t)(v / limb_count) * group_stride + v % limb_count;   // = v when the vectors are contiguous
    const u64x2* src = reinterpret_cast<const u64x2*>(data + row * N + base);
    u64x2 w[DG_ITER];
#pragma unroll
    for (int it = 0; it < DG_ITER; ++it) w[it] = __builtin_nontemporal_load(src + it * DG_THREADS + threadIdx.x);
    u64 acc = 0;
    int bad = 0;
#pragma unroll
    for (int it = 0; it < DG_ITER; ++it) {
        const u32 i = base + 2u * (u32)(it * DG_THREADS + threadIdx.x);
        bad |= (w[it].x >= q) | (w[it].y >= q);
        acc = dg_add(acc, dg_mul(key_red61(w[it].x), key_weight_pos(i)));
        acc = dg_add(acc, dg_mul(key_red61(w[it].y), key_weight_pos(i + 1)));
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) acc = dg_add(acc, __shfl_xor(acc, m, 64));
    __shared__ u64 wsum[DG_THREADS / 64];
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) wsum[wave] = acc;
    bad = __syncthreads_or(bad);
    if (threadIdx.x == 0) {
        u64 s = wsum[0];
        for (int k = 1; k < DG_THREADS / 64; ++k) s = dg_add(s, wsum[k]);
        part[(size_t)v * gridDim.x + blockIdx.x] = key_red61(s) | ((u64)(bad != 0) << 63);
    }
}

__global__ void key_digest_final_kernel(const u64* __restrict__ part, int nb, int n_vec, u64* __restrict__ out) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= n_vec) return;
    u64 s = 0, bad = 0;
    for (int b = 0; b < nb; ++b) {
        const u64 p = part[(size_t)v * nb + b];
        bad |= p >> 63;
        s = dg_add(s, p & KEY_DIGEST_P);
    }
    out[2 * v] = key_red61(s);
    out[2 * v + 1] = bad ? 0 : 1;
}

}  // namespace

size_t key_digest_scratch_words(int N, int n_vec) { return (size_t)n_vec * (size_t)(N / DG_CHUNK); }

void launch_key_digest_strided(const DeviceTables& dt, const u64* data, int n_vec, int limb_first, int limb_count, int group_stride,
                               u64* d_part, u64* d_out, hipStream_t s) {
    const int N = 1 << dt.log_n;
    if (N % DG_CHUNK || n_vec < 1 || n_vec > 65535 || limb_count < 1 || limb_first < 0 || limb_first + limb_count > dt.n_limbs ||
        group_stride < limb_count)
        return;   // callers check (capi_keys.cpp, capi_compact.cpp): N >= 4096, limbs inside the context
    const int nb = N / DG_CHUNK;
    key_digest_partial_kernel<<<dim3(nb, n_vec), DG_THREADS, 0, s>>>(data, dt.log_n, dt.moduli, limb_first, limb_count, group_stride,
                                                                     d_part);
    key_digest_final_kernel<<<(n_vec + 63) / 64, 64, 0, s>>>(d_part, nb, n_vec, d_out);
}

}  // namespace fhelin
