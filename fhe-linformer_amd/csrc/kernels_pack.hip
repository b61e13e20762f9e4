// Bit-packed wire formats (include/fhelin.h "Packed formats"): a residue below a w-bit modulus travels as w bits.
//
// A vector of N residues at width w is the bit stream sum_j v_j 2^(j w), cut into N w / 64 little-endian words.  A tile of 4096
// residues is exactly 64 w words, so every tile starts on a word boundary and blocks are independent: grid = (N / 4096 tiles,
// vectors).  blockIdx.y picks the vector's table entry, so source, destination and width are wave-uniform (scalar loads) and one
// launch serves vectors of different widths.
//
//  * pack_residues_kernel   : a lane forms two adjacent output words (128 stream bits) from the 3..8 residues that touch them and
//    stores them with one 16-byte store (a wave writes 1 KiB contiguous).  The residue loads of neighbouring lanes overlap; the
//    cache serves them and every source byte comes from HBM once.  The loads of a pair are in flight together (5 of them for
//    widths from 32 up, 8 below: the width is uniform, so is the choice).
//  * unpack_residues_kernel : a lane extracts two adjacent residues from the 1..3 words that hold them and stores 16 bytes; its 32
//    word loads carry no branch and are issued before the first is used.
//
// Shifts: a residue at stream offset `bit` relative to the word being formed is shifted left by bit in 0..63 or right by -bit in
// 1..w-1; the spill of a straddling residue into the next word, x >> (64 - bit), is formed as (x >> 1) >> (63 - bit), and unpack
// forms hi << (64 - s) as (hi << 1) << (63 - s).  A count of 64 is never formed.  Reads: the last residue of a tile
// ends exactly at the tile's last bit, so the second word of a straddle is addressed only when the residue really reaches into it and
// nothing is read past a vector's end.
#include <hip/hip_runtime.h>
#include "kernels_pack.h"

namespace fhelin {
namespace {

typedef u64 u64x2 __attribute__((ext_vector_type(2)));
// the table's pointers are global memory: said so, the compiler emits global_ rather than flat_ accesses
typedef __attribute__((address_space(1))) const u64 gu64;
typedef __attribute__((address_space(1))) u64x2 gu64x2;

constexpr int PK_THREADS = 256;
constexpr int PK_TILE = 4096;   // residues per block

// The pair of output words p of a tile: stream bits [128 p, 128 p + 128).  At most R residues touch it (R = 8 covers every width from
// 20 up, R = 5 every width from 32 up: ceil((128 + w - 1) / w)).  All R loads are issued before the first is used: an index past the
// residues that touch the pair is clamped to the tile's last residue (in bounds) and its value dropped.
template <int R>
__device__ __forceinline__ u64x2 pack_pair(const gu64* __restrict__ src, u32 p, u32 w, u64 mask) {
    const u32 first = 128 * p;                    // stream bit (inside the tile) of the pair's bit 0
    const u32 j0 = first / w;                     // the residue that holds it
    const int bit0 = (int)(j0 * w) - (int)first;  // its position relative to the pair: -(w-1)..0
    u64 v[R];
#pragma unroll
    for (int t = 0; t < R; ++t) v[t] = src[min(j0 + t, (u32)PK_TILE - 1)];
    u64 lo = 0, hi = 0;
#pragma unroll
    for (int t = 0; t < R; ++t) {
        const int bit = bit0 + t * (int)w;
        const u64 x = bit < 128 ? v[t] & mask : 0;   // the tile's last residue ends at the last pair's bit 128
        if (bit < 0) {
            lo |= x >> (u32)(-bit);
        } else if (bit < 64) {
            lo |= x << (u32)bit;
            hi |= (x >> 1) >> (u32)(63 - bit);    // x >> (64 - bit) without the count 64 at bit = 0
        } else {
            hi |= x << (u32)(bit & 63);           // bits past 128 fall off: the next pair forms them
        }
    }
    u64x2 o;
    o.x = lo;
    o.y = hi;
    return o;
}

__global__ __launch_bounds__(PK_THREADS) void pack_residues_kernel(const PackEntry* __restrict__ tab) {
    const PackEntry e = tab[blockIdx.y];
    const u32 w = e.width;
    const u64 mask = (1ull << w) - 1;   // w <= 60
    const gu64* __restrict__ src = (const gu64*)(e.src + (size_t)blockIdx.x * PK_TILE);
    gu64x2* __restrict__ dst = (gu64x2*)(e.dst + (size_t)blockIdx.x * 64 * w);
    const u32 pairs = 32 * w;           // 16-byte stores of this tile
    if (w >= 32) {
        for (u32 p = threadIdx.x; p < pairs; p += PK_THREADS) dst[p] = pack_pair<5>(src, p, w, mask);
    } else {
        for (u32 p = threadIdx.x; p < pairs; p += PK_THREADS) dst[p] = pack_pair<8>(src, p, w, mask);
    }
}

// Residue at stream bit `at` of the tile's words.  The second word is the next one only when the residue reaches into it (otherwise the
// same word again: in bounds, and no branch, so a lane's loads are all in flight together); its bits land at 64 - s and above, which
// the mask drops when there is no straddle.  (hi << 1) << (63 - s) is hi << (64 - s) without the count 64 at s = 0.
__device__ __forceinline__ u64 unpack_one(const gu64* __restrict__ src, u32 at, u32 w, u64 mask) {
    const u32 k = at >> 6, s = at & 63;
    const u64 lo = src[k], hi = src[k + (s + w > 64 ? 1u : 0u)];
    return ((lo >> s) | ((hi << 1) << (63 - s))) & mask;
}

__global__ __launch_bounds__(PK_THREADS) void unpack_residues_kernel(const PackEntry* __restrict__ tab) {
    const PackEntry e = tab[blockIdx.y];
    const u32 w = e.width;
    const u64 mask = (1ull << w) - 1;
    const gu64* __restrict__ src = (const gu64*)(e.src + (size_t)blockIdx.x * 64 * w);
    gu64x2* __restrict__ dst = (gu64x2*)(e.dst + (size_t)blockIdx.x * PK_TILE);
#pragma unroll
    for (int it = 0; it < PK_TILE / (2 * PK_THREADS); ++it) {
        const u32 i = it * PK_THREADS + threadIdx.x;   // residues 2 i, 2 i + 1
        u64x2 o;
        o.x = unpack_one(src, 2 * i * w, w, mask);
        o.y = unpack_one(src, (2 * i + 1) * w, w, mask);
        dst[i] = o;
    }
}

}  // namespace

void launch_pack_residues(const PackEntry* d_tab, int n_vec, int N, hipStream_t s) {
    if (N < PK_TILE || N % PK_TILE || n_vec < 1) return;   // callers check: N >= 4096
    for (int v0 = 0; v0 < n_vec; v0 += 65535)
        pack_residues_kernel<<<dim3(N / PK_TILE, std::min(65535, n_vec - v0)), PK_THREADS, 0, s>>>(d_tab + v0);
}

void launch_unpack_residues(const PackEntry* d_tab, int n_vec, int N, hipStream_t s) {
    if (N < PK_TILE || N % PK_TILE || n_vec < 1) return;
    for (int v0 = 0; v0 < n_vec; v0 += 65535)
        unpack_residues_kernel<<<dim3(N / PK_TILE, std::min(65535, n_vec - v0)), PK_THREADS, 0, s>>>(d_tab + v0);
}

}  // namespace fhelin
