// Launch interface of the bit-packing kernels (kernels_pack.hip): residues at their modulus width (include/fhelin.h "Packed formats").
#pragma once
#include "kernels.h"

namespace fhelin {

constexpr int PACK_MIN_WIDTH = 20, PACK_MAX_WIDTH = 60;

// One limb vector of a pack / unpack launch.  pack: src = N residues below 2^width, dst = N width / 64 packed words;
// unpack: src = N width / 64 packed words, dst = N residues.  Both 16-byte aligned (N is a multiple of 4096).
struct PackEntry {
    const u64* src;
    u64* dst;
    u32 width;   // PACK_MIN_WIDTH..PACK_MAX_WIDTH
    u32 pad;
};

// bits of m (the width a residue below m is packed at)
inline int pack_width(u64 m) { return m ? 64 - __builtin_clzll(m) : 0; }
// packed words of one vector of N residues at width w (exact: N is a multiple of 64)
inline size_t pack_words(size_t N, int w) { return N / 64 * (size_t)w; }

// d_tab[n_vec] on the device; N a multiple of 4096.  One launch per 65535 vectors, vectors of any widths side by side.
void launch_pack_residues(const PackEntry* d_tab, int n_vec, int N, hipStream_t s);
void launch_unpack_residues(const PackEntry* d_tab, int n_vec, int N, hipStream_t s);

}  // namespace fhelin
