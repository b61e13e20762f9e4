// Wire formats, device part: what every way of a ciphertext (or key) into or out of the device shares - limb widths, the table of a
// pack / unpack launch and its upload, the range-check-and-digest run, allocation by shape, and the import of ciphertext blobs.  The
// callers are capi_compact.cpp, capi_packed.cpp, capi_transport.cpp and capi_keys.cpp; the blob header is wire_header.h, the key-set header keyset_header.h.
#pragma once
#include <utility>
#include <vector>
#include "capi_internal.h"
#include "kernels_pack.h"
#include "wire_header.h"

namespace fhelin {

// widths of limbs [limb0, limb0 + limbs) of the context (ids: Q then P) and the packed words of one component made of them
inline size_t limb_widths(const Context& x, int limb0, int limbs, const char* who, std::vector<int>* width = nullptr) {
    return modulus_widths(x.moduli.data() + limb0, limbs, x.N, who, width);
}

// Appends the rows of block[rows][N] to the table of a pack / unpack launch: row r at width[r % limbs], the packed vectors back to back
// from `packed` on.  unpack: packed -> rows, else rows -> packed.  Returns the packed words.
size_t pack_rows(std::vector<PackEntry>& tab, size_t N, u64* block, size_t rows, const int* width, int limbs, u64* packed, bool unpack);
// the table on the device, through the pinned staging ring (no stream drain), in pieces of at most one staging slot
Scratch<PackEntry> upload_pack_table(Context& x, const std::vector<PackEntry>& tab);

// Range check and digest (kernels_keys.h) of several blocks of limb vectors in one go: the constructor sizes the scratch, issues the
// launches (at most 65535 vectors each, split between groups) and the download of the per-vector pairs on the context's stream; once
// the CALLER has synchronised, fold() and pairs() answer per block.
struct DigestItem {
    const u64* d;        // vector v at d + ((v / limb_count) * group_stride + v % limb_count) * N
    size_t n_vec;
    int limb_first, limb_count, group_stride;
};
class DigestRun {
public:
    DigestRun(Context& x, const std::vector<DigestItem>& items);
    const u64* pairs(size_t item) const { return &h_[2 * at_[item]]; }   // [n_vec][2]: digest, in-range flag
    // vectors [first, first + n_vec) of an item folded into one digest; in_range: every residue below its limb's modulus
    u64 fold(size_t item, size_t first, size_t n_vec, bool& in_range) const { return fold_key_digest(pairs(item) + 2 * first, n_vec, in_range); }
private:
    Scratch<u64> part_, dg_;
    std::vector<u64> h_;
    std::vector<size_t> at_;   // first vector of item k
};

// Ciphertexts of several shapes for one call: one batch allocation per (stored components, limbs) - 2 components for a seeded form
// that stores 1 - in key order, addressed in CALLER order afterwards.
struct ShapeBatch {
    std::vector<CtPtr> cts;                        // [n], caller order
    std::vector<DigestItem> items;                 // one per shape: the stored vectors of its ciphertexts
    std::vector<std::pair<size_t, size_t>> at;     // [n]: ciphertext i is vectors [second, second + stored ell) of items[first]
    int max_ell = 0;
    ShapeBatch(fhelin_ctx* c, const std::vector<std::pair<int, int>>& shape);   // shape[i] = (stored, ell)
};

// The header of ct's blob in format f, but for the digest, with `stored` components: 1 is the seeded form (seed, nonce and the
// positions of a wrapped input go along), 2 or 3 a full form, which carries none of them.
BlobHeader blob_header_of(const BlobFormat& f, const Context& x, const Ciphertext& ct, int stored);

// fhelin_ct_import_compact / fhelin_ct_import_packed: every header against the blob and the context, allocation by shape, upload
// (unpacked first where the format packs), range check + digest + expansion of the seeded c1, one synchronisation; all or nothing.
void import_blobs(fhelin_ctx* c, const std::string& who, const BlobFormat* fmts, size_t n_fmts, const uint8_t* const* blobs,
                  const size_t* sizes, int n, fhelin_ct** outs);

}  // namespace fhelin
