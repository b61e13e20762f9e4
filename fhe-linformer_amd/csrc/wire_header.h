// Wire formats, host part: the header of a ciphertext blob - compact ("FHELINCC", versions 1 and 2) and packed ("FHELINCP") - read and
// written by ONE codec that a small format description parameterises (include/fhelin.h "Compact ciphertexts", "Wrapped inputs" and
// "Packed formats" describe the layouts; bytes 0..95 are the same in all of them).  Header-only and free of any device call, so that a
// stand-alone host program can run it under a sanitizer (tools/wire_header_check.cpp): these readers parse bytes from outside the trust
// boundary.  The device side of the formats is wire.h.
#pragma once
#include <cmath>
#include <cstring>
#include <string>
#include <vector>
#include "../../include/fhelin.h"
#include "pool.h"           // Error
#include "kernels_keys.h"   // KEY_DIGEST_P
#include "kernels_pack.h"   // pack_width, pack_words

namespace fhelin {

// fields of the file and blob formats, at any alignment
template <class T> T get(const uint8_t* b, size_t off) {
    T v;
    std::memcpy(&v, b + off, sizeof(T));
    return v;
}
template <class T> void put(uint8_t* b, size_t off, T v) { std::memcpy(b + off, &v, sizeof(T)); }

// THE width check of the packed formats: a residue travels at 20..60 bits
inline int check_pack_width(int w, const char* who) {
    if (w < PACK_MIN_WIDTH || w > PACK_MAX_WIDTH) throw Error(FHELIN_ERR_ARG, std::string(who) + ": a modulus outside 20..60 bits");
    return w;
}
// widths of these moduli (appended to `width`) and the packed words of one component made of their limb vectors
inline size_t modulus_widths(const uint64_t* moduli, int limbs, size_t N, const char* who, std::vector<int>* width = nullptr) {
    size_t words = 0;
    for (int l = 0; l < limbs; ++l) {
        const int w = check_pack_width(pack_width(moduli[l]), who);
        if (width) width->push_back(w);
        words += pack_words(N, w);
    }
    return words;
}

// One (magic, version) of the ciphertext blobs.  After the shared 96 bytes come the optional u32 fields at the offsets given (0: the
// format has none), the moduli [ell] at `fixed`, the positions [count] of a wrapped input padded to 8 bytes, then the payload.
struct BlobFormat {
    const char* who;      // "compact ciphertext", "packed ciphertext": the prefix of every refusal
    char magic[9];
    uint32_t version;
    size_t fixed;         // header bytes before the moduli: 96, 104 or 112
    size_t stored_at;     // u32 stored components (none: 1, the seeded form)
    size_t count_at;      // u32 count, u32 total of a wrapped input (none: 0, 0)
    size_t reserved_at;   // u32 that must be zero
    int count_min;        // a format that exists for wrapped inputs only asks for count >= 1
    bool packed;          // payload at the modulus widths (else 64-bit words)
};
constexpr BlobFormat CC_FORMATS[2] = {{"compact ciphertext", "FHELINCC", 1, 96, 0, 0, 0, 0, false},
                                      {"compact ciphertext", "FHELINCC", 2, 104, 0, 96, 0, 1, false}};   // 2: a wrapped input
constexpr BlobFormat CP_FORMATS[1] = {{"packed ciphertext", "FHELINCP", 1, 112, 96, 100, 108, 0, true}};

struct BlobHeader {
    const BlobFormat* fmt = nullptr;
    int32_t log_n = 0, ell = 0, deg = 0, slots = 0;
    double scale_hi = 0, scale_lo = 0;
    uint64_t nonce = 0, digest = 0;
    uint8_t seed[32] = {};
    int32_t stored = 1, count = 0, total = 0;
    std::vector<uint64_t> moduli;       // [ell]
    std::vector<int> width;             // [ell], packed formats
    std::vector<int> pos;               // [count]
    const uint8_t* payload = nullptr;   // [stored] components of words_per_poly words, inside the blob (any alignment)
    size_t words_per_poly = 0;          // packed: sum_l N w_l / 64; else ell N
    bool wrapped() const { return count > 0; }
    long double scale() const { return (long double)scale_hi + (long double)scale_lo; }
    void set_scale(long double s) {     // as fhelin_ct_scale
        scale_hi = (double)s;
        scale_lo = (double)(s - (long double)scale_hi);
    }
    size_t header_bytes() const { return fmt->fixed + 8 * (size_t)ell + 8 * (((size_t)count + 1) / 2); }
    size_t bytes() const { return header_bytes() + 8 * (size_t)stored * words_per_poly; }
};

// words of one stored component of `ell` limbs with these moduli; a packed format refuses a width outside 20..60
inline size_t blob_words_per_poly(const BlobFormat& f, int log_n, const uint64_t* moduli, int ell, std::vector<int>* width = nullptr) {
    const size_t N = (size_t)1 << log_n;
    return f.packed ? modulus_widths(moduli, ell, N, f.who, width) : (size_t)ell * N;
}

// Every field validated against the others and against the blob's size; nothing about a context (host-only).  fmts[n_fmts]: the
// versions of one magic that the caller accepts.
inline BlobHeader read_blob_header(const BlobFormat* fmts, size_t n_fmts, const uint8_t* b, size_t bytes) {
    const std::string who = std::string(fmts[0].who) + ": ";
    auto refuse = [&](const char* what) { return Error(FHELIN_ERR_ARG, who + what); };
    if (!b) throw refuse("null blob");
    if (bytes < 96) throw refuse("truncated header");
    if (std::memcmp(b, fmts[0].magic, 8) != 0) throw refuse("bad magic");
    const BlobFormat* f = nullptr;
    for (size_t k = 0; k < n_fmts; ++k)
        if (get<uint32_t>(b, 8) == fmts[k].version) f = &fmts[k];
    if (!f) throw refuse("unsupported version");
    if (bytes < f->fixed) throw refuse("truncated header");
    BlobHeader h;
    h.fmt = f;
    h.log_n = get<int32_t>(b, 16);
    h.ell = get<int32_t>(b, 20);
    h.deg = get<int32_t>(b, 24);
    h.slots = get<int32_t>(b, 28);
    h.scale_hi = get<double>(b, 32);
    h.scale_lo = get<double>(b, 40);
    h.nonce = get<uint64_t>(b, 48);
    std::memcpy(h.seed, b + 56, 32);
    h.digest = get<uint64_t>(b, 88);
    const uint32_t stored = f->stored_at ? get<uint32_t>(b, f->stored_at) : 1;
    const uint32_t count = f->count_at ? get<uint32_t>(b, f->count_at) : 0, total = f->count_at ? get<uint32_t>(b, f->count_at + 4) : 0;
    if (h.log_n < 12 || h.log_n > 17 || h.ell < 1 || h.ell > 64) throw refuse("ring dimension or limb count out of range");
    if (stored < 1 || stored > 3) throw refuse("stored components must be 1 (seeded), 2 or 3");
    if (count > 128 || count < (uint32_t)f->count_min || (count > 0 && (stored != 1 || h.ell < 2 || total < count || total > 65535)) ||
        (count == 0 && total != 0))
        throw refuse("bad wrapped limb count, input count or total (a wrapped input is stored seeded)");
    if (f->reserved_at && get<uint32_t>(b, f->reserved_at) != 0) throw refuse("nonzero reserved word");
    h.stored = (int32_t)stored;
    h.count = (int32_t)count;
    h.total = (int32_t)total;
    const size_t head = h.header_bytes();
    if (get<uint32_t>(b, 12) != head) throw refuse("header size does not match the limb and input counts");
    if (bytes < head) throw refuse("truncated header");
    for (int l = 0; l < h.ell; ++l) h.moduli.push_back(get<uint64_t>(b, f->fixed + 8 * (size_t)l));
    h.words_per_poly = blob_words_per_poly(*f, h.log_n, h.moduli.data(), h.ell, &h.width);
    if (bytes != h.bytes()) throw refuse("size does not match the header (truncated?)");
    const size_t at = f->fixed + 8 * (size_t)h.ell;
    for (int t = 0; t < h.count; ++t) {
        const int32_t v = get<int32_t>(b, at + 4 * (size_t)t);
        if (v < 0 || v >= h.total || (t && v <= h.pos.back())) throw refuse("bad input positions");
        h.pos.push_back(v);
    }
    for (size_t k = at + 4 * (size_t)h.count; k < head; ++k)
        if (b[k]) throw refuse("nonzero padding");
    // a seeded form is an unmodified encryption (degree 1 or 2); a full form may be any value of a pass
    if (h.deg < 1 || h.deg > (h.stored == 1 ? 2 : 16) || h.slots < 1 || (h.slots & (h.slots - 1)) || h.slots > (1 << (h.log_n - 1)))
        throw refuse("bad degree or slot count");
    if (!(std::isfinite(h.scale_hi) && h.scale_hi > 0 && std::isfinite(h.scale_lo) && std::fabs(h.scale_lo) <= std::ldexp(h.scale_hi, -52)))
        throw refuse("bad scale");
    if (h.digest >= KEY_DIGEST_P) throw refuse("bad digest field");
    if (h.stored != 1) {
        bool zero = h.nonce == 0;
        for (uint8_t s : h.seed) zero &= s == 0;
        if (!zero) throw refuse("a full blob carries no seed or nonce");
    }
    h.payload = b + head;
    return h;
}

// the header_bytes() bytes in front of the payload; the caller filled every field but payload (fmt, moduli[ell] and pos[count] included)
inline void write_blob_header(const BlobHeader& h, uint8_t* out) {
    const BlobFormat& f = *h.fmt;
    const size_t head = h.header_bytes();
    std::memset(out, 0, head);
    std::memcpy(out, f.magic, 8);
    put<uint32_t>(out, 8, f.version);
    put<uint32_t>(out, 12, (uint32_t)head);
    const int32_t shape[4] = {h.log_n, h.ell, h.deg, h.slots};
    std::memcpy(out + 16, shape, sizeof(shape));
    put<double>(out, 32, h.scale_hi);
    put<double>(out, 40, h.scale_lo);
    put<uint64_t>(out, 48, h.nonce);
    std::memcpy(out + 56, h.seed, 32);
    put<uint64_t>(out, 88, h.digest);
    if (f.stored_at) put<uint32_t>(out, f.stored_at, (uint32_t)h.stored);
    if (f.count_at) {
        put<uint32_t>(out, f.count_at, (uint32_t)h.count);
        put<uint32_t>(out, f.count_at + 4, (uint32_t)h.total);
    }
    std::memcpy(out + f.fixed, h.moduli.data(), 8 * (size_t)h.ell);
    for (int t = 0; t < h.count; ++t) put<int32_t>(out, f.fixed + 8 * (size_t)h.ell + 4 * (size_t)t, h.pos[t]);
}

}  // namespace fhelin
