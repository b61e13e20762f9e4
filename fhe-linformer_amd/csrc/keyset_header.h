// Key-set files, host part: header, moduli and key table of an evaluation-key set - "FHELINEK" and "FHELINEC" in versions 1 and 2,
// "FHELINEP" - read and written by ONE codec that a small format description parameterises (include/fhelin.h "Evaluation-key sets",
// "Seeded evaluation keys", "Level-capped keys" and "Packed formats" describe the layouts).  The sibling of wire_header.h: header-only,
// no I/O and no device call, so that a stand-alone host program can run it under a sanitizer (tools/keyset_header_check.cpp) - the
// reader parses bytes from outside the trust boundary.  The device side - runs, packing, staging, digests - is capi_keys.cpp.
#pragma once
#include <algorithm>
#include <type_traits>
#include "wire_header.h"

namespace fhelin {

// EK_TO_SPARSE / EK_FROM_SPARSE: the two keys of sparse-secret bootstrapping (include/fhelin.h), in formats with 48-byte entries only;
// Galois element 0, and the entry's last word - zero on every other entry - is the Hamming weight of the ephemeral secret
enum : uint32_t { EK_PUBLIC = 0, EK_RELIN = 1, EK_ROTATION = 2, EK_CONJ = 3, EK_TO_SPARSE = 4, EK_FROM_SPARSE = 5 };
constexpr uint32_t EK_KINDS = 6;
constexpr size_t EK_ALIGN = 4096;   // the payloads start at a multiple of it
constexpr uint32_t EK_MAX_KEYS = 1u << 16;

// One (magic, version) of the key-set files: header, moduli [n_q + n_p], key table [n_keys], zeros up to EK_ALIGN, payloads.
struct KeysetFormat {
    char magic[9];
    uint32_t version;
    size_t header;      // bytes before the moduli: 96, 128 or 136
    size_t entry;       // bytes of a table entry: 40, or 48 with u32 max_ell, u32 0
    bool caps;          // entries carry max_ell, and a capped key is stored as its present rows
    size_t seed_at;     // u8[32] key-set seed (0: the format has none)
    size_t halves_at;   // u32 halves, u32 0 (0: not a field, `halves` below)
    uint32_t halves;    // 2: b and a halves of every key; 1: b halves, a is the expansion of the seed
    bool packed;        // payloads at the modulus widths (else 64-bit words)
};
constexpr KeysetFormat KEYSET_FORMATS[5] = {{"FHELINEK", 1, 96, 40, false, 0, 0, 2, false},
                                            {"FHELINEK", 2, 96, 48, true, 0, 0, 2, false},
                                            {"FHELINEC", 1, 128, 40, false, 96, 0, 1, false},
                                            {"FHELINEC", 2, 128, 48, true, 96, 0, 1, false},
                                            {"FHELINEP", 1, 136, 48, true, 96, 128, 0, true}};   // full or compact: halves is a field
constexpr size_t KEYSET_MAX_HEADER = 136;
// what a writer is handed: version 2 only where a key is capped, so that a set without caps is written as it always was
inline const KeysetFormat& keyset_format(bool packed, bool compact, bool any_capped) { return KEYSET_FORMATS[packed ? 4 : 2 * compact + any_capped]; }

struct EkEntry {
    uint32_t kind = 0, digits = 0;
    uint64_t galois = 0, offset = 0, words = 0, digest = 0;
    uint32_t max_ell = 0, reserved = 0;   // max_ell: n_q for the public key, for an uncapped key and for every key of a format without caps
                                          // reserved: 0, or on EK_TO_SPARSE / EK_FROM_SPARSE the Hamming weight of the ephemeral secret
};
struct EkFile {
    const KeysetFormat* fmt = nullptr;
    uint32_t version = 0, n_keys = 0;           // a writer's: seal_keyset
    int32_t prm[9] = {};                        // log_n, n_q, first_bits, scale_bits, n_p, special_bits, dnum, log_slots, hamming
    int32_t boot[7] = {};                       // budget_enc, budget_dec, slots (0: no bootstrapping set up), K, R, cheb_degree, correction
    uint64_t data_offset = 0, stride_word = 0;  // stride_word: 0, or the interleave stride when it is not 1
    uint8_t seed[32] = {};                      // zero unless compact()
    uint32_t halves = 2, reserved = 0;
    int32_t sparse_h = 0;                       // a reader's: the Hamming weight the two sparse-secret entries carry (0: the set has none)
    std::vector<uint64_t> moduli;
    std::vector<EkEntry> keys;
    int32_t stride() const { return stride_word ? (int32_t)stride_word : 1; }
    bool compact() const { return halves == 1; }   // b halves only, a expanded from `seed`
};

// THE field lists.  A field is read into a mutable object and written from a const one, so reader and writer share every offset.
struct KeysetIo {
    const uint8_t* in;
    uint8_t* out;
    template <class T> void operator()(size_t off, T& v) const {
        if constexpr (std::is_const<T>::value) put<typename std::remove_const<T>::type>(out, off, v);
        else v = get<T>(in, off);
    }
};
template <class E> void keyset_header_fields(const KeysetIo& io, const KeysetFormat& f, E& e) {
    io(8, e.version);
    io(12, e.n_keys);
    for (int i = 0; i < 9; ++i) io(16 + 4 * i, e.prm[i]);
    for (int i = 0; i < 7; ++i) io(52 + 4 * i, e.boot[i]);
    io(80, e.data_offset);
    io(88, e.stride_word);
    for (int i = 0; f.seed_at && i < 32; ++i) io(f.seed_at + i, e.seed[i]);
    if (f.halves_at) {
        io(f.halves_at, e.halves);
        io(f.halves_at + 4, e.reserved);
    }
}
template <class X> void keyset_entry_fields(const KeysetIo& io, const KeysetFormat& f, X& x) {
    io(0, x.kind);
    io(4, x.digits);
    io(8, x.galois);
    io(16, x.offset);
    io(24, x.words);
    io(32, x.digest);
    if (f.caps) {
        io(40, x.max_ell);
        io(44, x.reserved);
    }
}

// the format of these first bytes (12 at least), or null; known_magic tells an unknown version from an unknown magic
inline const KeysetFormat* keyset_format_of(const uint8_t* b, bool* known_magic = nullptr) {
    for (const KeysetFormat& f : KEYSET_FORMATS)
        if (std::memcmp(b, f.magic, 8) == 0) {
            if (known_magic) *known_magic = true;
            if (get<uint32_t>(b, 8) == f.version) return &f;
        }
    return nullptr;
}
inline uint64_t keyset_table_end(const KeysetFormat& f, uint64_t n_moduli, uint64_t n_keys) { return f.header + 8 * n_moduli + f.entry * n_keys; }
inline uint64_t keyset_data_offset(uint64_t table_end) { return (table_end + EK_ALIGN - 1) / EK_ALIGN * EK_ALIGN; }

// How many bytes from the file's start read_keyset_header wants (header, moduli, table), told from its first `have` bytes
// (KEYSET_MAX_HEADER are enough).  Where those do not say - too few, an unknown format, counts out of range - the answer is the
// longest header: the reader refuses such a file from that much.  At most 136 + 8 * 128 + 48 * 65536 bytes.
inline size_t keyset_prefix_bytes(const uint8_t* b, size_t have) {
    const KeysetFormat* f = have >= 96 ? keyset_format_of(b) : nullptr;
    if (!f) return KEYSET_MAX_HEADER;
    EkFile e;
    keyset_header_fields(KeysetIo{b, nullptr}, KEYSET_FORMATS[0], e);   // the 96 bytes that every format has
    const bool counts_ok = e.prm[1] >= 1 && e.prm[1] <= 64 && e.prm[4] >= 0 && e.prm[4] <= 64 && e.n_keys <= EK_MAX_KEYS;
    return counts_ok ? (size_t)keyset_table_end(*f, (uint64_t)e.prm[1] + e.prm[4], e.n_keys) : KEYSET_MAX_HEADER;
}

// Payload words of one key in format f: [digits, or 1 for the public key][halves] groups of the Q limb vectors 0 .. max_ell-1 and (a
// switching key) the n_p special ones, a vector being N words - or N width[limb] / 64 in a packed format (width[n_q + n_p])
inline uint64_t keyset_key_words(const KeysetFormat& f, const int32_t* prm, uint32_t kind, uint32_t digits, uint32_t max_ell, uint32_t halves,
                                 const int* width) {
    const uint64_t N = 1ull << prm[0], n_q = (uint64_t)prm[1], n_p = kind == EK_PUBLIC ? 0 : (uint64_t)prm[4];
    uint64_t per_group = 0;
    for (uint64_t l = 0; l < max_ell; ++l) per_group += f.packed ? pack_words(N, width[l]) : N;
    for (uint64_t l = 0; l < n_p; ++l) per_group += f.packed ? pack_words(N, width[n_q + l]) : N;
    return (kind == EK_PUBLIC ? 1 : (uint64_t)digits) * halves * per_group;
}

// Header, moduli and key table in b[have], the first bytes of a file of file_size bytes: every field validated against the others
// and against the file's size, nothing about a context.  A malformed set is FHELIN_ERR_ARG.
inline EkFile read_keyset_header(const uint8_t* b, size_t have, uint64_t file_size) {
    auto refuse = [](const char* what) { return Error(FHELIN_ERR_ARG, std::string("evaluation-key set: ") + what); };
    const uint64_t lim = std::min<uint64_t>(have, file_size);
    if (lim < 96) throw refuse("truncated header");
    bool known_magic = false;
    const KeysetFormat* fp = keyset_format_of(b, &known_magic);
    if (!fp) throw refuse(known_magic ? "unsupported version" : "bad magic");
    const KeysetFormat& f = *fp;
    if (lim < f.header) throw refuse("truncated header");
    EkFile e;
    e.fmt = fp;
    e.halves = f.halves;
    keyset_header_fields(KeysetIo{b, nullptr}, f, e);
    if (f.halves_at) {
        if (e.halves < 1 || e.halves > 2 || e.reserved != 0) throw refuse("packed set: halves must be 1 or 2");
        if (e.halves == 2)
            for (uint8_t s : e.seed)
                if (s) throw refuse("a full packed set carries no key-set seed");
    }
    const int log_n = e.prm[0], n_q = e.prm[1], n_p = e.prm[4], log_slots = e.prm[7];
    if (log_n < 12 || log_n > 17 || n_q < 1 || n_q > 64 || n_p < 0 || n_p > 64 || e.prm[6] < 1) throw refuse("parameters out of range");
    // the interleave stride: 0 (a set written at stride 1), or a power of two >= 2 whose physical packing fits the ring:
    // stride << log_slots <= N / 2, compared on the shifted-down side, where no stride word wraps
    const uint64_t sw = e.stride_word;
    if (sw == 1 || (sw & (sw - 1)) || log_slots < 1 || log_slots > log_n - 1 || sw > ((1ull << (log_n - 1)) >> log_slots))
        throw refuse("bad interleave stride");
    const int32_t* bt = e.boot;
    const bool boot_ok = bt[2] == 0 ? (bt[0] | bt[1] | bt[3] | bt[4] | bt[5] | bt[6]) == 0
                                    : bt[0] >= 1 && bt[1] >= 1 && bt[2] >= 4 && !(bt[2] & (bt[2] - 1)) && bt[3] >= 1 && bt[4] >= 0 && bt[4] <= 8 &&
                                          bt[5] >= 3 && bt[5] <= 255 && bt[6] >= 0 && bt[6] <= 20;
    if (!boot_ok) throw refuse("bad bootstrap configuration");
    if (e.n_keys > EK_MAX_KEYS) throw refuse("too many keys");
    const uint64_t N = 1ull << log_n, nm = (uint64_t)n_q + n_p;
    const uint64_t table = f.header + 8 * nm, table_end = keyset_table_end(f, nm, e.n_keys);
    const uint32_t alpha = ((uint32_t)n_q + (uint32_t)e.prm[6] - 1) / (uint32_t)e.prm[6];   // Context: limbs per digit
    if (file_size < table_end) throw refuse("truncated key table");
    if (have < table) throw refuse("truncated moduli");
    for (uint64_t l = 0; l < nm; ++l) e.moduli.push_back(get<uint64_t>(b, f.header + 8 * l));
    std::vector<int> width;
    if (f.packed) modulus_widths(e.moduli.data(), (int)nm, N, "evaluation-key set: packed set", &width);
    if (have < table_end) throw refuse("truncated key table");
    if (e.data_offset != keyset_data_offset(table_end)) throw refuse("bad payload offset");
    uint64_t at = e.data_offset, last_g = 0;
    int seen[EK_KINDS] = {};
    for (uint32_t k = 0; k < e.n_keys; ++k) {
        EkEntry x;
        x.max_ell = (uint32_t)n_q;
        keyset_entry_fields(KeysetIo{b + table + f.entry * k, nullptr}, f, x);
        if (f.caps) {
            const bool sparse = x.kind == EK_TO_SPARSE || x.kind == EK_FROM_SPARSE;
            if (sparse ? x.reserved < 8 || x.reserved > N || (e.sparse_h && (uint32_t)e.sparse_h != x.reserved) : x.reserved != 0)
                throw refuse(sparse ? "bad Hamming weight on a sparse-secret key" : "non-zero reserved word in the key table");
            if (sparse) e.sparse_h = (int32_t)x.reserved;
            if (x.max_ell < 1 || x.max_ell > (uint32_t)n_q || (x.kind == EK_PUBLIC && x.max_ell != (uint32_t)n_q)) throw refuse("max_ell outside 1 .. n_q");
            if (x.kind == EK_TO_SPARSE && x.max_ell != std::min<uint32_t>(2, (uint32_t)n_q)) throw refuse("the to-sparse key is held at two limbs");
            if (x.kind != EK_PUBLIC && x.kind < EK_KINDS && x.digits != (x.max_ell + alpha - 1) / alpha)
                throw refuse("digit count is not that of a key switch at max_ell limbs");
        }
        if (x.kind >= (f.caps ? EK_KINDS : EK_TO_SPARSE)) throw refuse("unknown key kind");
        if (x.kind != EK_ROTATION && ++seen[x.kind] > 1) throw refuse("duplicate key");
        if ((x.kind == EK_PUBLIC) != (x.digits == 0) || x.digits > (uint32_t)n_q ||
            x.words != keyset_key_words(f, e.prm, x.kind, x.digits, x.max_ell, e.halves, width.data()))
            throw refuse("key size does not match the parameters");
        if (x.kind == EK_ROTATION) {
            if (!(x.galois & 1) || x.galois >= 2 * N - 1 || x.galois <= last_g) throw refuse("bad or unordered Galois element");
            last_g = x.galois;
        } else if (x.galois != (x.kind == EK_CONJ ? 2 * N - 1 : 0)) {
            throw refuse("bad Galois element");
        }
        if (x.offset != at || x.digest >= KEY_DIGEST_P) throw refuse("bad key table entry");
        at += 8 * x.words;
        e.keys.push_back(x);
    }
    if (seen[EK_TO_SPARSE] != seen[EK_FROM_SPARSE]) throw refuse("one sparse-secret key without the other");
    if (file_size != at) throw refuse("file size does not match the key table (truncated?)");
    return e;
}

// A writer's last step before write_keyset_header: version, n_keys, data_offset and every key's offset from fmt, the moduli and the
// words of the keys (the payloads lie back to back).  Returns the file's size.
inline uint64_t seal_keyset(EkFile& e) {
    e.version = e.fmt->version;
    e.n_keys = (uint32_t)e.keys.size();
    uint64_t at = e.data_offset = keyset_data_offset(keyset_table_end(*e.fmt, e.moduli.size(), e.n_keys));
    for (EkEntry& x : e.keys) {
        x.offset = at;
        at += 8 * x.words;
    }
    return at;
}
// the data_offset bytes in front of the payloads, zero fill included; of a sealed set only
inline void write_keyset_header(const EkFile& e, uint8_t* out) {
    const KeysetFormat& f = *e.fmt;
    const size_t table = f.header + 8 * e.moduli.size();
    if (e.version != f.version || e.n_keys != e.keys.size() || e.reserved != 0 || e.data_offset != keyset_data_offset(table + f.entry * e.keys.size()))
        throw Error(FHELIN_ERR_INTERNAL, "evaluation-key set: header written before seal_keyset");
    std::memset(out, 0, e.data_offset);
    std::memcpy(out, f.magic, 8);
    keyset_header_fields(KeysetIo{nullptr, out}, f, e);
    std::memcpy(out + f.header, e.moduli.data(), 8 * e.moduli.size());
    for (size_t k = 0; k < e.keys.size(); ++k) keyset_entry_fields(KeysetIo{nullptr, out + table + f.entry * k}, f, e.keys[k]);
}

}  // namespace fhelin
