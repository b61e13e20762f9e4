// Host-only check of the key-set header codec (fhe-linformer_amd/csrc/keyset_header.h) under AddressSanitizer and
// UndefinedBehaviorSanitizer.  One valid header of each form is built with the writer - "FHELINEK" and "FHELINEC" in versions 1 and 2,
// "FHELINEP" with halves 2 and 1, one set without keys, one at interleave stride 2 - over toy parameters (N = 2^12, 4+2 limbs of
// different widths, dnum 2, 2^10 slots) with a table of five keys: public, relinearisation, conjugation and two rotations, capped at
// 3 and at 1 limb where the form has caps.  No payload exists: the codec is told the file's size as a number.  Each header is read back
// and compared field by field.  Then the reader is fed every truncation of the prefix (header, moduli, table) from 0 bytes to its end,
// and every single-byte change of the prefix at every value, three ways: as it is; with data_offset, the keys' offsets and the file
// size rewritten to what the changed fields imply; and with the prefix cut or grown to the length they imply as well, so that the
// reader's deeper checks meet changed counts.  Every buffer is a heap block of exactly the length handed to the reader, so a read past
// it is a sanitizer report.  Every call must return or throw Error(FHELIN_ERR_ARG), and whatever is accepted must hold together: a
// stride of 1 or a power of two with stride << log_slots <= N / 2, data_offset + 8 sum(words) = file size, every key's words those
// of the size function, public, relinearisation and conjugation key at most once, rotation elements strictly increasing.  A report or
// anything else ends the program with a non-zero status.  No device is touched and nothing of the library is linked.  Build and run,
// from the repository root:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include \
//       tools/keyset_header_check.cpp -o /tmp/keyset_header_check && /tmp/keyset_header_check
#include <cstdio>
#include <cstdlib>
#include <memory>
#include "../fhe-linformer_amd/csrc/keyset_header.h"

using namespace fhelin;

static const uint64_t MODULI[6] = {(1ull << 59) + 21, (1ull << 39) + 5, (1ull << 39) + 9,
                                   (1ull << 50) + 3,  (1ull << 59) + 55, (1ull << 44) + 7};   // widths 60, 40, 40, 51 | 60, 45
static const int32_t PRM[9] = {12, 4, 55, 40, 2, 60, 2, 10, 64};                              // alpha = 2 limbs per digit
static long calls = 0, accepted = 0;

struct Kind {
    const char* name;
    const KeysetFormat* f;
    uint32_t halves;
    int n_keys, stride;
};

static std::vector<int> widths_of(const EkFile& e) {
    std::vector<int> w;
    if (e.fmt->packed) modulus_widths(e.moduli.data(), (int)e.moduli.size(), (size_t)1 << e.prm[0], "check", &w);
    return w;
}

static EkFile make(const Kind& k, uint64_t* file_size) {
    EkFile e;
    e.fmt = k.f;
    e.halves = k.halves;
    e.stride_word = k.stride == 1 ? 0 : (uint64_t)k.stride;
    std::memcpy(e.prm, PRM, sizeof(PRM));
    if (k.stride == 1) {   // a bootstrap configuration in some, none in the other
        const int32_t boot[7] = {3, 3, 1024, 28, 3, 47, 10};
        std::memcpy(e.boot, boot, sizeof(boot));
    }
    for (int i = 0; i < 32 && e.compact(); ++i) e.seed[i] = (uint8_t)(0xA0 + i);
    e.moduli.assign(MODULI, MODULI + 6);
    const std::vector<int> w = widths_of(e);
    const uint64_t N = 1ull << PRM[0];
    const struct { uint32_t kind; uint64_t galois; uint32_t cap; } keys[5] = {{EK_PUBLIC, 0, 4}, {EK_RELIN, 0, 4}, {EK_CONJ, 2 * N - 1, 4},
                                                                             {EK_ROTATION, 5, 3}, {EK_ROTATION, 25, 1}};
    for (int i = 0; i < k.n_keys; ++i) {
        EkEntry x;
        x.kind = keys[i].kind;
        x.galois = keys[i].galois;
        x.max_ell = k.f->caps ? keys[i].cap : 4;
        x.digits = x.kind == EK_PUBLIC ? 0 : (x.max_ell + 1) / 2;
        x.digest = 0x123456789abcdefull + (uint64_t)i;
        x.words = keyset_key_words(*k.f, e.prm, x.kind, x.digits, x.max_ell, e.halves, w.data());
        e.keys.push_back(x);
    }
    *file_size = seal_keyset(e);
    return e;
}

static void fail(const char* name, const char* what) {
    std::printf("FAIL %s: %s\n", name, what);
    std::exit(1);
}

// the reader on a heap block of exactly `have` bytes - the first min(have, src_len) of src, zeros after - of a file said to have
// file_size bytes; what it accepts must hold together
static bool feed(const Kind& k, const uint8_t* src, size_t src_len, size_t have, uint64_t file_size, EkFile* out = nullptr) {
    std::unique_ptr<uint8_t[]> b(new uint8_t[have ? have : 1]);
    const size_t copy = std::min(have, src_len);
    std::memcpy(b.get(), src, copy);
    std::memset(b.get() + copy, 0, have - copy);
    ++calls;
    try {
        const EkFile e = read_keyset_header(b.get(), have, file_size);
        const uint64_t s = (uint64_t)e.stride(), half_ring = 1ull << (e.prm[0] - 1);
        if (!(s == 1 || (s >= 2 && !(s & (s - 1)) && s <= half_ring && (s << e.prm[7]) <= half_ring))) fail(k.name, "accepted a bad stride");
        const std::vector<int> w = widths_of(e);
        uint64_t at = e.data_offset, last_g = 0;
        int seen[4] = {};
        for (const EkEntry& x : e.keys) {
            if (x.words != keyset_key_words(*e.fmt, e.prm, x.kind, x.digits, x.max_ell, e.halves, w.data())) fail(k.name, "accepted a key of another size");
            if (x.kind > EK_CONJ || (x.kind != EK_ROTATION && ++seen[x.kind] > 1)) fail(k.name, "accepted a key twice, or of no kind");
            if (x.kind == EK_ROTATION && x.galois <= last_g) fail(k.name, "accepted unordered rotation keys");
            if (x.kind == EK_ROTATION) last_g = x.galois;
            at += 8 * x.words;
        }
        if (at != file_size || e.n_keys != e.keys.size()) fail(k.name, "accepted a table that does not add up to the file's size");
        ++accepted;
        if (out) *out = e;
        return true;
    } catch (const Error& e) {
        if (e.code != FHELIN_ERR_ARG) fail(k.name, e.what());
        return false;
    }
    // anything else thrown ends the program through std::terminate: a failure
}

// m[len] with data_offset and the keys' offsets rewritten to what its (changed) fields imply; returns the file size they imply and
// the prefix length in *prefix, or 0 where the fields imply none
static uint64_t make_consistent(uint8_t* m, size_t len, size_t* prefix) {
    const KeysetFormat* f = keyset_format_of(m);
    *prefix = keyset_prefix_bytes(m, std::min<size_t>(len, KEYSET_MAX_HEADER));
    EkFile e;
    keyset_header_fields(KeysetIo{m, nullptr}, KEYSET_FORMATS[0], e);
    if (!f || e.prm[1] < 1 || e.prm[1] > 64 || e.prm[4] < 0 || e.prm[4] > 64 || e.n_keys > EK_MAX_KEYS) return 0;   // the counts say no length
    const size_t table = f->header + 8 * ((size_t)e.prm[1] + e.prm[4]);
    uint64_t at = keyset_data_offset(*prefix);
    const uint64_t data_offset = at;
    for (uint32_t k = 0; k < e.n_keys; ++k) {
        const size_t o = table + f->entry * k;
        EkEntry x;   // an entry past the bytes there are is all zero
        if (o + f->entry <= len) {
            keyset_entry_fields(KeysetIo{m + o, nullptr}, *f, x);
            x.offset = at;
            keyset_entry_fields(KeysetIo{nullptr, m + o}, *f, static_cast<const EkEntry&>(x));
        }
        at += 8 * x.words;
    }
    put<uint64_t>(m, 80, data_offset);
    return at;
}

int main() {
    const KeysetFormat* F = KEYSET_FORMATS;
    const Kind kinds[] = {{"full v1", &F[0], 2, 5, 1},       {"full v2", &F[1], 2, 5, 1},         {"compact v1", &F[2], 1, 5, 1},
                          {"compact v2", &F[3], 1, 5, 1},    {"packed full", &F[4], 2, 5, 1},     {"packed compact", &F[4], 1, 5, 1},
                          {"full v1, no keys", &F[0], 2, 0, 1}, {"compact v2, stride 2", &F[3], 1, 5, 2}};
    for (const Kind& k : kinds) {
        uint64_t size = 0;
        const EkFile want = make(k, &size);
        const size_t prefix = (size_t)keyset_table_end(*k.f, 6, (uint64_t)k.n_keys);
        std::vector<uint8_t> head(want.data_offset, 0xEE);
        write_keyset_header(want, head.data());
        for (size_t i = prefix; i < head.size(); ++i)
            if (head[i]) fail(k.name, "the writer leaves the fill up to the payloads non-zero");
        if (keyset_prefix_bytes(head.data(), KEYSET_MAX_HEADER) != prefix) fail(k.name, "the prefix helper disagrees with the writer");
        // 1. the round trip, field by field
        EkFile got;
        if (!feed(k, head.data(), prefix, prefix, size, &got)) fail(k.name, "the writer's header is refused");
        bool same = got.fmt == want.fmt && got.version == k.f->version && got.n_keys == (uint32_t)k.n_keys && got.data_offset == want.data_offset &&
                    std::memcmp(got.prm, want.prm, sizeof(want.prm)) == 0 && std::memcmp(got.boot, want.boot, sizeof(want.boot)) == 0 &&
                    got.stride() == k.stride && got.halves == k.halves && got.compact() == (k.halves == 1) &&
                    std::memcmp(got.seed, want.seed, 32) == 0 && got.moduli == want.moduli && got.keys.size() == want.keys.size();
        for (size_t i = 0; same && i < want.keys.size(); ++i) {
            const EkEntry &a = got.keys[i], &b = want.keys[i];
            same = a.kind == b.kind && a.digits == b.digits && a.galois == b.galois && a.offset == b.offset && a.words == b.words &&
                   a.digest == b.digest && a.max_ell == b.max_ell;
        }
        if (!same) fail(k.name, "a field changed on the way through writer and reader");
        // 2. every truncation of the prefix, of the bytes in hand and of the file itself: none is a set
        for (size_t cut = 0; cut < prefix; ++cut)
            if (feed(k, head.data(), prefix, cut, size) || feed(k, head.data(), prefix, cut, cut)) fail(k.name, "accepted a truncated prefix");
        // 3. every single-byte change of the prefix
        const long before = accepted;
        std::vector<uint8_t> m(head.begin(), head.begin() + prefix);
        for (size_t at = 0; at < prefix; ++at)
            for (int v = 0; v < 256; ++v) {
                if ((uint8_t)v == head[at]) continue;
                std::memcpy(m.data(), head.data(), prefix);
                m[at] = (uint8_t)v;
                feed(k, m.data(), prefix, prefix, size);   // as it is
                size_t p2 = 0;
                const uint64_t size2 = make_consistent(m.data(), prefix, &p2);
                if (!size2) continue;
                feed(k, m.data(), prefix, prefix, size2);                    // offsets and file size consistent with the changed fields
                if (p2 != prefix) feed(k, m.data(), prefix, p2, size2);      // and the prefix as long as they say
            }
        std::printf("%-22s prefix %3zu bytes, file %8llu: round trip ok, %zu truncations refused, %ld of the changed headers still valid\n", k.name,
                    prefix, (unsigned long long)size, 2 * prefix, accepted - before);
    }
    // 4. stride words whose shift by log_slots = 10 leaves the 64 bits
    for (int bit : {53, 54, 63}) {
        uint64_t size = 0;
        const EkFile e = make(kinds[0], &size);
        std::vector<uint8_t> head(e.data_offset);
        write_keyset_header(e, head.data());
        put<uint64_t>(head.data(), 88, 1ull << bit);
        if (feed(kinds[0], head.data(), head.size(), head.size(), size)) fail("stride word", "accepted 1 << 53, 54 or 63");
    }
    std::printf("keyset_header_check: %ld reader calls, every one returned or refused with FHELIN_ERR_ARG; %ld headers accepted\n", calls, accepted);
    return 0;
}
