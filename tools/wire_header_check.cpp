// Host-only check of the ciphertext blob header codec (fhe-linformer_amd/csrc/wire_header.h) under AddressSanitizer and
// UndefinedBehaviorSanitizer.  One valid header of each kind is built with the writer - compact version 1, compact version 2 with an
// odd and an even input count, packed full with 2 and 3 components, packed seeded, packed wrapped - read back and compared field by
// field.  Then the reader is fed every truncation of each blob from 0 bytes to header + 8, and every single-byte change of the header
// at every value, three ways: as it is; with the header-size field rewritten to what the changed fields imply; and with the blob cut
// or grown to the length they imply as well, so that the reader's deeper checks (moduli, positions, padding) meet changed counts.
// Every buffer is a heap block of exactly the length handed to the reader, so a read past it is a sanitizer report.  Every call must
// return or throw Error(FHELIN_ERR_ARG); a report or anything else ends the program with a non-zero status.  No device is touched and
// nothing of the library is linked.  Build and run, from the repository root:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include \
//       tools/wire_header_check.cpp -o /tmp/wire_header_check && /tmp/wire_header_check
#include <cstdio>
#include <cstdlib>
#include <memory>
#include "../fhe-linformer_amd/csrc/wire_header.h"

using namespace fhelin;

static const uint64_t MODULI[4] = {(1ull << 59) + 21, (1ull << 39) + 5, (1ull << 39) + 9, (1ull << 50) + 3};   // widths 60, 40, 40, 51
static long calls = 0, accepted = 0;

struct Kind {
    const char* name;
    const BlobFormat* fmts;
    size_t n_fmts;
    const BlobFormat* f;
    int ell, stored, count;
};

static BlobHeader make(const Kind& k) {
    BlobHeader h;
    h.fmt = k.f;
    h.log_n = 12;
    h.ell = k.ell;
    h.deg = k.stored == 1 ? 1 : 2;
    h.slots = 1 << 10;
    h.set_scale(1.25L * (1ull << 40) + 0.0000003L);
    h.digest = 0x123456789abcdefull;
    h.stored = k.stored;
    if (k.stored == 1) {
        h.nonce = 0x0102030405060708ull;
        for (int i = 0; i < 32; ++i) h.seed[i] = (uint8_t)(0xA0 + i);
    }
    h.count = k.count;
    h.total = k.count ? 3 * k.count : 0;
    for (int t = 0; t < k.count; ++t) h.pos.push_back(3 * t + 1);
    h.moduli.assign(MODULI, MODULI + k.ell);
    h.words_per_poly = blob_words_per_poly(*k.f, h.log_n, h.moduli.data(), h.ell, &h.width);
    return h;
}

// the reader on a heap block of exactly `len` bytes: the first min(len, src_len) of src, zeros after - as far as any header can reach
// (112 + 8 * 64 + 8 * 64 bytes); the reader never looks at a payload, which stays as the allocator left it
static bool feed(const Kind& k, const uint8_t* src, size_t src_len, size_t len, BlobHeader* out = nullptr) {
    std::unique_ptr<uint8_t[]> b(new uint8_t[len ? len : 1]);
    const size_t reach = std::min<size_t>(len, 2048), have = std::min(reach, src_len);
    std::memcpy(b.get(), src, have);
    std::memset(b.get() + have, 0, reach - have);
    ++calls;
    try {
        const BlobHeader h = read_blob_header(k.fmts, k.n_fmts, b.get(), len);
        // what it accepted lies inside the block
        if (h.payload != b.get() + h.header_bytes() || h.bytes() != len) {
            std::printf("FAIL %s: accepted a blob whose payload is not the rest of it\n", k.name);
            std::exit(1);
        }
        ++accepted;
        if (out) {
            *out = h;
            out->payload = nullptr;
        }
        return true;
    } catch (const Error& e) {
        if (e.code != FHELIN_ERR_ARG) {
            std::printf("FAIL %s: refusal with code %d: %s\n", k.name, e.code, e.what());
            std::exit(1);
        }
        return false;
    }
    // anything else thrown ends the program through std::terminate: a failure
}

// the length the (possibly changed) header fields imply, 0 when they imply none below 1 MiB
static size_t implied_bytes(const Kind& k, const uint8_t* b, size_t len, size_t* head) {
    const BlobFormat* f = nullptr;
    for (size_t i = 0; i < k.n_fmts; ++i)
        if (get<uint32_t>(b, 8) == k.fmts[i].version) f = &k.fmts[i];
    if (!f) return 0;
    const int32_t log_n = get<int32_t>(b, 16), ell = get<int32_t>(b, 20);
    const uint32_t stored = f->stored_at ? get<uint32_t>(b, f->stored_at) : 1, count = f->count_at ? get<uint32_t>(b, f->count_at) : 0;
    if (log_n < 12 || log_n > 13 || ell < 1 || ell > 64 || stored < 1 || stored > 3 || count > 128) return 0;
    *head = f->fixed + 8 * (size_t)ell + 8 * (((size_t)count + 1) / 2);
    if (*head > len) return *head;
    std::vector<uint64_t> m;
    for (int l = 0; l < ell; ++l) m.push_back(f->fixed + 8 * (size_t)l + 8 <= len ? get<uint64_t>(b, f->fixed + 8 * (size_t)l) : 0);
    try {
        const size_t total = *head + 8 * stored * blob_words_per_poly(*f, log_n, m.data(), ell);
        return total <= ((size_t)1 << 20) ? total : 0;
    } catch (const Error&) {
        return *head;
    }
}

int main() {
    const Kind kinds[] = {{"compact v1", CC_FORMATS, 2, &CC_FORMATS[0], 3, 1, 0},  {"compact v2, 3 inputs", CC_FORMATS, 2, &CC_FORMATS[1], 3, 1, 3},
                          {"compact v2, 4 inputs", CC_FORMATS, 2, &CC_FORMATS[1], 2, 1, 4}, {"packed full 2", CP_FORMATS, 1, &CP_FORMATS[0], 3, 2, 0},
                          {"packed full 3", CP_FORMATS, 1, &CP_FORMATS[0], 4, 3, 0}, {"packed seeded", CP_FORMATS, 1, &CP_FORMATS[0], 2, 1, 0},
                          {"packed wrapped", CP_FORMATS, 1, &CP_FORMATS[0], 3, 1, 5}};
    for (const Kind& k : kinds) {
        const BlobHeader want = make(k);
        const size_t head = want.header_bytes(), len = want.bytes();
        std::vector<uint8_t> blob(len, 0);
        write_blob_header(want, blob.data());
        // 1. the round trip, field by field
        BlobHeader got;
        if (!feed(k, blob.data(), len, len, &got)) {
            std::printf("FAIL %s: the writer's header is refused\n", k.name);
            return 1;
        }
        const bool same = got.fmt == want.fmt && got.log_n == want.log_n && got.ell == want.ell && got.deg == want.deg && got.slots == want.slots &&
                          got.scale_hi == want.scale_hi && got.scale_lo == want.scale_lo && got.scale() == want.scale() && got.nonce == want.nonce &&
                          got.digest == want.digest && std::memcmp(got.seed, want.seed, 32) == 0 && got.stored == want.stored &&
                          got.count == want.count && got.total == want.total && got.moduli == want.moduli && got.pos == want.pos &&
                          got.words_per_poly == want.words_per_poly && (!k.f->packed || got.width == want.width) &&
                          get<uint32_t>(blob.data(), 12) == head;
        if (!same) {
            std::printf("FAIL %s: a field changed on the way through writer and reader\n", k.name);
            return 1;
        }
        // 2. every truncation from nothing to header + 8: none is a blob
        for (size_t cut = 0; cut <= head + 8; ++cut)
            if (cut != len && feed(k, blob.data(), len, cut)) {
                std::printf("FAIL %s: accepted when cut to %zu bytes\n", k.name, cut);
                return 1;
            }
        // 3. every single-byte change of the header
        const long before = accepted;
        std::vector<uint8_t> m = blob;
        for (size_t at = 0; at < head; ++at) {
            for (int v = 0; v < 256; ++v) {
                if ((uint8_t)v == blob[at]) continue;
                m[at] = (uint8_t)v;
                feed(k, m.data(), len, len);                                   // the size field as written
                size_t h2 = 0;
                const size_t l2 = implied_bytes(k, m.data(), len, &h2);
                if (l2 && at != 12 && at != 13 && at != 14 && at != 15) {
                    const uint32_t keep = get<uint32_t>(m.data(), 12);
                    put<uint32_t>(m.data(), 12, (uint32_t)h2);
                    feed(k, m.data(), len, len);                               // the size field consistent with the changed counts
                    if (l2 != len) feed(k, m.data(), len, l2);                 // and the blob as long as they say
                    put<uint32_t>(m.data(), 12, keep);
                }
            }
            m[at] = blob[at];
        }
        std::printf("%-22s header %3zu bytes, blob %6zu: round trip ok, %zu truncations refused, %ld of the changed headers still valid\n", k.name,
                    head, len, head + 9 - (len <= head + 8 ? 1 : 0), accepted - before);
    }
    std::printf("wire_header_check: %ld reader calls, every one returned or refused with FHELIN_ERR_ARG\n", calls);
    return 0;
}
