// extern "C" boundary, part 4: evaluation-key sets (include/fhelin.h "Evaluation-key sets" and "Seeded evaluation keys": both file
// formats are documented there).  A client context writes its public key and every switching key it holds; a context that never
// held a secret loads them and evaluates with them alone.  Every key is range-checked and digested on the device (kernels_keys.hip)
// on the way out and on the way in; the file is streamed through two pinned staging buffers, so host memory stays bounded by them.
// A compact set ("FHELINEC") stores the b halves and the key-set seed; the loader expands every a half in one launch
// (kernels_seeded.hip) before it digests.
// Version 2 of both formats (include/fhelin.h "Level-capped keys") stores the present rows of capped keys only.  Payloads are dense in
// the file and full-stride on the device: the staging pipeline copies run by run (one run of Q rows and one of special rows per digit
// and half - plain 1D copies, a few MB each at driver scale), and the digest reads the rows where they lie through the strided digest
// launch (kernels_keys.h), one launch for the Q rows and one for the special rows of a key.  No scatter kernel: a scatter would need
// the dense payload in device memory first, which is exactly the copy the cap saves.
// A packed set ("FHELINEP", include/fhelin.h "Packed formats") holds the same present rows, every limb vector at its modulus width: one
// key at a time is packed into (or unpacked out of) a scratch block of one key's packed payload, which is what the staging pipeline then
// streams; digests are those of the unpacked residues, computed by the same launches as for the other two formats.
// Shared with the ciphertext formats (wire.h): the limb widths with the one 20..60 check, the pack-table row builder and the digest
// run of fhelin_debug_key_digest.  The key-set headers and tables, key_digests (whose capped keys reorder the per-vector pairs) and the
// table's upload beside the staged file stream stay here.
#include "../../include/fhelin.h"
#include <hip/hip_runtime.h>
#include <sys/stat.h>
#include <cstdio>
#include <cstring>
#include <memory>
#include "capi_internal.h"
#include "kernels_keys.h"
#include "kernels_pack.h"
#include "kernels_seeded.h"
#include "wire.h"   // limb widths, the pack-table builder and the digest run, shared with the ciphertext formats

using namespace fhelin;

namespace {

constexpr char EK_MAGIC[8] = {'F', 'H', 'E', 'L', 'I', 'N', 'E', 'K'};
constexpr char EC_MAGIC[8] = {'F', 'H', 'E', 'L', 'I', 'N', 'E', 'C'};   // compact (seeded) set
constexpr char EP_MAGIC[8] = {'F', 'H', 'E', 'L', 'I', 'N', 'E', 'P'};   // packed set, full or compact (u32 halves at 128)
constexpr uint32_t EP_VERSION = 1;
constexpr size_t EP_HEADER = 136;   // EK's 96, the key-set seed (zero for a full set), u32 halves, u32 0
constexpr uint32_t EK_VERSION = 1, EC_VERSION = 1;
constexpr uint32_t EK_VERSION_CAPS = 2;   // both magics: 48-byte table entries (the 40 of version 1, u32 max_ell, u32 0), present rows only
constexpr size_t EK_HEADER = 96, EC_HEADER = 128, EK_ENTRY = 40, EK_ENTRY_CAPS = 48, EK_ALIGN = 4096;
constexpr uint32_t EK_MAX_KEYS = 1u << 16;
constexpr size_t EK_STAGE_BYTES = size_t(4) << 20;   // per staging buffer (two of them)
enum : uint32_t { EK_PUBLIC = 0, EK_RELIN = 1, EK_ROTATION = 2, EK_CONJ = 3 };

struct EkEntry {
    uint32_t kind = 0, digits = 0;
    uint64_t galois = 0, offset = 0, words = 0, digest = 0;
    uint32_t max_ell = 0;   // n_q for the public key, for an uncapped key and for every key of a version 1 set
};
struct EkFile {
    int32_t prm[9] = {};    // log_n, n_q, first_bits, scale_bits, n_p, special_bits, dnum, log_slots, hamming
    int32_t boot[7] = {};   // budget_enc, budget_dec, slots (0: no bootstrapping set up), K, R, cheb_degree, correction
    std::vector<uint64_t> moduli;
    std::vector<EkEntry> keys;
    uint64_t data_offset = 0;
    int32_t stride = 1;       // interleave stride (header word 88: 0 = 1)
    bool compact = false;     // "FHELINEC", or "FHELINEP" with halves = 1: b halves only, a expanded from `seed`
    bool packed = false;      // "FHELINEP": every limb vector at its modulus width; 48-byte table entries, words = packed words
    uint32_t version = 1;
    uint8_t seed[32] = {};
};

struct File {
    FILE* f = nullptr;
    File(const char* path, const char* mode) : f(std::fopen(path, mode)) {}
    ~File() {
        if (f) std::fclose(f);
    }
};

const char* kind_name(uint32_t k) {
    static const char* n[] = {"public key", "relinearisation key", "rotation key", "conjugation key"};
    return k < 4 ? n[k] : "?";
}

Params to_params(const int32_t* p, int device, uint64_t seed) {
    Params q;
    q.log_n = p[0];
    q.n_q = p[1];
    q.first_bits = p[2];
    q.scale_bits = p[3];
    q.n_p = p[4];
    q.special_bits = p[5];
    q.dnum = p[6];
    q.log_slots = p[7];
    q.hamming = p[8];
    q.device = device;
    q.seed = seed;
    return q;
}
void from_params(const Params& q, int32_t* p) {
    const int32_t v[9] = {q.log_n, q.n_q, q.first_bits, q.scale_bits, q.n_p, q.special_bits, q.dnum, q.log_slots, q.hamming};
    std::memcpy(p, v, sizeof(v));
}

// header + moduli + key table, every field validated against the others and against the file's size: a malformed set is
// FHELIN_ERR_ARG before anything is allocated
EkFile read_header(const char* path) {
    File fh(path, "rb");
    if (!fh.f) throw Error(FHELIN_ERR_ARG, std::string("evaluation-key set: cannot open ") + path);
    struct stat st;
    if (fstat(fileno(fh.f), &st) != 0) throw Error(FHELIN_ERR_ARG, "evaluation-key set: cannot stat the file");
    const uint64_t fsize = (uint64_t)st.st_size;
    uint8_t h[EK_HEADER];
    if (fsize < EK_HEADER || std::fread(h, 1, EK_HEADER, fh.f) != EK_HEADER) throw Error(FHELIN_ERR_ARG, "evaluation-key set: truncated header");
    EkFile e;
    if (std::memcmp(h, EC_MAGIC, 8) == 0) e.compact = true;
    else if (std::memcmp(h, EP_MAGIC, 8) == 0) e.packed = true;
    else if (std::memcmp(h, EK_MAGIC, 8) != 0) throw Error(FHELIN_ERR_ARG, "evaluation-key set: bad magic");
    e.version = get<uint32_t>(h, 8);
    if (e.packed ? e.version != EP_VERSION : e.version != (e.compact ? EC_VERSION : EK_VERSION) && e.version != EK_VERSION_CAPS)
        throw Error(FHELIN_ERR_ARG, "evaluation-key set: unsupported version");
    const bool caps_table = e.packed || e.version == EK_VERSION_CAPS;   // 48-byte entries that carry max_ell
    const size_t entry = caps_table ? EK_ENTRY_CAPS : EK_ENTRY;
    if (e.packed) {   // seed, halves, reserved
        uint8_t x[EP_HEADER - EK_HEADER];
        if (fsize < EP_HEADER || std::fread(x, 1, sizeof(x), fh.f) != sizeof(x)) throw Error(FHELIN_ERR_ARG, "evaluation-key set: truncated header");
        std::memcpy(e.seed, x, 32);
        const uint32_t halves = get<uint32_t>(x, 32);
        if (halves < 1 || halves > 2 || get<uint32_t>(x, 36) != 0) throw Error(FHELIN_ERR_ARG, "evaluation-key set: packed set: halves must be 1 or 2");
        e.compact = halves == 1;
        if (!e.compact)
            for (uint8_t b : e.seed)
                if (b) throw Error(FHELIN_ERR_ARG, "evaluation-key set: a full packed set carries no key-set seed");
    }
    const uint64_t head = e.packed ? EP_HEADER : e.compact ? EC_HEADER : EK_HEADER;
    if (!e.packed && e.compact && (fsize < EC_HEADER || std::fread(e.seed, 1, 32, fh.f) != 32)) throw Error(FHELIN_ERR_ARG, "evaluation-key set: truncated header");
    const uint32_t n_keys = get<uint32_t>(h, 12);
    for (int i = 0; i < 9; ++i) e.prm[i] = get<int32_t>(h, 16 + 4 * i);
    for (int i = 0; i < 7; ++i) e.boot[i] = get<int32_t>(h, 52 + 4 * i);
    e.data_offset = get<uint64_t>(h, 80);
    const int log_n = e.prm[0], n_q = e.prm[1], n_p = e.prm[4];
    if (log_n < 12 || log_n > 17 || n_q < 1 || n_q > 64 || n_p < 0 || n_p > 64 || e.prm[6] < 1)
        throw Error(FHELIN_ERR_ARG, "evaluation-key set: parameters out of range");
    // the interleave stride: 0 (a set written at stride 1), or a power of two >= 2 whose physical packing fits the ring
    const uint64_t sw = get<uint64_t>(h, 88);
    if (sw == 1 || (sw & (sw - 1)) || e.prm[7] < 1 || e.prm[7] > log_n - 1 || (sw << e.prm[7]) > (1ull << (log_n - 1)))
        throw Error(FHELIN_ERR_ARG, "evaluation-key set: bad interleave stride");
    e.stride = sw ? (int32_t)sw : 1;
    const int32_t* b = e.boot;
    const bool boot_ok = b[2] == 0 ? (b[0] | b[1] | b[3] | b[4] | b[5] | b[6]) == 0
                                   : b[0] >= 1 && b[1] >= 1 && b[2] >= 4 && !(b[2] & (b[2] - 1)) && b[3] >= 1 && b[4] >= 0 && b[4] <= 8 &&
                                         b[5] >= 3 && b[5] <= 255 && b[6] >= 0 && b[6] <= 20;
    if (!boot_ok) throw Error(FHELIN_ERR_ARG, "evaluation-key set: bad bootstrap configuration");
    if (n_keys > EK_MAX_KEYS) throw Error(FHELIN_ERR_ARG, "evaluation-key set: too many keys");
    const uint64_t N = 1ull << log_n, nm = (uint64_t)n_q + n_p;
    const uint64_t table_end = head + 8 * nm + entry * (uint64_t)n_keys;
    const uint32_t alpha = ((uint32_t)n_q + (uint32_t)e.prm[6] - 1) / (uint32_t)e.prm[6];   // Context: limbs per digit
    if (fsize < table_end) throw Error(FHELIN_ERR_ARG, "evaluation-key set: truncated key table");
    e.moduli.resize(nm);
    if (std::fread(e.moduli.data(), 8, nm, fh.f) != nm) throw Error(FHELIN_ERR_ARG, "evaluation-key set: truncated moduli");
    std::vector<uint64_t> width(nm, 64);   // packed: words of one limb vector = N / 64 * width
    if (e.packed)
        for (uint64_t l = 0; l < nm; ++l) {
            width[l] = (uint64_t)pack_width(e.moduli[l]);
            if (width[l] < (uint64_t)PACK_MIN_WIDTH || width[l] > (uint64_t)PACK_MAX_WIDTH)
                throw Error(FHELIN_ERR_ARG, "evaluation-key set: packed set: a modulus outside 20..60 bits");
        }
    std::vector<uint8_t> t(entry * n_keys);
    if (n_keys && std::fread(t.data(), 1, t.size(), fh.f) != t.size()) throw Error(FHELIN_ERR_ARG, "evaluation-key set: truncated key table");
    if (e.data_offset != (table_end + EK_ALIGN - 1) / EK_ALIGN * EK_ALIGN)
        throw Error(FHELIN_ERR_ARG, "evaluation-key set: bad payload offset");
    uint64_t at = e.data_offset;
    int seen[4] = {};
    uint64_t last_g = 0;
    for (uint32_t k = 0; k < n_keys; ++k) {
        const uint8_t* r = t.data() + entry * k;
        EkEntry x;
        x.kind = get<uint32_t>(r, 0);
        x.digits = get<uint32_t>(r, 4);
        x.galois = get<uint64_t>(r, 8);
        x.offset = get<uint64_t>(r, 16);
        x.words = get<uint64_t>(r, 24);
        x.digest = get<uint64_t>(r, 32);
        x.max_ell = (uint32_t)n_q;
        if (caps_table) {
            x.max_ell = get<uint32_t>(r, 40);
            if (get<uint32_t>(r, 44) != 0) throw Error(FHELIN_ERR_ARG, "evaluation-key set: non-zero reserved word in the key table");
            if (x.max_ell < 1 || x.max_ell > (uint32_t)n_q || (x.kind == EK_PUBLIC && x.max_ell != (uint32_t)n_q))
                throw Error(FHELIN_ERR_ARG, "evaluation-key set: max_ell outside 1 .. n_q");
            if (x.kind != EK_PUBLIC && x.kind <= EK_CONJ && x.digits != (x.max_ell + alpha - 1) / alpha)
                throw Error(FHELIN_ERR_ARG, "evaluation-key set: digit count is not that of a key switch at max_ell limbs");
        }
        if (x.kind > EK_CONJ) throw Error(FHELIN_ERR_ARG, "evaluation-key set: unknown key kind");
        if (x.kind != EK_ROTATION && ++seen[x.kind] > 1) throw Error(FHELIN_ERR_ARG, "evaluation-key set: duplicate key");
        // the compact form stores the b halves only
        const uint64_t halves = e.compact ? 1 : 2;
        uint64_t want = x.kind == EK_PUBLIC ? halves * (uint64_t)n_q * N : (uint64_t)x.digits * halves * ((uint64_t)x.max_ell + n_p) * N;
        if (e.packed) {   // the same vectors, each N w / 64 words: Q limbs 0 .. max_ell-1, then (switching keys) the special limbs
            uint64_t bits = 0;
            for (uint64_t l = 0; l < x.max_ell; ++l) bits += width[l];
            for (uint64_t l = 0; x.kind != EK_PUBLIC && l < (uint64_t)n_p; ++l) bits += width[(uint64_t)n_q + l];
            want = (x.kind == EK_PUBLIC ? halves : (uint64_t)x.digits * halves) * bits * (N / 64);
        }
        if ((x.kind == EK_PUBLIC) != (x.digits == 0) || x.digits > (uint32_t)n_q || x.words != want)
            throw Error(FHELIN_ERR_ARG, "evaluation-key set: key size does not match the parameters");
        const uint64_t g_want = x.kind == EK_CONJ ? 2 * N - 1 : 0;
        if (x.kind == EK_ROTATION) {
            if (!(x.galois & 1) || x.galois >= 2 * N - 1 || x.galois <= last_g)
                throw Error(FHELIN_ERR_ARG, "evaluation-key set: bad or unordered Galois element");
            last_g = x.galois;
        } else if (x.galois != g_want) {
            throw Error(FHELIN_ERR_ARG, "evaluation-key set: bad Galois element");
        }
        if (x.offset != at || x.digest >= KEY_DIGEST_P) throw Error(FHELIN_ERR_ARG, "evaluation-key set: bad key table entry");
        at += 8 * x.words;
        e.keys.push_back(x);
    }
    if (fsize != at) throw Error(FHELIN_ERR_ARG, "evaluation-key set: file size does not match the key table (truncated?)");
    return e;
}

// the host-only parameter context of the header: its prime chain must be the file's
void check_moduli(const EkFile& e, const std::vector<u64>& moduli) {
    if (moduli.size() != e.moduli.size() || std::memcmp(moduli.data(), e.moduli.data(), 8 * moduli.size()) != 0)
        throw Error(FHELIN_ERR_ARG, "evaluation-key set: moduli do not match the parameters");
}

struct Pinned {
    void* p[2] = {};
    hipEvent_t ev[2] = {};
    bool used[2] = {};
    hipStream_t s;
    explicit Pinned(hipStream_t st) : s(st) {
        for (int i = 0; i < 2; ++i) {
            hip_check(hipHostMalloc(&p[i], EK_STAGE_BYTES, hipHostMallocDefault), "hipHostMalloc(key staging)");
            hip_check(hipEventCreateWithFlags(&ev[i], hipEventDisableTiming), "hipEventCreate(key staging)");
        }
    }
    void wait(int i) {
        if (used[i]) hip_check(hipEventSynchronize(ev[i]), "hipEventSynchronize(key staging)");
        used[i] = false;
    }
    ~Pinned() {
        (void)hipStreamSynchronize(s);
        for (int i = 0; i < 2; ++i) {
            if (p[i]) (void)hipHostFree(p[i]);
            if (ev[i]) (void)hipEventDestroy(ev[i]);
        }
    }
};

struct Seg {
    u64* d;
    size_t words;
    // > 0: a capped switching key [digits][2][n_q + n_p][N] at d; words counts its PRESENT rows, [digits][2][max_ell + n_p][N]
    int max_ell = 0;
    int digits = 0;
    // a run of rows that is written or read (the packed formats pack row by row): row r belongs to limb limb0 + r % limbs
    int limb0 = 0;
    int limbs = 0;
};

// the runs of a capped key's present rows in storage order ([digits][halves][max_ell + n_p][N]; halves 1: the b halves): per digit and
// half the Q rows 0 .. max_ell-1, then the special rows, where they lie in the full-stride layout
void present_runs(std::vector<Seg>& out, const Context& x, u64* d, int digits, int halves, int max_ell) {
    const size_t N = x.N, nl = (size_t)x.L + 1 + x.K;
    for (int j = 0; j < digits; ++j)
        for (int h = 0; h < halves; ++h) {
            u64* base = d + ((size_t)2 * j + h) * nl * N;
            out.push_back(Seg{base, (size_t)max_ell * N, 0, 0, 0, max_ell});
            out.push_back(Seg{base + (size_t)(x.L + 1) * N, (size_t)x.K * N, 0, 0, x.L + 1, x.K});
        }
}

// per-vector digests / range flags of every key on the device, folded into one digest per key on the host.  ok[k] = every
// residue of key k below its limb's modulus.
void key_digests(Context& x, const std::vector<Seg>& segs, const std::vector<uint32_t>& kinds, std::vector<uint64_t>& digest,
                 std::vector<char>& ok) {
    const size_t N = x.N;
    size_t total = 0, max_vec = 0;
    for (const Seg& s : segs) {
        total += s.words / N;
        max_vec = std::max(max_vec, s.words / N);
    }
    digest.assign(segs.size(), 0);
    ok.assign(segs.size(), 1);
    if (!total) return;
    Scratch<u64> part = x.scratch<u64>(key_digest_scratch_words(x.N, (int)max_vec));
    Scratch<u64> out = x.scratch<u64>(2 * total);
    size_t v0 = 0;
    for (size_t k = 0; k < segs.size(); ++k) {
        const int n_vec = (int)(segs[k].words / N);
        const int limb_count = kinds[k] == EK_PUBLIC ? x.L + 1 : x.L + 1 + x.K;
        if (segs[k].max_ell > 0) {
            // a capped key's present rows where they lie (row-to-limb mapping of version 2: stored row r of a group is Q limb r below
            // max_ell, else special limb r - max_ell): the Q rows of all groups, then the special rows of all groups; folded in storage
            // order below
            const int groups = 2 * segs[k].digits, mq = segs[k].max_ell;
            launch_key_digest_strided(x.dt, segs[k].d, groups * mq, 0, mq, limb_count, part, out + 2 * v0, x.stream);
            launch_key_digest_strided(x.dt, segs[k].d + (size_t)(x.L + 1) * N, groups * x.K, x.L + 1, x.K, limb_count, part,
                                      out + 2 * (v0 + (size_t)groups * mq), x.stream);
        } else {
            launch_key_digest(x.dt, segs[k].d, n_vec, 0, limb_count, part, out + 2 * v0, x.stream);
        }
        v0 += n_vec;
    }
    hip_check(hipGetLastError(), "key digest kernels");
    std::vector<u64> h(2 * total);
    hip_check(hipMemcpyAsync(h.data(), out, h.size() * 8, hipMemcpyDeviceToHost, x.stream), "key digest download");
    hip_check(hipStreamSynchronize(x.stream), "key digest sync");
    part.reset();
    out.reset();
    v0 = 0;
    for (size_t k = 0; k < segs.size(); ++k) {
        const size_t n_vec = segs[k].words / N;
        bool in_range;
        if (segs[k].max_ell > 0) {   // device order (all Q rows, all special rows) -> storage order (per group: Q rows, special rows)
            const size_t groups = (size_t)2 * segs[k].digits, mq = (size_t)segs[k].max_ell, K = (size_t)x.K;
            std::vector<u64> st(2 * n_vec);
            for (size_t g = 0; g < groups; ++g)
                for (size_t r = 0; r < mq + K; ++r) {
                    const size_t from = r < mq ? g * mq + r : groups * mq + g * K + (r - mq), to = g * (mq + K) + r;
                    st[2 * to] = h[2 * (v0 + from)];
                    st[2 * to + 1] = h[2 * (v0 + from) + 1];
                }
            std::copy(st.begin(), st.end(), h.begin() + 2 * v0);
        }
        digest[k] = fold_key_digest(&h[2 * v0], n_vec, in_range);
        ok[k] = in_range ? 1 : 0;
        v0 += n_vec;
    }
}

// packed sets: the rows of runs[lo, hi) in order, one table entry each; the packed vectors lie back to back from `packed` on.  unpack:
// packed -> rows, else rows -> packed.  Returns the packed words.
size_t pack_table(std::vector<PackEntry>& tab, const Context& x, const std::vector<Seg>& runs, size_t lo, size_t hi, u64* packed, bool unpack) {
    size_t at = 0;
    for (size_t i = lo; i < hi; ++i) {
        std::vector<int> width;
        limb_widths(x, runs[i].limb0, runs[i].limbs, "packed key set", &width);
        at += pack_rows(tab, x.N, runs[i].d, runs[i].words / x.N, width.data(), runs[i].limbs, packed + at, unpack);
    }
    return at;
}
size_t packed_words_of(const Context& x, const std::vector<Seg>& runs, size_t lo, size_t hi) {
    std::vector<PackEntry> t;
    return pack_table(t, x, runs, lo, hi, nullptr, false);
}
void check_pack_widths(const Context& x) { limb_widths(x, 0, (int)x.moduli.size(), "packed key set"); }

bool fresh(const fhelin_ctx* c) {
    if (c->cl.keygen_run() || c->cl.eval_only() || c->cl.has_public_key() || c->ev.relin_key || c->ev.conj_key || c->boot.ready())
        return false;
    for (const auto& kv : c->ev.rot_keys)
        if (kv.second) return false;
    return true;
}

std::string key_what(uint32_t kind, uint64_t galois) {
    return std::string(kind_name(kind)) + (kind == EK_ROTATION ? " (Galois element " + std::to_string(galois) + ")" : "");
}

// v1 (full keys) or compact (b halves and the key-set seed): the same table, digests of the full keys in both.  packed: "FHELINEP", the
// same rows in the same order at their modulus widths; the two unpacked forms are written exactly as before
void save_set(fhelin_ctx* c, const char* path, bool compact, bool packed = false) {
    Context& x = c->ctx;
    x.require_device();
    x.sync();
    const u64 g_conj = 2ull * x.N - 1;
    std::vector<Seg> segs;
    std::vector<EkEntry> ents;
    std::vector<char> seeded;
    bool any_capped = false;   // then version 2: 48-byte entries, capped keys as their present rows; else version 1, byte for byte
    auto add = [&](uint32_t kind, uint32_t digits, uint64_t g, u64* d, size_t words, bool sd) {
        EkEntry e;
        e.kind = kind;
        e.digits = digits;
        e.galois = g;
        e.words = words;
        e.max_ell = (uint32_t)(x.L + 1);
        ents.push_back(e);
        segs.push_back({d, words});
        seeded.push_back(sd);
    };
    auto add_key = [&](uint32_t kind, uint64_t g, const EvalKey& k) {
        add(kind, k.digits, g, k.d, k.words(), k.seeded);
        if (!k.capped()) return;
        any_capped = true;
        const size_t present = (size_t)k.digits * 2 * (k.max_ell + x.K) * x.N;
        ents.back().max_ell = (uint32_t)k.max_ell;
        ents.back().words = present;
        segs.back() = Seg{k.d, present, k.max_ell, k.digits};
    };
    if (c->cl.has_public_key())
        add(EK_PUBLIC, 0, 0, const_cast<u64*>(c->cl.public_key()), (size_t)2 * (x.L + 1) * x.N, c->cl.public_key_seeded());
    const KeyPtr& rk = c->ev.relin_key;
    const KeyPtr& ck = c->ev.conj_key;
    if (rk) add_key(EK_RELIN, 0, *rk);
    if (ck) add_key(EK_CONJ, g_conj, *ck);
    for (const auto& kv : c->ev.rot_keys)   // ordered by Galois element; the conjugation key is stored once, above
        if (kv.second && kv.first != g_conj) add_key(EK_ROTATION, kv.first, *kv.second);
    if (ents.empty()) throw Error(FHELIN_ERR_KEY, "evalkeys_save: the context holds no keys");
    if (ents.size() > EK_MAX_KEYS) throw Error(FHELIN_ERR_ARG, "evalkeys_save: too many keys");
    if (x.N % 4096) throw Error(FHELIN_ERR_ARG, "evalkeys_save: ring dimension below 2^12");
    if (packed) check_pack_widths(x);
    if (compact) {
        if (!c->cl.has_key_seed())
            throw Error(FHELIN_ERR_STATE, "evalkeys_save_compact: the keys are not seeded (fhelin_ctx_set_seeded_keys before fhelin_keygen)");
        for (size_t k = 0; k < ents.size(); ++k)
            if (!seeded[k])
                throw Error(FHELIN_ERR_STATE, "evalkeys_save_compact: the " + key_what(ents[k].kind, ents[k].galois) +
                                                  " is not seeded (imported or made outside seeded-key mode)");
    }

    std::vector<uint32_t> kinds;
    for (const auto& e : ents) kinds.push_back(e.kind);
    std::vector<uint64_t> digest;
    std::vector<char> ok;
    key_digests(x, segs, kinds, digest, ok);
    for (size_t k = 0; k < ents.size(); ++k) {
        if (!ok[k]) throw Error(FHELIN_ERR_INTERNAL, std::string("evalkeys_save: ") + kind_name(ents[k].kind) + " holds a residue out of range");
        ents[k].digest = digest[k];
    }
    // what is written: every key whole, or the b half of every digit
    std::vector<Seg> out;
    std::vector<size_t> out_begin;   // first run of key k (and the end, last)
    for (size_t k = 0; k < ents.size(); ++k) {
        out_begin.push_back(out.size());
        const int rows = ents[k].kind == EK_PUBLIC ? x.L + 1 : x.L + 1 + x.K;   // limbs per half of an uncapped key
        if (compact) {
            const size_t half = (size_t)rows * x.N;
            const uint32_t nd = ents[k].kind == EK_PUBLIC ? 1 : ents[k].digits;
            if (segs[k].max_ell > 0) present_runs(out, x, segs[k].d, segs[k].digits, 1, segs[k].max_ell);
            else
                for (uint32_t j = 0; j < nd; ++j) out.push_back(Seg{segs[k].d + (size_t)2 * j * half, half, 0, 0, 0, rows});
            ents[k].words /= 2;
        } else {
            if (segs[k].max_ell > 0) present_runs(out, x, segs[k].d, segs[k].digits, 2, segs[k].max_ell);
            else out.push_back(Seg{segs[k].d, segs[k].words, 0, 0, 0, rows});
        }
    }
    out_begin.push_back(out.size());
    // packed: one table for the whole set (key k's rows -> one scratch block, reused key after key in stream order)
    Scratch<u64> pk_scratch;
    Scratch<PackEntry> pk_dtab;
    std::vector<PackEntry> pk_tab;
    std::vector<size_t> pk_tab_begin;
    if (packed) {
        size_t most = 0;
        for (size_t k = 0; k < ents.size(); ++k) {
            ents[k].words = packed_words_of(x, out, out_begin[k], out_begin[k + 1]);
            most = std::max(most, (size_t)ents[k].words);
        }
        pk_scratch = x.scratch<u64>(most);
        for (size_t k = 0; k < ents.size(); ++k) {
            pk_tab_begin.push_back(pk_tab.size());
            pack_table(pk_tab, x, out, out_begin[k], out_begin[k + 1], pk_scratch, false);
        }
        pk_tab_begin.push_back(pk_tab.size());
        pk_dtab = x.scratch<PackEntry>(pk_tab.size());
        hip_check(hipMemcpyAsync(pk_dtab, pk_tab.data(), pk_tab.size() * sizeof(PackEntry), hipMemcpyHostToDevice, x.stream), "pack table upload");
    }

    const size_t nm = x.moduli.size();
    const size_t head = packed ? EP_HEADER : compact ? EC_HEADER : EK_HEADER;
    const size_t entry = any_capped || packed ? EK_ENTRY_CAPS : EK_ENTRY;
    const uint64_t table_end = head + 8 * nm + entry * ents.size();
    const uint64_t data_offset = (table_end + EK_ALIGN - 1) / EK_ALIGN * EK_ALIGN;
    std::vector<uint8_t> h(data_offset, 0);
    std::memcpy(h.data(), packed ? EP_MAGIC : compact ? EC_MAGIC : EK_MAGIC, 8);
    put<uint32_t>(h.data(), 8, packed ? EP_VERSION : any_capped ? EK_VERSION_CAPS : compact ? EC_VERSION : EK_VERSION);
    put<uint32_t>(h.data(), 12, (uint32_t)ents.size());
    int32_t prm[9];
    from_params(x.prm, prm);
    std::memcpy(h.data() + 16, prm, sizeof(prm));
    if (c->boot.ready()) {
        const int32_t b[7] = {c->boot.budget_enc(), c->boot.budget_dec(), c->boot.logical_slots(), c->boot.K, c->boot.R, c->boot.cheb_degree,
                              c->boot.correction};
        std::memcpy(h.data() + 52, b, sizeof(b));
    }
    put<uint64_t>(h.data(), 80, data_offset);
    if (x.stride != 1) put<uint64_t>(h.data(), 88, (uint64_t)x.stride);   // a set written at stride 1 keeps 0 here
    if (compact) std::memcpy(h.data() + EK_HEADER, c->cl.key_seed(), 32);
    if (packed) put<uint32_t>(h.data(), 128, compact ? 1u : 2u);   // halves; then u32 0
    std::memcpy(h.data() + head, x.moduli.data(), 8 * nm);
    uint64_t at = data_offset;
    for (size_t k = 0; k < ents.size(); ++k) {
        ents[k].offset = at;
        at += 8 * ents[k].words;
        const size_t o = head + 8 * nm + entry * k;
        if (any_capped || packed) put<uint32_t>(h.data(), o + 40, ents[k].max_ell);   // then u32 0 (reserved)
        put<uint32_t>(h.data(), o, ents[k].kind);
        put<uint32_t>(h.data(), o + 4, ents[k].digits);
        put<uint64_t>(h.data(), o + 8, ents[k].galois);
        put<uint64_t>(h.data(), o + 16, ents[k].offset);
        put<uint64_t>(h.data(), o + 24, ents[k].words);
        put<uint64_t>(h.data(), o + 32, ents[k].digest);
    }

    bool written = false;
    {
        File fh(path, "wb");
        if (!fh.f) throw Error(FHELIN_ERR_ARG, std::string("evalkeys_save: cannot create ") + path);
        bool io_ok = std::fwrite(h.data(), 1, h.size(), fh.f) == h.size();
        // payloads: device -> pinned buffer b while the host writes the other buffer's previous chunk
        Pinned stg(x.stream);
        int cur = 0;
        size_t pend_bytes[2] = {};
        // packed: key k is packed into the scratch block (in stream order behind the downloads of key k - 1) and that block is streamed
        std::vector<Seg> packed_runs;
        for (size_t k = 0; packed && k < ents.size(); ++k) packed_runs.push_back({pk_scratch, (size_t)ents[k].words});
        const std::vector<Seg>& runs = packed ? packed_runs : out;
        for (size_t i = 0; i < runs.size(); ++i) {
            const Seg& s = runs[i];
            if (packed && io_ok) {
                launch_pack_residues(pk_dtab + pk_tab_begin[i], (int)(pk_tab_begin[i + 1] - pk_tab_begin[i]), x.N, x.stream);
                hip_check(hipGetLastError(), "pack kernel");
            }
            const size_t bytes = s.words * 8;
            for (size_t off = 0; off < bytes && io_ok; off += EK_STAGE_BYTES) {
                const size_t n = std::min(EK_STAGE_BYTES, bytes - off);
                hip_check(hipMemcpyAsync(stg.p[cur], reinterpret_cast<const char*>(s.d) + off, n, hipMemcpyDeviceToHost, x.stream),
                          "key download");
                hip_check(hipEventRecord(stg.ev[cur], x.stream), "hipEventRecord(key staging)");
                stg.used[cur] = true;
                pend_bytes[cur] = n;
                const int prev = cur ^ 1;
                if (stg.used[prev]) {
                    stg.wait(prev);
                    io_ok = std::fwrite(stg.p[prev], 1, pend_bytes[prev], fh.f) == pend_bytes[prev];
                }
                cur = prev;
            }
        }
        const int last = cur ^ 1;
        if (io_ok && stg.used[last]) {
            stg.wait(last);
            io_ok = std::fwrite(stg.p[last], 1, pend_bytes[last], fh.f) == pend_bytes[last];
        }
        written = io_ok && std::fflush(fh.f) == 0;
    }
    if (!written) {
        std::remove(path);
        throw Error(FHELIN_ERR_ARG, std::string("evalkeys_save: write to ") + path + " failed");
    }
}

}  // namespace

extern "C" {

int fhelin_evalkeys_params(const char* path, fhelin_params* out) {
    if (!path || !out) return capi_fail(FHELIN_ERR_ARG, "null argument");
    FHELIN_TRY
    EkFile e = read_header(path);
    Context host(to_params(e.prm, -1, 1));   // host-only: the prime chain the parameters give
    check_moduli(e, host.moduli);
    Params q = to_params(e.prm, 0, 0);
    fhelin_params r{q.log_n, q.n_q, q.first_bits, q.scale_bits, q.n_p, q.special_bits, q.dnum, q.log_slots, q.hamming, 0, 0};
    *out = r;
    FHELIN_CATCH
}

int fhelin_evalkeys_info(const char* path, int32_t* boot7, int32_t* n_keys) {
    if (!path) return capi_fail(FHELIN_ERR_ARG, "null argument");
    FHELIN_TRY
    EkFile e = read_header(path);
    if (boot7) std::memcpy(boot7, e.boot, sizeof(e.boot));
    if (n_keys) *n_keys = (int32_t)e.keys.size();
    FHELIN_CATCH
}

int fhelin_evalkeys_interleave(const char* path, int32_t* stride) {
    if (!path || !stride) return capi_fail(FHELIN_ERR_ARG, "null argument");
    FHELIN_TRY
    *stride = read_header(path).stride;
    FHELIN_CATCH
}

int fhelin_evalkeys_save(fhelin_ctx* c, const char* path) {
    if (!c || !path) return capi_fail(FHELIN_ERR_ARG, "null argument");
    FHELIN_TRY
    save_set(c, path, false);
    FHELIN_CATCH
}

int fhelin_evalkeys_save_compact(fhelin_ctx* c, const char* path) {
    if (!c || !path) return capi_fail(FHELIN_ERR_ARG, "null argument");
    FHELIN_TRY
    save_set(c, path, true);
    FHELIN_CATCH
}

int fhelin_evalkeys_save_packed(fhelin_ctx* c, const char* path, int32_t compact) {
    if (!c || !path) return capi_fail(FHELIN_ERR_ARG, "null argument");
    FHELIN_TRY
    save_set(c, path, compact != 0, true);
    FHELIN_CATCH
}

int fhelin_ctx_set_seeded_keys(fhelin_ctx* c, int32_t on) {
    if (!c) return capi_fail(FHELIN_ERR_ARG, "null argument");
    FHELIN_TRY
    if (c->cl.eval_only()) throw Error(FHELIN_ERR_KEY, "set_seeded_keys: an evaluation context holds no secret and makes no keys");
    if (!fresh(c)) throw Error(FHELIN_ERR_STATE, "set_seeded_keys: call it before keygen, while the context holds no key");
    c->cl.set_seeded_keys(on != 0);
    FHELIN_CATCH
}

int fhelin_ctx_key_set_seed(const fhelin_ctx* c, uint8_t* out32) {
    if (!c || !out32) return capi_fail(FHELIN_ERR_ARG, "null argument");
    if (!c->cl.has_key_seed()) return capi_fail(FHELIN_ERR_STATE, "key_set_seed: the keys are not seeded");
    std::memcpy(out32, c->cl.key_seed(), 32);
    return FHELIN_OK;
}

int fhelin_evalkeys_load(fhelin_ctx* c, const char* path) {
    if (!c || !path) return capi_fail(FHELIN_ERR_ARG, "null argument");
    FHELIN_TRY
    Context& x = c->ctx;
    x.require_device();
    EkFile e = read_header(path);
    if (!fresh(c)) throw Error(FHELIN_ERR_STATE, "evalkeys_load: the context must be fresh (no keygen, no keys, no bootstrap set-up)");
    int32_t prm[9];
    from_params(x.prm, prm);
    if (std::memcmp(prm, e.prm, sizeof(prm)) != 0) throw Error(FHELIN_ERR_STATE, "evalkeys_load: the set was made for other parameters");
    check_moduli(e, x.moduli);
    // the set's interleave stride: adopted, unless this context was told another one
    if (e.stride != x.stride) {
        if (x.stride_explicit) throw Error(FHELIN_ERR_STATE, "evalkeys_load: the set was written at interleave stride " + std::to_string(e.stride) +
                                                                 ", the context was set to " + std::to_string(x.stride));
        if (x.stride_locked) throw Error(FHELIN_ERR_STATE, "evalkeys_load: the set has another interleave stride than the plaintexts or ciphertexts the context already holds");
    }
    for (const auto& k : e.keys)
        if (k.kind != EK_PUBLIC && (int)k.digits != x.digits_at((int)k.max_ell))
            throw Error(FHELIN_ERR_ARG, "evalkeys_load: switching key digit count does not match the context");

    // destinations: nothing is installed until every key has passed (their owners free the blocks on any failure)
    Scratch<u64> pk;
    std::vector<KeyPtr> sw(e.keys.size());
    std::vector<Seg> segs;
    std::vector<uint32_t> kinds;
    for (size_t k = 0; k < e.keys.size(); ++k) {
        if (e.keys[k].kind == EK_PUBLIC) {
            const size_t pk_words = (size_t)2 * (x.L + 1) * x.N;   // the whole key (a compact entry's words count its b half)
            pk = x.scratch<u64>(pk_words);
            segs.push_back({pk, pk_words});
        } else {
            sw[k] = c->ev.new_key((int)e.keys[k].max_ell);   // a capped key: zero-filled, the payload lands in its present rows
            if (sw[k]->capped())
                segs.push_back(Seg{sw[k]->d, (size_t)sw[k]->digits * 2 * (sw[k]->max_ell + x.K) * x.N, sw[k]->max_ell, sw[k]->digits});
            else
                segs.push_back({sw[k]->d, sw[k]->words()});
        }
        kinds.push_back(e.keys[k].kind);
    }
    // what the file holds: every key whole, or the b half of every digit (the a halves are expanded below)
    std::vector<Seg> in;
    std::vector<size_t> in_begin;   // first run of key k (and the end, last)
    std::vector<SeededEntry> tab;
    if (e.compact) {
        SamplerKey sk;
        for (int w = 0; w < 8; ++w) sk.w[w] = get<uint32_t>(e.seed, 4 * w);
        for (size_t k = 0; k < e.keys.size(); ++k) {
            in_begin.push_back(in.size());
            const bool pub = e.keys[k].kind == EK_PUBLIC;
            const int ell = pub ? x.L + 1 : x.L + 1 + x.K;
            const size_t half = (size_t)ell * x.N;
            const uint32_t nd = pub ? 1 : e.keys[k].digits;
            if (segs[k].max_ell > 0) present_runs(in, x, segs[k].d, segs[k].digits, 1, segs[k].max_ell);
            for (uint32_t j = 0; j < nd; ++j) {
                if (segs[k].max_ell == 0) in.push_back(Seg{segs[k].d + (size_t)2 * j * half, half, 0, 0, 0, ell});
                SeededEntry se;
                se.key = sk;
                se.nonce = key_nonce(e.keys[k].kind, j, e.keys[k].galois);
                se.dst = segs[k].d + (size_t)(2 * j + 1) * half;
                se.ell = ell;
                if (segs[k].max_ell > 0) {   // the a half of the present rows only, each at its absolute limb
                    se.ell = segs[k].max_ell + x.K;
                    se.split = segs[k].max_ell;
                    se.skip = x.L + 1 - segs[k].max_ell;
                }
                tab.push_back(se);
            }
        }
    } else {
        for (size_t k = 0; k < segs.size(); ++k) {
            const Seg& s = segs[k];
            in_begin.push_back(in.size());
            if (s.max_ell > 0) present_runs(in, x, s.d, s.digits, 2, s.max_ell);
            else in.push_back(Seg{s.d, s.words, 0, 0, 0, kinds[k] == EK_PUBLIC ? x.L + 1 : x.L + 1 + x.K});
        }
    }
    in_begin.push_back(in.size());
    // packed: what is read is key k's packed payload, into one scratch block (reused key after key in stream order), and unpacked
    // from there into the rows the unpacked formats are read into
    Scratch<u64> pk_scratch;
    Scratch<PackEntry> pk_dtab;
    std::vector<PackEntry> pk_tab;
    std::vector<size_t> pk_tab_begin;
    std::vector<Seg> packed_runs;
    if (e.packed) {
        if (x.N % 4096) throw Error(FHELIN_ERR_ARG, "evalkeys_load: ring dimension below 2^12");
        size_t most = 0;
        for (const auto& k : e.keys) most = std::max(most, (size_t)k.words);
        pk_scratch = x.scratch<u64>(most);
        for (size_t k = 0; k < e.keys.size(); ++k) {
            pk_tab_begin.push_back(pk_tab.size());
            if (pack_table(pk_tab, x, in, in_begin[k], in_begin[k + 1], pk_scratch, true) != e.keys[k].words)
                throw Error(FHELIN_ERR_ARG, "evalkeys_load: packed key size does not match the context");
            packed_runs.push_back({pk_scratch, (size_t)e.keys[k].words});
        }
        pk_tab_begin.push_back(pk_tab.size());
        pk_dtab = x.scratch<PackEntry>(pk_tab.size());
        hip_check(hipMemcpyAsync(pk_dtab, pk_tab.data(), pk_tab.size() * sizeof(PackEntry), hipMemcpyHostToDevice, x.stream), "unpack table upload");
    }
    {
        const std::vector<Seg>& runs = e.packed ? packed_runs : in;
        File fh(path, "rb");
        if (!fh.f || std::fseek(fh.f, (long)e.data_offset, SEEK_SET) != 0) throw Error(FHELIN_ERR_ARG, "evalkeys_load: cannot read the payloads");
        // file -> pinned buffer b while buffer b^1's previous chunk is on its way to the device
        Pinned stg(x.stream);
        int cur = 0;
        for (size_t i = 0; i < runs.size(); ++i) {
            const Seg& s = runs[i];
            const size_t bytes = s.words * 8;
            for (size_t off = 0; off < bytes; off += EK_STAGE_BYTES) {
                const size_t n = std::min(EK_STAGE_BYTES, bytes - off);
                stg.wait(cur);
                if (std::fread(stg.p[cur], 1, n, fh.f) != n) throw Error(FHELIN_ERR_ARG, "evalkeys_load: truncated payload");
                hip_check(hipMemcpyAsync(reinterpret_cast<char*>(s.d) + off, stg.p[cur], n, hipMemcpyHostToDevice, x.stream), "key upload");
                hip_check(hipEventRecord(stg.ev[cur], x.stream), "hipEventRecord(key staging)");
                stg.used[cur] = true;
                cur ^= 1;
            }
            if (e.packed) {
                launch_unpack_residues(pk_dtab + pk_tab_begin[i], (int)(pk_tab_begin[i + 1] - pk_tab_begin[i]), x.N, x.stream);
                hip_check(hipGetLastError(), "unpack kernel");
            }
        }
    }
    if (!tab.empty()) {   // every a half of the set: one launch (per 65535 key digits), before the digests see the full keys
        Scratch<SeededEntry> dt = x.scratch<SeededEntry>(tab.size());
        hip_check(hipMemcpyAsync(dt, tab.data(), tab.size() * sizeof(SeededEntry), hipMemcpyHostToDevice, x.stream), "seed table upload");
        const int max_ell = x.L + 1 + x.K;
        for (size_t lo = 0; lo < tab.size(); lo += 65535)
            launch_seeded_expand(x.dt, dt + lo, (int)std::min<size_t>(65535, tab.size() - lo), max_ell, x.stream);
        hip_check(hipGetLastError(), "seeded expand kernel");
    }
    std::vector<uint64_t> digest;
    std::vector<char> ok;
    key_digests(x, segs, kinds, digest, ok);
    for (size_t k = 0; k < e.keys.size(); ++k) {
        const auto& ek = e.keys[k];
        const std::string what = key_what(ek.kind, ek.galois);
        if (!ok[k]) throw Error(FHELIN_ERR_ARG, "evalkeys_load: " + what + " holds a residue not below its modulus");
        if (digest[k] != ek.digest) throw Error(FHELIN_ERR_ARG, "evalkeys_load: " + what + " does not match its digest");
    }

    // install
    x.stride = e.stride;
    for (size_t k = 0; k < e.keys.size(); ++k) {
        if (sw[k]) {
            sw[k]->seeded = e.compact;
            sw[k]->kind = (int)e.keys[k].kind;   // the file's numbering is EvalKey::kind's
            sw[k]->galois = e.keys[k].galois;
        }
        switch (e.keys[k].kind) {
            case EK_RELIN: c->ev.relin_key = sw[k]; break;
            case EK_CONJ:
                c->ev.conj_key = sw[k];
                c->ev.rot_keys[2ull * x.N - 1] = sw[k];
                break;
            case EK_ROTATION: c->ev.rot_keys[e.keys[k].galois] = sw[k]; break;
            default: break;
        }
    }
    c->cl.install_public_key(pk.release(), e.compact);
    if (e.compact) c->cl.install_key_seed(e.seed);
    if (e.boot[2] > 0) {   // the client's approximation parameters; fhelin_bootstrap_setup is the caller's (fhelin_evalkeys_info)
        c->boot.K = e.boot[3];
        c->boot.R = e.boot[4];
        c->boot.cheb_degree = e.boot[5];
        c->boot.correction = e.boot[6];
    }
    FHELIN_CATCH
}

int fhelin_debug_key_digest(fhelin_ctx* c, const uint64_t* words, int32_t n_limbs, int32_t limb_first, uint64_t* out_digests,
                            int32_t* out_ok) {
    if (!c || !words || !out_digests || !out_ok) return capi_fail(FHELIN_ERR_ARG, "null argument");
    FHELIN_TRY
    Context& x = c->ctx;
    x.require_device();
    if (n_limbs < 1 || limb_first < 0 || limb_first + n_limbs > x.L + 1 + x.K) throw Error(FHELIN_ERR_ARG, "debug_key_digest: limbs out of range");
    if (x.N % 4096) throw Error(FHELIN_ERR_ARG, "debug_key_digest: ring dimension below 2^12");
    const size_t n = (size_t)n_limbs * x.N;
    Scratch<u64> d = x.scratch<u64>(n);
    hip_check(hipMemcpyAsync(d, words, n * 8, hipMemcpyHostToDevice, x.stream), "debug digest upload");
    DigestRun run(x, {DigestItem{d, (size_t)n_limbs, limb_first, n_limbs, n_limbs}});
    hip_check(hipStreamSynchronize(x.stream), "debug digest sync");
    const u64* h = run.pairs(0);
    for (int i = 0; i < n_limbs; ++i) {
        out_digests[i] = h[2 * i];
        out_ok[i] = (int32_t)h[2 * i + 1];
    }
    FHELIN_CATCH
}

}  // extern "C"
