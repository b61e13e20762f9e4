// extern "C" boundary, part 4: evaluation-key sets (include/fhelin.h "Evaluation-key sets" and "Seeded evaluation keys": both file
// formats are documented there).  A client context writes its public key and every switching key it holds; a context that never
// held a secret loads them and evaluates with them alone.  Every key is range-checked and digested on the device (kernels_keys.hip)
// on the way out and on the way in; the file is streamed through two pinned staging buffers, so host memory stays bounded by them.
// A compact set ("FHELINEC") stores the b halves and the key-set seed; the loader expands every a half in one launch
// (kernels_seeded.hip) before it digests.
// Version 2 of both formats (include/fhelin.h "Level-capped keys") stores the present rows of capped keys only.  Payloads are dense in
// the file and full-stride on the device: the staging pipeline copies run by run (one run of Q rows and one of special rows per digit
// and half - plain 1D copies, a few MB each at driver scale), and the digest reads the rows where they lie through the strided digest
// launch (kernels_keys.h), one item for the Q rows and one for the special rows of a key.  No scatter kernel: a scatter would need
// the dense payload in device memory first, which is exactly the copy the cap saves.
// A packed set ("FHELINEP", include/fhelin.h "Packed formats") holds the same present rows, every limb vector at its modulus width: one
// key at a time is packed into (or unpacked out of) a scratch block of one key's packed payload, which is what the staging pipeline then
// streams; digests are those of the unpacked residues, computed by the same run as for the other two formats.
// Elsewhere: the five headers and tables, every check of a file's fields and the payload size of a key are keyset_header.h (no device,
// no I/O); limb widths, the pack-table rows with their staged upload and the digest run are wire.h, shared with the ciphertext formats.
// What stays here is what saver and loader share on the device - a key's runs in storage order (key_runs), a set's packed plan (PackPlan),
// the staged file stream (Pinned::to_file / from_file), the per-key digests (key_digests) - and save_set and fhelin_evalkeys_load themselves.
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
#include "keyset_header.h"   // formats, EkFile / EkEntry, reader and writer, the payload size of a key
#include "wire.h"            // limb widths, the pack-table builder and its upload, the digest run: shared with the ciphertext formats

using namespace fhelin;

namespace {

constexpr size_t EK_STAGE_BYTES = size_t(4) << 20;   // per staging buffer (two of them)

struct File {
    FILE* f = nullptr;
    File(const char* path, const char* mode) : f(std::fopen(path, mode)) {}
    ~File() {
        if (f) std::fclose(f);
    }
};

const char* kind_name(uint32_t k) {
    static const char* n[] = {"public key", "relinearisation key", "rotation key", "conjugation key", "to-sparse key", "from-sparse key"};
    return k < EK_KINDS ? n[k] : "?";
}

Params to_params(const int32_t* p, int device, uint64_t seed) {
    static_assert(offsetof(Params, log_n) == 0 && offsetof(Params, n_q) == 4 && offsetof(Params, first_bits) == 8 && offsetof(Params, scale_bits) == 12 &&
                      offsetof(Params, n_p) == 16 && offsetof(Params, special_bits) == 20 && offsetof(Params, dnum) == 24 && offsetof(Params, log_slots) == 28 &&
                      offsetof(Params, hamming) == 32 && offsetof(Params, seed) == 40, "the header's nine parameters are Params' first members, in this order, then seed");
    Params q{p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7], p[8], seed};
    q.device = device;
    return q;
}
void from_params(const Params& q, int32_t* p) {
    const int32_t v[9] = {q.log_n, q.n_q, q.first_bits, q.scale_bits, q.n_p, q.special_bits, q.dnum, q.log_slots, q.hamming};
    std::memcpy(p, v, sizeof(v));
}

// header + moduli + key table (keyset_header.h validates every field against the others and against the file's size): a malformed
// set is FHELIN_ERR_ARG before anything is allocated on the device, and what is read here is bounded by the file's own size
EkFile read_header(const char* path) {
    File fh(path, "rb");
    if (!fh.f) throw Error(FHELIN_ERR_ARG, std::string("evaluation-key set: cannot open ") + path);
    struct stat st;
    if (fstat(fileno(fh.f), &st) != 0) throw Error(FHELIN_ERR_ARG, "evaluation-key set: cannot stat the file");
    const uint64_t fsize = (uint64_t)st.st_size;
    std::vector<uint8_t> b((size_t)std::min<uint64_t>(KEYSET_MAX_HEADER, fsize));
    size_t have = std::fread(b.data(), 1, b.size(), fh.f);
    if (have == b.size()) {   // the rest of the prefix that these bytes announce, as far as the file goes
        b.resize((size_t)std::min<uint64_t>(std::max(keyset_prefix_bytes(b.data(), have), have), fsize));
        have += std::fread(b.data() + have, 1, b.size() - have, fh.f);
    }
    return read_keyset_header(b.data(), have, fsize);
}

// the host-only parameter context of the header: its prime chain must be the file's
void check_moduli(const EkFile& e, const std::vector<u64>& moduli) {
    if (moduli.size() != e.moduli.size() || std::memcmp(moduli.data(), e.moduli.data(), 8 * moduli.size()) != 0)
        throw Error(FHELIN_ERR_ARG, "evaluation-key set: moduli do not match the parameters");
}

// The staged stream between a file and device memory: two pinned buffers, a chunk in each, in the stream's order.
struct Pinned {
    void* p[2] = {};
    hipEvent_t ev[2] = {};
    bool used[2] = {};
    size_t pend[2] = {};   // to_file: the bytes of buffer i that its copy fills and the file has not got yet
    int cur = 0;
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
    void mark() {
        hip_check(hipEventRecord(ev[cur], s), "hipEventRecord(key staging)");
        used[cur] = true;
    }
    bool write_out(FILE* f, int i) {   // buffer i to the file, once its copy has landed
        if (!used[i]) return true;
        wait(i);
        return std::fwrite(p[i], 1, pend[i], f) == pend[i];
    }
    // device -> pinned buffer `cur` while the host writes the other buffer's previous chunk; nothing more once io_ok is false
    void to_file(FILE* f, const void* dev, size_t bytes, bool& io_ok) {
        for (size_t off = 0; off < bytes && io_ok; off += EK_STAGE_BYTES) {
            pend[cur] = std::min(EK_STAGE_BYTES, bytes - off);
            hip_check(hipMemcpyAsync(p[cur], static_cast<const char*>(dev) + off, pend[cur], hipMemcpyDeviceToHost, s), "key download");
            mark();
            cur ^= 1;
            io_ok = write_out(f, cur);
        }
    }
    void drain(FILE* f, bool& io_ok) { io_ok = io_ok && write_out(f, cur ^ 1); }   // the writer's last buffer
    // file -> pinned buffer `cur` while the other buffer's chunk is on its way to the device: a buffer is waited for when it is reused
    void from_file(FILE* f, void* dev, size_t bytes) {
        for (size_t off = 0; off < bytes; off += EK_STAGE_BYTES) {
            const size_t n = std::min(EK_STAGE_BYTES, bytes - off);
            wait(cur);
            if (std::fread(p[cur], 1, n, f) != n) throw Error(FHELIN_ERR_ARG, "evalkeys_load: truncated payload");
            hip_check(hipMemcpyAsync(static_cast<char*>(dev) + off, p[cur], n, hipMemcpyHostToDevice, s), "key upload");
            mark();
            cur ^= 1;
        }
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
    int digits = 0;   // of a switching key, capped or not
    // a run of rows that is written or read (the packed formats pack row by row): row r belongs to limb limb0 + r % limbs
    int limb0 = 0;
    int limbs = 0;
};

// a switching key on the device, capped or not
Seg key_seg(const Context& x, const EvalKey& k) {
    return k.capped() ? Seg{k.d, (size_t)k.digits * 2 * (k.max_ell + x.K) * x.N, k.max_ell, k.digits} : Seg{k.d, k.words(), 0, k.digits};
}

// The runs of one key in storage order - what a file holds of it, where that lies on the device.  halves 2: the key whole (an
// uncapped one is one run); halves 1: the b half of every digit (of the public key: its one b half).  A capped key's present rows
// ([digits][halves][max_ell + n_p][N]): per digit and half the Q rows 0 .. max_ell-1, then the special rows, where they lie in the
// full-stride layout.
std::vector<Seg> key_runs(const Context& x, uint32_t kind, const Seg& key, int halves) {
    const int rows = kind == EK_PUBLIC ? x.L + 1 : x.L + 1 + x.K;   // limbs per half on the device
    const size_t N = x.N, half = (size_t)rows * N;
    if (key.max_ell == 0 && halves == 2) return {Seg{key.d, key.words, 0, 0, 0, rows}};
    std::vector<Seg> out;
    for (int j = 0; j < (kind == EK_PUBLIC ? 1 : key.digits); ++j)
        for (int h = 0; h < halves; ++h) {
            u64* base = key.d + ((size_t)2 * j + h) * half;
            if (key.max_ell == 0) {
                out.push_back(Seg{base, half, 0, 0, 0, rows});
            } else {
                out.push_back(Seg{base, (size_t)key.max_ell * N, 0, 0, 0, key.max_ell});
                out.push_back(Seg{base + (size_t)(x.L + 1) * N, (size_t)x.K * N, 0, 0, x.L + 1, x.K});
            }
        }
    return out;
}

// per-vector digests / range flags of every key on the device (one digest run, one synchronisation), folded into one digest per key
// on the host: (digest, every residue of the key below its limb's modulus) per key
std::vector<std::pair<uint64_t, bool>> key_digests(Context& x, const std::vector<Seg>& segs, const std::vector<EkEntry>& keys) {
    const size_t N = x.N, K = (size_t)x.K;
    std::vector<std::pair<uint64_t, bool>> out(segs.size(), {0, true});
    std::vector<DigestItem> items;   // one per key, two for a capped key
    for (size_t k = 0; k < segs.size(); ++k) {
        const Seg& s = segs[k];
        const int nl = keys[k].kind == EK_PUBLIC ? x.L + 1 : x.L + 1 + x.K;
        if (s.max_ell > 0) {
            // a capped key's present rows where they lie (row-to-limb mapping of version 2: stored row r of a group is Q limb r below
            // max_ell, else special limb r - max_ell): the Q rows of all groups, then the special rows of all groups
            const size_t groups = (size_t)2 * s.digits;
            items.push_back(DigestItem{s.d, groups * s.max_ell, 0, s.max_ell, nl});
            items.push_back(DigestItem{s.d + (size_t)(x.L + 1) * N, groups * K, x.L + 1, x.K, nl});
        } else {
            items.push_back(DigestItem{s.d, s.words / N, 0, nl, nl});
        }
    }
    if (items.empty()) return out;
    DigestRun run(x, items);
    hip_check(hipStreamSynchronize(x.stream), "key digest sync");
    for (size_t k = 0, i = 0; k < segs.size(); i += segs[k].max_ell > 0 ? 2 : 1, ++k) {
        if (segs[k].max_ell > 0) {   // device order (all Q rows, all special rows) -> storage order (per group: Q rows, special rows)
            const size_t mq = (size_t)segs[k].max_ell;
            std::vector<u64> st;
            for (size_t g = 0; g < (size_t)2 * segs[k].digits; ++g) {
                st.insert(st.end(), run.pairs(i) + 2 * g * mq, run.pairs(i) + 2 * (g + 1) * mq);
                st.insert(st.end(), run.pairs(i + 1) + 2 * g * K, run.pairs(i + 1) + 2 * (g + 1) * K);
            }
            out[k].first = fold_key_digest(st.data(), st.size() / 2, out[k].second);
        } else {
            out[k].first = run.fold(i, 0, items[i].n_vec, out[k].second);
        }
    }
    return out;
}

// Packed sets: key k's rows - runs[run_begin[k], run_begin[k + 1]), one table entry per row - and its packed payload of keys[k].words
// words (keyset_key_words: the rows must add up to it), which lies in ONE scratch block as large as the largest key's, reused key
// after key in stream order.  unpack: block -> rows, else rows -> block.
struct PackPlan {
    Scratch<u64> block;
    std::vector<PackEntry> tab;   // the whole set's
    std::vector<size_t> begin;    // first entry of key k (and the end, last)
    Scratch<PackEntry> d_tab;
    bool unpack;
    PackPlan(Context& x, const std::vector<EkEntry>& keys, const std::vector<Seg>& runs, const std::vector<size_t>& run_begin, bool unpack_) : unpack(unpack_) {
        uint64_t most = 0;
        for (const EkEntry& k : keys) most = std::max(most, k.words);
        block = x.scratch<u64>((size_t)most);
        for (size_t k = 0; k < keys.size(); ++k) {
            begin.push_back(tab.size());
            size_t at = 0;
            for (size_t i = run_begin[k]; i < run_begin[k + 1]; ++i) {
                std::vector<int> width;
                limb_widths(x, runs[i].limb0, runs[i].limbs, "packed key set", &width);
                at += pack_rows(tab, x.N, runs[i].d, runs[i].words / x.N, width.data(), runs[i].limbs, block + at, unpack);
            }
            if (at != keys[k].words) throw Error(FHELIN_ERR_INTERNAL, "packed key set: the rows of a key do not add up to its table entry");
        }
        begin.push_back(tab.size());
        d_tab = upload_pack_table(x, tab);
    }
    void launch(Context& x, size_t k) const {
        (unpack ? launch_unpack_residues : launch_pack_residues)(d_tab + begin[k], (int)(begin[k + 1] - begin[k]), x.N, x.stream);
        hip_check(hipGetLastError(), unpack ? "unpack kernel" : "pack kernel");
    }
};

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

// full keys or compact (b halves and the key-set seed): the same table, digests of the full keys in both.  packed: "FHELINEP", the
// same rows in the same order at their modulus widths
void save_set(fhelin_ctx* c, const char* path, bool compact, bool packed = false) {
    Context& x = c->ctx;
    x.require_device();
    x.sync();
    const u64 g_conj = 2ull * x.N - 1;
    EkFile e;
    std::vector<Seg> segs;
    std::vector<char> seeded;
    bool any_capped = false;   // then version 2: 48-byte entries, capped keys as their present rows; else version 1, byte for byte
    auto add = [&](uint32_t kind, uint64_t g, const EvalKey* k) {   // k null: the public key
        segs.push_back(k ? key_seg(x, *k) : Seg{const_cast<u64*>(c->cl.public_key()), (size_t)2 * (x.L + 1) * x.N});
        e.keys.push_back(EkEntry{kind, (uint32_t)segs.back().digits, g, 0, 0, 0, (uint32_t)(k ? k->max_ell : x.L + 1)});
        seeded.push_back(k ? k->seeded : c->cl.public_key_seeded());
        any_capped |= k && k->capped();
    };
    if (c->cl.has_public_key()) add(EK_PUBLIC, 0, nullptr);
    if (c->ev.relin_key) add(EK_RELIN, 0, c->ev.relin_key.get());
    if (c->ev.conj_key) add(EK_CONJ, g_conj, c->ev.conj_key.get());
    if (c->ev.to_sparse_key && c->ev.from_sparse_key) {   // sparse-secret bootstrapping: both or neither; their entries carry h~ (48-byte entries)
        if (c->boot.sparse_h() < 8)   // keys put in by fhelin_key_import under a knob that is off: no reader would take the set
            throw Error(FHELIN_ERR_STATE, "evalkeys_save: the context holds the to-sparse and from-sparse keys but sparse-secret bootstrapping is off - "
                                          "set fhelin_ctx_set_bootstrap_sparse_secret to the weight they were made for");
        add(EK_TO_SPARSE, 0, c->ev.to_sparse_key.get());
        e.keys.back().reserved = (uint32_t)c->boot.sparse_h();
        add(EK_FROM_SPARSE, 0, c->ev.from_sparse_key.get());
        e.keys.back().reserved = (uint32_t)c->boot.sparse_h();
        any_capped = true;
    }
    for (const auto& kv : c->ev.rot_keys)   // ordered by Galois element; the conjugation key is stored once, above
        if (kv.second && kv.first != g_conj) add(EK_ROTATION, kv.first, kv.second.get());
    if (e.keys.empty()) throw Error(FHELIN_ERR_KEY, "evalkeys_save: the context holds no keys");
    if (e.keys.size() > EK_MAX_KEYS) throw Error(FHELIN_ERR_ARG, "evalkeys_save: too many keys");
    if (x.N % 4096) throw Error(FHELIN_ERR_ARG, "evalkeys_save: ring dimension below 2^12");
    std::vector<int> width;   // packed: of every limb, Q then P
    if (packed) limb_widths(x, 0, (int)x.moduli.size(), "packed key set", &width);
    if (compact) {
        if (!c->cl.has_key_seed())
            throw Error(FHELIN_ERR_STATE, "evalkeys_save_compact: the keys are not seeded (fhelin_ctx_set_seeded_keys before fhelin_keygen)");
        for (size_t k = 0; k < e.keys.size(); ++k)
            if (!seeded[k])
                throw Error(FHELIN_ERR_STATE, "evalkeys_save_compact: the " + key_what(e.keys[k].kind, e.keys[k].galois) +
                                                  " is not seeded (imported or made outside seeded-key mode)");
    }

    const auto digest = key_digests(x, segs, e.keys);
    for (size_t k = 0; k < e.keys.size(); ++k) {
        if (!digest[k].second) throw Error(FHELIN_ERR_INTERNAL, std::string("evalkeys_save: ") + kind_name(e.keys[k].kind) + " holds a residue out of range");
        e.keys[k].digest = digest[k].first;
    }
    // the header, and what is written of every key: the key whole, or the b half of every digit
    e.fmt = &keyset_format(packed, compact, any_capped);
    e.halves = compact ? 1 : 2;
    e.stride_word = x.stride != 1 ? (uint64_t)x.stride : 0;   // a set written at stride 1 keeps 0 here
    from_params(x.prm, e.prm);
    if (c->boot.ready()) {
        const int32_t b[7] = {c->boot.budget_enc(), c->boot.budget_dec(), c->boot.logical_slots(), c->boot.K, c->boot.R, c->boot.cheb_degree,
                              c->boot.correction};
        std::memcpy(e.boot, b, sizeof(b));
    }
    if (compact) std::memcpy(e.seed, c->cl.key_seed(), 32);
    e.moduli.assign(x.moduli.begin(), x.moduli.end());
    std::vector<Seg> out;
    std::vector<size_t> out_begin;   // first run of key k (and the end, last)
    for (size_t k = 0; k < e.keys.size(); ++k) {
        EkEntry& ek = e.keys[k];
        ek.words = keyset_key_words(*e.fmt, e.prm, ek.kind, ek.digits, ek.max_ell, e.halves, width.data());
        out_begin.push_back(out.size());
        for (const Seg& r : key_runs(x, ek.kind, segs[k], (int)e.halves)) out.push_back(r);
    }
    out_begin.push_back(out.size());
    seal_keyset(e);
    std::vector<uint8_t> h(e.data_offset);
    write_keyset_header(e, h.data());
    std::unique_ptr<PackPlan> plan;
    if (packed) plan.reset(new PackPlan(x, e.keys, out, out_begin, false));

    bool written = false;
    {
        File fh(path, "wb");
        if (!fh.f) throw Error(FHELIN_ERR_ARG, std::string("evalkeys_save: cannot create ") + path);
        bool io_ok = std::fwrite(h.data(), 1, h.size(), fh.f) == h.size();
        Pinned stg(x.stream);
        // packed: key k is packed into the scratch block (in stream order behind the downloads of key k - 1) and that block is streamed
        for (size_t k = 0; packed && k < e.keys.size(); ++k) {
            if (io_ok) plan->launch(x, k);
            stg.to_file(fh.f, plan->block, (size_t)e.keys[k].words * 8, io_ok);
        }
        for (size_t i = 0; !packed && i < out.size(); ++i) stg.to_file(fh.f, out[i].d, out[i].words * 8, io_ok);
        stg.drain(fh.f, io_ok);
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
    *stride = read_header(path).stride();
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
    if (e.stride() != x.stride) {
        if (x.stride_explicit) throw Error(FHELIN_ERR_STATE, "evalkeys_load: the set was written at interleave stride " + std::to_string(e.stride()) +
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
    for (size_t k = 0; k < e.keys.size(); ++k) {
        if (e.keys[k].kind == EK_PUBLIC) {
            const size_t pk_words = (size_t)2 * (x.L + 1) * x.N;   // the whole key (a compact entry's words count its b half)
            pk = x.scratch<u64>(pk_words);
            segs.push_back({pk, pk_words});
        } else {
            sw[k] = c->ev.new_key((int)e.keys[k].max_ell);   // a capped key: zero-filled, the payload lands in its present rows
            segs.push_back(key_seg(x, *sw[k]));
        }
    }
    // what the file holds: every key whole, or the b half of every digit (the a halves are expanded below)
    std::vector<Seg> in;
    std::vector<size_t> in_begin;   // first run of key k (and the end, last)
    std::vector<SeededEntry> tab;
    SamplerKey sk;
    for (int w = 0; w < 8; ++w) sk.w[w] = get<uint32_t>(e.seed, 4 * w);
    for (size_t k = 0; k < e.keys.size(); ++k) {
        in_begin.push_back(in.size());
        for (const Seg& r : key_runs(x, e.keys[k].kind, segs[k], (int)e.halves)) in.push_back(r);
        if (!e.compact()) continue;   // a compact set only: the a half of every digit is the expansion of the key-set seed
        const bool pub = e.keys[k].kind == EK_PUBLIC;
        const int ell = pub ? x.L + 1 : x.L + 1 + x.K;
        const size_t half = (size_t)ell * x.N;
        for (uint32_t j = 0; j < (pub ? 1 : e.keys[k].digits); ++j) {
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
    in_begin.push_back(in.size());
    // packed: what is read is key k's packed payload, into one scratch block (reused key after key in stream order), and unpacked
    // from there into the rows the unpacked formats are read into
    std::unique_ptr<PackPlan> plan;
    if (e.fmt->packed) {
        if (x.N % 4096) throw Error(FHELIN_ERR_ARG, "evalkeys_load: ring dimension below 2^12");
        std::vector<int> width;
        limb_widths(x, 0, (int)x.moduli.size(), "packed key set", &width);
        for (const auto& k : e.keys)
            if (keyset_key_words(*e.fmt, prm, k.kind, k.digits, k.max_ell, e.halves, width.data()) != k.words)
                throw Error(FHELIN_ERR_ARG, "evalkeys_load: packed key size does not match the context");
        plan.reset(new PackPlan(x, e.keys, in, in_begin, true));
    }
    {
        File fh(path, "rb");
        if (!fh.f || std::fseek(fh.f, (long)e.data_offset, SEEK_SET) != 0) throw Error(FHELIN_ERR_ARG, "evalkeys_load: cannot read the payloads");
        Pinned stg(x.stream);
        for (size_t k = 0; plan && k < e.keys.size(); ++k) {
            stg.from_file(fh.f, plan->block, (size_t)e.keys[k].words * 8);
            plan->launch(x, k);
        }
        for (size_t i = 0; !plan && i < in.size(); ++i) stg.from_file(fh.f, in[i].d, in[i].words * 8);
    }
    if (!tab.empty()) {   // every a half of the set: one launch (per 65535 key digits), before the digests see the full keys
        Scratch<SeededEntry> dt = x.scratch<SeededEntry>(tab.size());
        hip_check(hipMemcpyAsync(dt, tab.data(), tab.size() * sizeof(SeededEntry), hipMemcpyHostToDevice, x.stream), "seed table upload");
        const int max_ell = x.L + 1 + x.K;
        for (size_t lo = 0; lo < tab.size(); lo += 65535)
            launch_seeded_expand(x.dt, dt + lo, (int)std::min<size_t>(65535, tab.size() - lo), max_ell, x.stream);
        hip_check(hipGetLastError(), "seeded expand kernel");
    }
    const auto digest = key_digests(x, segs, e.keys);
    for (size_t k = 0; k < e.keys.size(); ++k) {
        const auto& ek = e.keys[k];
        const std::string what = key_what(ek.kind, ek.galois);
        if (!digest[k].second) throw Error(FHELIN_ERR_ARG, "evalkeys_load: " + what + " holds a residue not below its modulus");
        if (digest[k].first != ek.digest) throw Error(FHELIN_ERR_ARG, "evalkeys_load: " + what + " does not match its digest");
    }

    // install
    x.stride = e.stride();
    for (size_t k = 0; k < e.keys.size(); ++k) {
        if (sw[k]) {
            sw[k]->seeded = e.compact();
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
            case EK_TO_SPARSE: c->ev.to_sparse_key = sw[k]; break;
            case EK_FROM_SPARSE: c->ev.from_sparse_key = sw[k]; break;
            default: break;
        }
    }
    c->cl.install_public_key(pk.release(), e.compact());
    if (e.compact()) c->cl.install_key_seed(e.seed);
    // the client's sparse-secret knob (its keys' entries carry it), then its approximation parameters over what the knob writes
    if (e.sparse_h && e.sparse_h != c->boot.sparse_h()) c->boot.set_sparse(e.sparse_h);
    if (e.boot[2] > 0) {   // fhelin_bootstrap_setup is the caller's (fhelin_evalkeys_info)
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
