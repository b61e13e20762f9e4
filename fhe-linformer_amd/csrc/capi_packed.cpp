// extern "C" boundary, part 12: packed ciphertext blobs (include/fhelin.h "Packed formats": the stream and the blob are documented
// there).  Export range-checks, digests and packs on the device and downloads only the packed words; import uploads the packed words,
// unpacks every blob's vectors in one launch (kernels_pack.hip), then runs the range check and digest of the other loaders on the
// unpacked residues (kernels_keys.hip) and expands every seeded c1 in one launch (kernels_seeded.hip).  One synchronisation per call.
#include "../../include/fhelin.h"
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstring>
#include <map>
#include <vector>
#include "capi_internal.h"
#include "kernels_keys.h"
#include "kernels_pack.h"
#include "kernels_seeded.h"

using namespace fhelin;

namespace {

constexpr char CP_MAGIC[8] = {'F', 'H', 'E', 'L', 'I', 'N', 'C', 'P'};
constexpr uint32_t CP_VERSION = 1;
constexpr size_t CP_FIXED = 112;   // header bytes before the moduli

struct CpHeader {
    int32_t log_n = 0, ell = 0, deg = 0, slots = 0;
    double scale_hi = 0, scale_lo = 0;
    uint64_t nonce = 0, digest = 0;
    uint8_t seed[32] = {};
    int32_t stored = 0, count = 0, total = 0;
    std::vector<uint64_t> moduli;   // [ell]
    std::vector<int> width;         // [ell]
    std::vector<int> pos;           // [count]
    const uint8_t* payload = nullptr;
    size_t words_per_poly = 0;      // packed words of one component: sum_l N w_l / 64
};

size_t cp_header(int ell, int count) { return CP_FIXED + 8 * (size_t)ell + 8 * (((size_t)count + 1) / 2); }

bool all_zero(const uint8_t* b, size_t n) {
    for (size_t k = 0; k < n; ++k)
        if (b[k]) return false;
    return true;
}

// every field validated against the others and against the blob's size; nothing about a context (host-only)
CpHeader read_header(const uint8_t* b, size_t bytes) {
    if (!b) throw Error(FHELIN_ERR_ARG, "packed ciphertext: null blob");
    if (bytes < CP_FIXED) throw Error(FHELIN_ERR_ARG, "packed ciphertext: truncated header");
    if (std::memcmp(b, CP_MAGIC, 8) != 0) throw Error(FHELIN_ERR_ARG, "packed ciphertext: bad magic");
    if (get<uint32_t>(b, 8) != CP_VERSION) throw Error(FHELIN_ERR_ARG, "packed ciphertext: unsupported version");
    CpHeader h;
    h.log_n = get<int32_t>(b, 16);
    h.ell = get<int32_t>(b, 20);
    h.deg = get<int32_t>(b, 24);
    h.slots = get<int32_t>(b, 28);
    h.scale_hi = get<double>(b, 32);
    h.scale_lo = get<double>(b, 40);
    h.nonce = get<uint64_t>(b, 48);
    std::memcpy(h.seed, b + 56, 32);
    h.digest = get<uint64_t>(b, 88);
    const uint32_t stored = get<uint32_t>(b, 96), count = get<uint32_t>(b, 100), total = get<uint32_t>(b, 104);
    if (h.log_n < 12 || h.log_n > 17 || h.ell < 1 || h.ell > 64) throw Error(FHELIN_ERR_ARG, "packed ciphertext: ring dimension or limb count out of range");
    if (stored < 1 || stored > 3) throw Error(FHELIN_ERR_ARG, "packed ciphertext: stored components must be 1 (seeded), 2 or 3");
    if (count > 128 || (count > 0 && (stored != 1 || h.ell < 2 || total < count || total > 65535)) || (count == 0 && total != 0))
        throw Error(FHELIN_ERR_ARG, "packed ciphertext: bad wrapped input count or total (a wrapped input is stored seeded)");
    if (get<uint32_t>(b, 108) != 0) throw Error(FHELIN_ERR_ARG, "packed ciphertext: nonzero reserved word");
    h.stored = (int32_t)stored;
    h.count = (int32_t)count;
    h.total = (int32_t)total;
    const size_t head = cp_header(h.ell, h.count);
    if (get<uint32_t>(b, 12) != head) throw Error(FHELIN_ERR_ARG, "packed ciphertext: header size does not match the limb and input counts");
    if (bytes < head) throw Error(FHELIN_ERR_ARG, "packed ciphertext: truncated header");
    const size_t N = (size_t)1 << h.log_n;
    for (int l = 0; l < h.ell; ++l) {
        const uint64_t m = get<uint64_t>(b, CP_FIXED + 8 * (size_t)l);
        const int w = pack_width(m);
        if (w < PACK_MIN_WIDTH || w > PACK_MAX_WIDTH) throw Error(FHELIN_ERR_ARG, "packed ciphertext: a modulus outside 20..60 bits");
        h.moduli.push_back(m);
        h.width.push_back(w);
        h.words_per_poly += pack_words(N, w);
    }
    if (bytes != head + 8 * (size_t)h.stored * h.words_per_poly)
        throw Error(FHELIN_ERR_ARG, "packed ciphertext: size does not match the header (truncated?)");
    const size_t at = CP_FIXED + 8 * (size_t)h.ell;
    for (int t = 0; t < h.count; ++t) {
        const int32_t v = get<int32_t>(b, at + 4 * (size_t)t);
        if (v < 0 || v >= h.total || (t && v <= h.pos.back())) throw Error(FHELIN_ERR_ARG, "packed ciphertext: bad input positions");
        h.pos.push_back(v);
    }
    if (!all_zero(b + at + 4 * (size_t)h.count, head - at - 4 * (size_t)h.count)) throw Error(FHELIN_ERR_ARG, "packed ciphertext: nonzero padding");
    if (h.deg < 1 || h.deg > (h.stored == 1 ? 2 : 16) || h.slots < 1 || (h.slots & (h.slots - 1)) || h.slots > (1 << (h.log_n - 1)))
        throw Error(FHELIN_ERR_ARG, "packed ciphertext: bad degree or slot count");
    if (!(std::isfinite(h.scale_hi) && h.scale_hi > 0 && std::isfinite(h.scale_lo) && std::fabs(h.scale_lo) <= std::ldexp(h.scale_hi, -52)))
        throw Error(FHELIN_ERR_ARG, "packed ciphertext: bad scale");
    if (h.digest >= KEY_DIGEST_P) throw Error(FHELIN_ERR_ARG, "packed ciphertext: bad digest field");
    if (h.stored != 1 && (h.nonce != 0 || !all_zero(h.seed, 32))) throw Error(FHELIN_ERR_ARG, "packed ciphertext: a full blob carries no seed or nonce");
    h.payload = b + head;
    return h;
}

const char* const NOT_SEEDED = "packed seeded form: only an unmodified seeded (secret-key) encryption has one";

// widths of limb ids 0 .. ell-1 (Q then P) and the packed words of one component
size_t widths_of(const Context& x, int ell, std::vector<int>& width) {
    size_t words = 0;
    width.resize(ell);
    for (int l = 0; l < ell; ++l) {
        width[l] = pack_width(x.moduli[l]);
        if (width[l] < PACK_MIN_WIDTH || width[l] > PACK_MAX_WIDTH) throw Error(FHELIN_ERR_ARG, "packed formats: a modulus outside 20..60 bits");
        words += pack_words(x.N, width[l]);
    }
    return words;
}

void check_widths(const int32_t* widths, int n_vec) {
    for (int i = 0; i < n_vec; ++i)
        if (widths[i] < PACK_MIN_WIDTH || widths[i] > PACK_MAX_WIDTH) throw Error(FHELIN_ERR_ARG, "pack: width outside 20..60");
}

}  // namespace

extern "C" {

int fhelin_ct_packed_bytes(fhelin_ctx* c, const fhelin_ct* ct, int32_t seeded, size_t* bytes) {
    if (!c || !ct || !bytes) return capi_fail(FHELIN_ERR_ARG, "null argument");
    FHELIN_TRY
    if (seeded) {
        if (!ct->p || !ct->p->seeded) throw Error(FHELIN_ERR_STATE, NOT_SEEDED);
    } else {
        force(c, ct);
        if (ct->p->wrapped()) throw Error(FHELIN_ERR_ARG, "packed full form: a wrapped input has the seeded form only");
        if (ct->p->npoly < 2 || ct->p->npoly > 3) throw Error(FHELIN_ERR_ARG, "packed full form: 2 or 3 components");
    }
    std::vector<int> width;
    const size_t words = widths_of(c->ctx, ct->p->ell, width);
    *bytes = cp_header(ct->p->ell, (int)ct->p->wrap_pos.size()) + 8 * (size_t)(seeded ? 1 : ct->p->npoly) * words;
    FHELIN_CATCH
}

int fhelin_ct_export_packed(fhelin_ctx* c, const fhelin_ct* ct, int32_t seeded, uint8_t* out, size_t cap) {
    if (!c || !ct || !out) return capi_fail(FHELIN_ERR_ARG, "null argument");
    FHELIN_TRY
    if (seeded && (!ct->p || !ct->p->seeded)) throw Error(FHELIN_ERR_STATE, NOT_SEEDED);
    const bool wrapped = seeded && ct->p->wrapped();   // a wrapped input is not a value of the pass (no level-plan terminal)
    if (!wrapped && c->plan.live(ct->node, ct->node_epoch)) c->plan.terminal(ct->node, 2);
    const CtPtr& p = wrapped ? ct->p : ct_in(c, ct);   // a wrapped handle with seeded = 0: FHELIN_ERR_ARG from ct_in
    if (!wrapped) c->plan.check_terminal(*p, 2);
    Context& x = c->ctx;
    x.require_device();
    if (x.N % 4096) throw Error(FHELIN_ERR_ARG, "export_packed: ring dimension below 2^12");
    if (!seeded && (p->npoly < 2 || p->npoly > 3)) throw Error(FHELIN_ERR_ARG, "export_packed: 2 or 3 components");
    const int ell = p->ell, count = wrapped ? (int)p->wrap_pos.size() : 0, stored = seeded ? 1 : p->npoly, n_vec = stored * ell;
    std::vector<int> width;
    const size_t N = x.N, words = widths_of(x, ell, width), head = cp_header(ell, count);
    if (cap < head + 8 * (size_t)stored * words) throw Error(FHELIN_ERR_ARG, "export_packed: buffer too small");
    // range check + digest of the unpacked residues and the pack, one after the other on the stream; only packed words come back
    Scratch<u64> part = x.scratch<u64>(key_digest_scratch_words(x.N, n_vec));
    Scratch<u64> dg = x.scratch<u64>(2 * (size_t)n_vec);
    Scratch<u64> packed = x.scratch<u64>((size_t)stored * words);
    Scratch<PackEntry> d_tab = x.scratch<PackEntry>((size_t)n_vec);
    std::vector<PackEntry> tab(n_vec);
    size_t at = 0;
    for (int v = 0; v < n_vec; ++v) {
        tab[v] = PackEntry{p->d + (size_t)v * N, packed + at, (u32)width[v % ell], 0};
        at += pack_words(N, width[v % ell]);
    }
    hip_check(hipMemcpyAsync(d_tab, tab.data(), tab.size() * sizeof(PackEntry), hipMemcpyHostToDevice, x.stream), "pack table upload");
    launch_key_digest(x.dt, p->d, n_vec, 0, ell, part, dg, x.stream);
    launch_pack_residues(d_tab, n_vec, x.N, x.stream);
    hip_check(hipGetLastError(), "packed export kernels");
    std::vector<u64> h(2 * (size_t)n_vec);
    hip_check(hipMemcpyAsync(h.data(), dg, h.size() * 8, hipMemcpyDeviceToHost, x.stream), "packed digest download");
    hip_check(hipMemcpyAsync(out + head, packed, (size_t)stored * words * 8, hipMemcpyDeviceToHost, x.stream), "packed export");
    hip_check(hipStreamSynchronize(x.stream), "packed export sync");
    bool in_range;
    const u64 digest = fold_key_digest(h.data(), (size_t)n_vec, in_range);
    if (!in_range) throw Error(FHELIN_ERR_INTERNAL, "export_packed: the ciphertext holds a residue out of range");
    std::memset(out, 0, head);
    std::memcpy(out, CP_MAGIC, 8);
    put<uint32_t>(out, 8, CP_VERSION);
    put<uint32_t>(out, 12, (uint32_t)head);
    const int32_t shape[4] = {x.prm.log_n, ell, p->deg, p->slots};
    std::memcpy(out + 16, shape, sizeof(shape));
    const double hi = (double)p->scale, lo = (double)(p->scale - (long double)hi);   // as fhelin_ct_scale
    put<double>(out, 32, hi);
    put<double>(out, 40, lo);
    if (seeded) {
        put<uint64_t>(out, 48, p->nonce);
        std::memcpy(out + 56, p->seed, 32);
    }
    put<uint64_t>(out, 88, digest);
    put<uint32_t>(out, 96, (uint32_t)stored);
    put<uint32_t>(out, 100, (uint32_t)count);
    put<uint32_t>(out, 104, (uint32_t)(wrapped ? p->wrap_total : 0));
    std::memcpy(out + CP_FIXED, x.moduli.data(), 8 * (size_t)ell);   // the first ell moduli of Q then P
    for (int t = 0; t < count; ++t) put<int32_t>(out, CP_FIXED + 8 * (size_t)ell + 4 * (size_t)t, p->wrap_pos[t]);
    FHELIN_CATCH
}

int fhelin_packed_info(const uint8_t* blob, size_t bytes, int32_t* log_n, int32_t* ell, int32_t* deg, int32_t* slots, int32_t* stored,
                       int32_t* count) {
    FHELIN_TRY
    const CpHeader h = read_header(blob, bytes);
    if (log_n) *log_n = h.log_n;
    if (ell) *ell = h.ell;
    if (deg) *deg = h.deg;
    if (slots) *slots = h.slots;
    if (stored) *stored = h.stored;
    if (count) *count = h.count;
    FHELIN_CATCH
}

int fhelin_ct_import_packed(fhelin_ctx* c, const uint8_t* const* blobs, const size_t* sizes, int32_t n, fhelin_ct** outs) {
    if (!c || (n > 0 && (!blobs || !sizes || !outs)) || n < 0) return capi_fail(FHELIN_ERR_ARG, "null argument");
    FHELIN_TRY
    Context& x = c->ctx;
    x.require_device();
    if (n == 0) return FHELIN_OK;
    if (n > 65535) throw Error(FHELIN_ERR_ARG, "import_packed: at most 65535 blobs per call");
    if (x.N % 4096) throw Error(FHELIN_ERR_ARG, "import_packed: ring dimension below 2^12");
    const size_t N = x.N;
    // 1. every header, against the blob and against this context, before anything is allocated
    std::vector<CpHeader> hs(n);
    size_t total_words = 0, total_vec = 0;
    for (int i = 0; i < n; ++i) {
        hs[i] = read_header(blobs[i], sizes[i]);
        const CpHeader& h = hs[i];
        const std::string at = "import_packed: blob " + std::to_string(i) + ": ";
        if (h.log_n != x.prm.log_n) throw Error(FHELIN_ERR_ARG, at + "made for another ring dimension");
        // wrapped: ell <= n_q + 1, the first ell moduli of Q then P (the extra limb of an input at n_q limbs is p_0)
        if (h.ell > x.L + 1 + (h.count > 0 && x.K > 0 ? 1 : 0)) throw Error(FHELIN_ERR_ARG, at + "more limbs than the context's chain");
        if (std::memcmp(h.moduli.data(), x.moduli.data(), 8 * (size_t)h.ell) != 0) throw Error(FHELIN_ERR_ARG, at + "moduli do not match the context");
        total_words += (size_t)h.stored * h.words_per_poly;
        total_vec += (size_t)h.stored * h.ell;
    }
    // 2. one batch allocation per (stored components, limb count); every packed payload uploaded into one scratch block
    std::map<std::pair<int, int>, std::vector<int>> groups;
    for (int i = 0; i < n; ++i) groups[{hs[i].stored, hs[i].ell}].push_back(i);
    std::vector<CtPtr> cts(n);
    int max_ell = 0;
    size_t max_vec = 0;   // most vectors one digest launch covers
    for (auto& g : groups) {
        const int stored = g.first.first, ell = g.first.second;
        std::vector<CtPtr> b = c->ev.new_ct_batch((int)g.second.size(), std::max(2, stored), ell, 1, 1.0L, 1);
        for (size_t k = 0; k < g.second.size(); ++k) cts[g.second[k]] = b[k];
        max_ell = std::max(max_ell, ell);
        max_vec = std::max(max_vec, g.second.size() * (size_t)stored * ell);
    }
    if (max_vec > 65535) throw Error(FHELIN_ERR_ARG, "import_packed: too many limbs of one level in one call");
    Scratch<u64> packed = x.scratch<u64>(total_words);
    std::vector<PackEntry> ptab;
    std::vector<SeededEntry> stab;
    ptab.reserve(total_vec);
    size_t at = 0;
    for (int i = 0; i < n; ++i) {
        const CpHeader& h = hs[i];
        Ciphertext& ct = *cts[i];
        ct.deg = h.deg;
        ct.slots = h.slots;
        ct.scale = (long double)h.scale_hi + (long double)h.scale_lo;
        if (h.count > 0) {
            ct.wrap_pos = h.pos;
            ct.wrap_total = h.total;
        }
        hip_check(hipMemcpyAsync(packed + at, h.payload, (size_t)h.stored * h.words_per_poly * 8, hipMemcpyHostToDevice, x.stream), "packed upload");
        for (int v = 0; v < h.stored * h.ell; ++v) {
            ptab.push_back(PackEntry{packed + at, ct.d + (size_t)v * N, (u32)h.width[v % h.ell], 0});
            at += pack_words(N, h.width[v % h.ell]);
        }
        if (h.stored == 1) {
            SeededEntry e;
            for (int w = 0; w < 8; ++w) e.key.w[w] = get<uint32_t>(h.seed, 4 * w);
            e.nonce = h.nonce;
            e.dst = ct.d + (size_t)h.ell * N;
            e.ell = h.ell;
            stab.push_back(e);
        }
    }
    // 3. unpack everything in one launch; range check + digest of the unpacked residues (one launch pair per group: the stored
    // vectors of a seeded blob are ell apart in groups of 2 ell); every seeded c1 in one launch; one synchronisation for the call
    Scratch<PackEntry> d_ptab = x.scratch<PackEntry>(ptab.size());
    hip_check(hipMemcpyAsync(d_ptab, ptab.data(), ptab.size() * sizeof(PackEntry), hipMemcpyHostToDevice, x.stream), "unpack table upload");
    launch_unpack_residues(d_ptab, (int)ptab.size(), x.N, x.stream);
    Scratch<u64> part = x.scratch<u64>(key_digest_scratch_words(x.N, (int)max_vec));
    Scratch<u64> dg = x.scratch<u64>(2 * total_vec);
    std::vector<size_t> dg_at(n);   // first digest vector of blob i
    size_t v0 = 0;
    for (auto& g : groups) {
        const int stored = g.first.first, ell = g.first.second, cnt = (int)g.second.size(), per = stored * ell;
        launch_key_digest_strided(x.dt, cts[g.second[0]]->d, cnt * per, 0, ell, stored == 1 ? 2 * ell : ell, part, dg + 2 * v0, x.stream);
        for (int k = 0; k < cnt; ++k) dg_at[g.second[k]] = v0 + (size_t)k * per;
        v0 += (size_t)cnt * per;
    }
    Scratch<SeededEntry> d_stab;
    if (!stab.empty()) {
        d_stab = x.scratch<SeededEntry>(stab.size());
        hip_check(hipMemcpyAsync(d_stab, stab.data(), stab.size() * sizeof(SeededEntry), hipMemcpyHostToDevice, x.stream), "seed table upload");
        launch_seeded_expand(x.dt, d_stab, (int)stab.size(), max_ell, x.stream);
    }
    hip_check(hipGetLastError(), "packed import kernels");
    std::vector<u64> h(2 * v0);
    hip_check(hipMemcpyAsync(h.data(), dg, h.size() * 8, hipMemcpyDeviceToHost, x.stream), "packed digest download");
    hip_check(hipStreamSynchronize(x.stream), "packed import sync");
    // 4. all or nothing: a handle only when every blob passed
    for (int i = 0; i < n; ++i) {
        bool in_range;
        const u64 digest = fold_key_digest(&h[2 * dg_at[i]], (size_t)hs[i].stored * hs[i].ell, in_range);
        if (!in_range) throw Error(FHELIN_ERR_ARG, "import_packed: blob " + std::to_string(i) + " holds a residue not below its modulus (range check)");
        if (digest != hs[i].digest) throw Error(FHELIN_ERR_ARG, "import_packed: blob " + std::to_string(i) + " does not match its digest");
    }
    for (int i = 0; i < n; ++i) outs[i] = wrap(c, cts[i]);   // imported: not a level-plan source, never lowered
    FHELIN_CATCH
}

int fhelin_debug_pack(fhelin_ctx* c, const uint64_t* words, const int32_t* widths, int32_t n_vec, uint64_t* out, size_t cap_words,
                      size_t* n_words) {
    if (!c || !words || !widths || !out || !n_words || n_vec < 1) return capi_fail(FHELIN_ERR_ARG, "null argument");
    FHELIN_TRY
    Context& x = c->ctx;
    x.require_device();
    if (x.N % 4096) throw Error(FHELIN_ERR_ARG, "debug_pack: ring dimension below 2^12");
    check_widths(widths, n_vec);
    const size_t N = x.N;
    size_t total = 0;
    for (int i = 0; i < n_vec; ++i) {
        total += pack_words(N, widths[i]);
        for (size_t j = 0; j < N; ++j)
            if (words[(size_t)i * N + j] >> widths[i]) throw Error(FHELIN_ERR_ARG, "debug_pack: a value at or above 2^w");
    }
    if (cap_words < total) throw Error(FHELIN_ERR_ARG, "debug_pack: buffer too small");
    Scratch<u64> src = x.scratch<u64>((size_t)n_vec * N);
    Scratch<u64> dst = x.scratch<u64>(total);
    Scratch<PackEntry> d_tab = x.scratch<PackEntry>((size_t)n_vec);
    std::vector<PackEntry> tab(n_vec);
    size_t at = 0;
    for (int i = 0; i < n_vec; ++i) {
        tab[i] = PackEntry{src + (size_t)i * N, dst + at, (u32)widths[i], 0};
        at += pack_words(N, widths[i]);
    }
    hip_check(hipMemcpyAsync(src, words, (size_t)n_vec * N * 8, hipMemcpyHostToDevice, x.stream), "debug_pack upload");
    hip_check(hipMemcpyAsync(d_tab, tab.data(), tab.size() * sizeof(PackEntry), hipMemcpyHostToDevice, x.stream), "pack table upload");
    launch_pack_residues(d_tab, n_vec, x.N, x.stream);
    hip_check(hipGetLastError(), "pack kernel");
    hip_check(hipMemcpyAsync(out, dst, total * 8, hipMemcpyDeviceToHost, x.stream), "debug_pack download");
    hip_check(hipStreamSynchronize(x.stream), "debug_pack sync");
    *n_words = total;
    FHELIN_CATCH
}

int fhelin_debug_unpack(fhelin_ctx* c, const uint64_t* packed, size_t n_words, const int32_t* widths, int32_t n_vec, uint64_t* out) {
    if (!c || !packed || !widths || !out || n_vec < 1) return capi_fail(FHELIN_ERR_ARG, "null argument");
    FHELIN_TRY
    Context& x = c->ctx;
    x.require_device();
    if (x.N % 4096) throw Error(FHELIN_ERR_ARG, "debug_unpack: ring dimension below 2^12");
    check_widths(widths, n_vec);
    const size_t N = x.N;
    size_t total = 0;
    for (int i = 0; i < n_vec; ++i) total += pack_words(N, widths[i]);
    if (n_words != total) throw Error(FHELIN_ERR_ARG, "debug_unpack: the word count does not match the widths");
    Scratch<u64> src = x.scratch<u64>(total);
    Scratch<u64> dst = x.scratch<u64>((size_t)n_vec * N);
    Scratch<PackEntry> d_tab = x.scratch<PackEntry>((size_t)n_vec);
    std::vector<PackEntry> tab(n_vec);
    size_t at = 0;
    for (int i = 0; i < n_vec; ++i) {
        tab[i] = PackEntry{src + at, dst + (size_t)i * N, (u32)widths[i], 0};
        at += pack_words(N, widths[i]);
    }
    hip_check(hipMemcpyAsync(src, packed, total * 8, hipMemcpyHostToDevice, x.stream), "debug_unpack upload");
    hip_check(hipMemcpyAsync(d_tab, tab.data(), tab.size() * sizeof(PackEntry), hipMemcpyHostToDevice, x.stream), "unpack table upload");
    launch_unpack_residues(d_tab, n_vec, x.N, x.stream);
    hip_check(hipGetLastError(), "unpack kernel");
    hip_check(hipMemcpyAsync(out, dst, (size_t)n_vec * N * 8, hipMemcpyDeviceToHost, x.stream), "debug_unpack download");
    hip_check(hipStreamSynchronize(x.stream), "debug_unpack sync");
    FHELIN_CATCH
}

int fhelin_debug_pack_rate(fhelin_ctx* c, const int32_t* widths, int32_t n_vec, int32_t reps, float* ms) {
    if (!c || !widths || !ms || n_vec < 1 || reps < 1) return capi_fail(FHELIN_ERR_ARG, "null argument");
    FHELIN_TRY
    Context& x = c->ctx;
    x.require_device();
    if (x.N % 4096) throw Error(FHELIN_ERR_ARG, "debug_pack_rate: ring dimension below 2^12");
    check_widths(widths, n_vec);
    const size_t N = x.N, words = (size_t)n_vec * N;
    size_t total = 0;
    for (int i = 0; i < n_vec; ++i) total += pack_words(N, widths[i]);
    Scratch<u64> a = x.scratch<u64>(words);
    Scratch<u64> b = x.scratch<u64>(words);
    Scratch<u64> pk = x.scratch<u64>(total);
    Scratch<PackEntry> d_tab = x.scratch<PackEntry>((size_t)2 * n_vec);
    std::vector<PackEntry> tab(2 * (size_t)n_vec);
    size_t at = 0;
    for (int i = 0; i < n_vec; ++i) {
        tab[i] = PackEntry{a + (size_t)i * N, pk + at, (u32)widths[i], 0};
        tab[n_vec + i] = PackEntry{pk + at, b + (size_t)i * N, (u32)widths[i], 0};
        at += pack_words(N, widths[i]);
    }
    hip_check(hipMemcpyAsync(d_tab, tab.data(), tab.size() * sizeof(PackEntry), hipMemcpyHostToDevice, x.stream), "pack table upload");
    hip_check(hipMemsetAsync(a, 0x15, words * 8, x.stream), "debug_pack_rate fill");
    struct Events {   // destroyed on every way out
        std::vector<hipEvent_t> v;
        explicit Events(size_t n) : v(n, nullptr) {}
        ~Events() {
            for (hipEvent_t e : v)
                if (e) (void)hipEventDestroy(e);
        }
    } events(4 * (size_t)reps + 1);
    std::vector<hipEvent_t>& ev = events.v;
    for (auto& e : ev) hip_check(hipEventCreate(&e), "hipEventCreate");
    // one untimed round, then pack, copy, unpack, copy in turn: the copy moves the same unpacked bytes device to device
    for (int r = -1; r < reps; ++r) {
        const bool timed = r >= 0;
        if (r == 0) hip_check(hipEventRecord(ev[0], x.stream), "hipEventRecord");
        launch_pack_residues(d_tab, n_vec, x.N, x.stream);
        if (timed) hip_check(hipEventRecord(ev[4 * r + 1], x.stream), "hipEventRecord");
        hip_check(hipMemcpyAsync(b, a, words * 8, hipMemcpyDeviceToDevice, x.stream), "debug_pack_rate copy");
        if (timed) hip_check(hipEventRecord(ev[4 * r + 2], x.stream), "hipEventRecord");
        launch_unpack_residues(d_tab + n_vec, n_vec, x.N, x.stream);
        if (timed) hip_check(hipEventRecord(ev[4 * r + 3], x.stream), "hipEventRecord");
        hip_check(hipMemcpyAsync(a, b, words * 8, hipMemcpyDeviceToDevice, x.stream), "debug_pack_rate copy");
        if (timed) hip_check(hipEventRecord(ev[4 * r + 4], x.stream), "hipEventRecord");
    }
    hip_check(hipGetLastError(), "pack kernels");
    hip_check(hipStreamSynchronize(x.stream), "debug_pack_rate sync");
    for (int k = 0; k < 4 * reps; ++k) hip_check(hipEventElapsedTime(&ms[k], ev[k], ev[k + 1]), "hipEventElapsedTime");
    FHELIN_CATCH
}

}  // extern "C"
