// extern "C" boundary, part 5: seeded secret-key encryption and compact ciphertexts (include/fhelin.h "Compact ciphertexts": the
// expansion and the blob format are documented there).  A seeded encryption's c1 is the expansion of a public (seed, nonce), so a
// compact blob carries c0 alone; import uploads every c0, range-checks and digests them on the device (kernels_keys.hip) and
// expands every c1 in one launch (kernels_seeded.hip), with one host synchronisation per call.
#include "../../include/fhelin.h"
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstring>
#include <map>
#include <vector>
#include "capi_internal.h"
#include "kernels_keys.h"
#include "kernels_seeded.h"

using namespace fhelin;

namespace {

constexpr char CC_MAGIC[8] = {'F', 'H', 'E', 'L', 'I', 'N', 'C', 'C'};
constexpr uint32_t CC_VERSION = 1;
constexpr uint32_t CC_VERSION_WRAPPED = 2;   // a wrapped input (include/fhelin.h "Wrapped inputs")
constexpr size_t CC_FIXED = 96;   // header bytes before the moduli (version 1)
constexpr size_t CC_FIXED_WRAPPED = 104;     // version 2: + count, total

struct CcHeader {
    int32_t log_n = 0, ell = 0, deg = 0, slots = 0;
    double scale_hi = 0, scale_lo = 0;
    uint64_t nonce = 0, digest = 0;
    uint8_t seed[32] = {};
    const uint64_t* moduli = nullptr;   // [ell], inside the blob (may be unaligned: read with memcpy)
    const uint8_t* c0 = nullptr;        // [ell][N] u64, inside the blob
    uint32_t version = 1;
    int32_t count = 0, total = 0;       // version 2
    std::vector<int> pos;               // version 2: the inputs' positions, [count]
};

size_t cc_bytes(int log_n, int ell) { return CC_FIXED + 8 * (size_t)ell + 8 * (size_t)ell * ((size_t)1 << log_n); }
size_t cc_header_wrapped(int ell, int count) { return CC_FIXED_WRAPPED + 8 * (size_t)ell + 8 * (((size_t)count + 1) / 2); }
size_t cc_bytes_wrapped(int log_n, int ell, int count) { return cc_header_wrapped(ell, count) + 8 * (size_t)ell * ((size_t)1 << log_n); }

// every field validated against the others and against the blob's size; nothing about a context (host-only)
CcHeader read_header(const uint8_t* b, size_t bytes) {
    if (!b) throw Error(FHELIN_ERR_ARG, "compact ciphertext: null blob");
    if (bytes < CC_FIXED) throw Error(FHELIN_ERR_ARG, "compact ciphertext: truncated header");
    if (std::memcmp(b, CC_MAGIC, 8) != 0) throw Error(FHELIN_ERR_ARG, "compact ciphertext: bad magic");
    const uint32_t version = get<uint32_t>(b, 8);
    if (version != CC_VERSION && version != CC_VERSION_WRAPPED) throw Error(FHELIN_ERR_ARG, "compact ciphertext: unsupported version");
    if (version == CC_VERSION_WRAPPED && bytes < CC_FIXED_WRAPPED) throw Error(FHELIN_ERR_ARG, "compact ciphertext: truncated header");
    CcHeader h;
    h.version = version;
    h.log_n = get<int32_t>(b, 16);
    h.ell = get<int32_t>(b, 20);
    h.deg = get<int32_t>(b, 24);
    h.slots = get<int32_t>(b, 28);
    h.scale_hi = get<double>(b, 32);
    h.scale_lo = get<double>(b, 40);
    h.nonce = get<uint64_t>(b, 48);
    std::memcpy(h.seed, b + 56, 32);
    h.digest = get<uint64_t>(b, 88);
    if (h.log_n < 12 || h.log_n > 17 || h.ell < 1 || h.ell > 64) throw Error(FHELIN_ERR_ARG, "compact ciphertext: ring dimension or limb count out of range");
    size_t head = CC_FIXED + 8 * (size_t)h.ell;
    if (version == CC_VERSION_WRAPPED) {
        h.count = get<int32_t>(b, 96);
        h.total = get<int32_t>(b, 100);
        if (h.ell < 2 || h.count < 1 || h.count > 128 || h.total < h.count || h.total > 65535)
            throw Error(FHELIN_ERR_ARG, "compact ciphertext: bad wrapped limb count, input count or total");
        head = cc_header_wrapped(h.ell, h.count);
    }
    if (get<uint32_t>(b, 12) != head) throw Error(FHELIN_ERR_ARG, "compact ciphertext: header size does not match the limb count");
    if (bytes != (version == CC_VERSION ? cc_bytes(h.log_n, h.ell) : cc_bytes_wrapped(h.log_n, h.ell, h.count)))
        throw Error(FHELIN_ERR_ARG, "compact ciphertext: size does not match the header (truncated?)");
    if (version == CC_VERSION_WRAPPED) {
        const size_t at = CC_FIXED_WRAPPED + 8 * (size_t)h.ell;
        for (int t = 0; t < h.count; ++t) {
            const int32_t v = get<int32_t>(b, at + 4 * (size_t)t);
            if (v < 0 || v >= h.total || (t && v <= h.pos.back())) throw Error(FHELIN_ERR_ARG, "compact ciphertext: bad input positions");
            h.pos.push_back(v);
        }
        for (size_t k = at + 4 * (size_t)h.count; k < head; ++k)
            if (b[k]) throw Error(FHELIN_ERR_ARG, "compact ciphertext: nonzero padding");
    }
    if (h.deg < 1 || h.deg > 2 || h.slots < 1 || (h.slots & (h.slots - 1)) || h.slots > (1 << (h.log_n - 1)))
        throw Error(FHELIN_ERR_ARG, "compact ciphertext: bad degree or slot count");
    if (!(std::isfinite(h.scale_hi) && h.scale_hi > 0 && std::isfinite(h.scale_lo) && std::fabs(h.scale_lo) <= std::ldexp(h.scale_hi, -52)))
        throw Error(FHELIN_ERR_ARG, "compact ciphertext: bad scale");
    if (h.digest >= KEY_DIGEST_P) throw Error(FHELIN_ERR_ARG, "compact ciphertext: bad digest field");
    h.moduli = reinterpret_cast<const uint64_t*>(b + (version == CC_VERSION ? CC_FIXED : CC_FIXED_WRAPPED));
    h.c0 = b + head;
    return h;
}

}  // namespace

extern "C" {

int fhelin_ctx_set_seeded_encryption(fhelin_ctx* c, int32_t on) {
    if (!c) return capi_fail(FHELIN_ERR_ARG, "null argument");
    FHELIN_TRY
    c->cl.set_seeded(on != 0);
    FHELIN_CATCH
}

int fhelin_ct_compact_bytes(const fhelin_ct* ct, size_t* bytes) {
    if (!ct || !bytes) return capi_fail(FHELIN_ERR_ARG, "null argument");
    // a deferred handle is an operation's result: never a seeded encryption
    if (!ct->p || !ct->p->seeded) return capi_fail(FHELIN_ERR_STATE, "compact form: only an unmodified seeded (secret-key) encryption has one");
    *bytes = ct->p->wrapped() ? cc_bytes_wrapped(ct->p->ctx->prm.log_n, ct->p->ell, (int)ct->p->wrap_pos.size())
                              : cc_bytes(ct->p->ctx->prm.log_n, ct->p->ell);
    return FHELIN_OK;
}

int fhelin_ct_export_compact(fhelin_ctx* c, const fhelin_ct* ct, uint8_t* out, size_t cap) {
    if (!c || !ct || !out) return capi_fail(FHELIN_ERR_ARG, "null argument");
    FHELIN_TRY
    if (!ct->p || !ct->p->seeded) throw Error(FHELIN_ERR_STATE, "compact form: only an unmodified seeded (secret-key) encryption has one");
    const bool wrapped = ct->p->wrapped();   // version 2; a wrapped input is not a value of the pass (no level-plan terminal)
    if (!wrapped && c->plan.live(ct->node, ct->node_epoch)) c->plan.terminal(ct->node, 2);
    const CtPtr& p = wrapped ? ct->p : ct_in(c, ct);
    if (!wrapped) c->plan.check_terminal(*p, 2);
    Context& x = c->ctx;
    const int ell = p->ell, count = (int)p->wrap_pos.size();
    const size_t N = x.N, bytes = wrapped ? cc_bytes_wrapped(x.prm.log_n, ell, count) : cc_bytes(x.prm.log_n, ell);
    const size_t head = wrapped ? cc_header_wrapped(ell, count) : CC_FIXED + 8 * (size_t)ell;
    if (cap < bytes) throw Error(FHELIN_ERR_ARG, "export_compact: buffer too small");
    if (x.N % 4096) throw Error(FHELIN_ERR_ARG, "export_compact: ring dimension below 2^12");
    // c0's digest on the device, c0 itself straight into the blob; one synchronisation
    Scratch<u64> part = x.scratch<u64>(key_digest_scratch_words(x.N, ell));
    Scratch<u64> dg = x.scratch<u64>(2 * (size_t)ell);
    launch_key_digest(x.dt, p->d, ell, 0, ell, part, dg, x.stream);
    hip_check(hipGetLastError(), "compact digest kernels");
    std::vector<u64> h(2 * (size_t)ell);
    hip_check(hipMemcpyAsync(h.data(), dg, h.size() * 8, hipMemcpyDeviceToHost, x.stream), "compact digest download");
    hip_check(hipMemcpyAsync(out + head, p->d, (size_t)ell * N * 8, hipMemcpyDeviceToHost, x.stream), "compact export");
    hip_check(hipStreamSynchronize(x.stream), "compact export sync");
    part.reset();
    dg.reset();
    bool in_range;
    const u64 digest = fold_key_digest(h.data(), (size_t)ell, in_range);
    if (!in_range) throw Error(FHELIN_ERR_INTERNAL, "export_compact: c0 holds a residue out of range");
    std::memcpy(out, CC_MAGIC, 8);
    put<uint32_t>(out, 8, wrapped ? CC_VERSION_WRAPPED : CC_VERSION);
    put<uint32_t>(out, 12, (uint32_t)head);
    const int32_t shape[4] = {x.prm.log_n, ell, p->deg, p->slots};
    std::memcpy(out + 16, shape, sizeof(shape));
    const double hi = (double)p->scale, lo = (double)(p->scale - (long double)hi);   // as fhelin_ct_scale
    put<double>(out, 32, hi);
    put<double>(out, 40, lo);
    put<uint64_t>(out, 48, p->nonce);
    std::memcpy(out + 56, p->seed, 32);
    put<uint64_t>(out, 88, digest);
    if (!wrapped) {
        std::memcpy(out + CC_FIXED, x.chain.q.data(), 8 * (size_t)ell);
    } else {
        put<int32_t>(out, 96, count);
        put<int32_t>(out, 100, p->wrap_total);
        std::memcpy(out + CC_FIXED_WRAPPED, x.moduli.data(), 8 * (size_t)ell);   // the first ell moduli of Q then P
        const size_t at = CC_FIXED_WRAPPED + 8 * (size_t)ell;
        std::memset(out + at, 0, head - at);
        for (int t = 0; t < count; ++t) put<int32_t>(out, at + 4 * (size_t)t, p->wrap_pos[t]);
    }
    FHELIN_CATCH
}

int fhelin_compact_info(const uint8_t* blob, size_t bytes, int32_t* log_n, int32_t* ell, int32_t* deg, int32_t* slots) {
    FHELIN_TRY
    const CcHeader h = read_header(blob, bytes);
    if (log_n) *log_n = h.log_n;
    if (ell) *ell = h.ell;
    if (deg) *deg = h.deg;
    if (slots) *slots = h.slots;
    FHELIN_CATCH
}

int fhelin_ct_import_compact(fhelin_ctx* c, const uint8_t* const* blobs, const size_t* sizes, int32_t n, fhelin_ct** outs) {
    if (!c || (n > 0 && (!blobs || !sizes || !outs)) || n < 0) return capi_fail(FHELIN_ERR_ARG, "null argument");
    FHELIN_TRY
    Context& x = c->ctx;
    x.require_device();
    if (n == 0) return FHELIN_OK;
    if (n > 65535) throw Error(FHELIN_ERR_ARG, "import_compact: at most 65535 blobs per call");
    if (x.N % 4096) throw Error(FHELIN_ERR_ARG, "import_compact: ring dimension below 2^12");
    const size_t N = x.N;
    // 1. every header, against the blob and against this context, before anything is allocated
    std::vector<CcHeader> hs(n);
    for (int i = 0; i < n; ++i) {
        hs[i] = read_header(blobs[i], sizes[i]);
        const CcHeader& h = hs[i];
        const std::string at = "import_compact: blob " + std::to_string(i) + ": ";
        if (h.log_n != x.prm.log_n) throw Error(FHELIN_ERR_ARG, at + "made for another ring dimension");
        // version 2 (wrapped): ell <= n_q + 1, the first ell moduli of Q then P (the extra limb of an input at n_q limbs is p_0)
        if (h.ell > x.L + 1 + (h.version == CC_VERSION_WRAPPED && x.K > 0 ? 1 : 0)) throw Error(FHELIN_ERR_ARG, at + "more limbs than the context's chain");
        if (std::memcmp(h.moduli, x.moduli.data(), 8 * (size_t)h.ell) != 0) throw Error(FHELIN_ERR_ARG, at + "moduli do not match the context");
    }
    // 2. one batch allocation per limb count; c0 of every blob uploaded into its ciphertext
    std::map<int, std::vector<int>> groups;
    for (int i = 0; i < n; ++i) groups[hs[i].ell].push_back(i);
    std::vector<CtPtr> cts(n);
    int max_ell = 0, max_vec = 0;
    for (auto& g : groups) {
        const int ell = g.first;
        std::vector<CtPtr> b = c->ev.new_ct_batch((int)g.second.size(), 2, ell, 1, 1.0L, 1);
        for (size_t k = 0; k < g.second.size(); ++k) cts[g.second[k]] = b[k];
        max_ell = std::max(max_ell, ell);
        max_vec = std::max(max_vec, (int)g.second.size() * ell);
    }
    if (max_vec > 65535) throw Error(FHELIN_ERR_ARG, "import_compact: too many limbs of one level in one call");
    std::vector<SeededEntry> tab(n);
    for (int i = 0; i < n; ++i) {
        const CcHeader& h = hs[i];
        Ciphertext& ct = *cts[i];
        ct.deg = h.deg;
        ct.slots = h.slots;
        ct.scale = (long double)h.scale_hi + (long double)h.scale_lo;
        if (h.version == CC_VERSION_WRAPPED) {
            ct.wrap_pos = h.pos;
            ct.wrap_total = h.total;
        }
        hip_check(hipMemcpyAsync(ct.d, h.c0, (size_t)h.ell * N * 8, hipMemcpyHostToDevice, x.stream), "compact upload");
        for (int w = 0; w < 8; ++w) tab[i].key.w[w] = get<uint32_t>(h.seed, 4 * w);
        tab[i].nonce = h.nonce;
        tab[i].dst = ct.d + (size_t)h.ell * N;
        tab[i].ell = h.ell;
    }
    // 3. range check + digest of every c0 (one launch pair per limb count: c0 vectors ell apart in groups of 2 ell), then every c1
    // in one launch; one synchronisation for the call
    Scratch<u64> part = x.scratch<u64>(key_digest_scratch_words(x.N, max_vec));
    Scratch<u64> dg = x.scratch<u64>(2 * (size_t)n * max_ell);
    Scratch<SeededEntry> d_tab = x.scratch<SeededEntry>((size_t)n);
    hip_check(hipMemcpyAsync(d_tab, tab.data(), (size_t)n * sizeof(SeededEntry), hipMemcpyHostToDevice, x.stream), "seed table upload");
    std::vector<size_t> dg_at(n);   // first digest vector of blob i
    size_t v0 = 0;
    for (auto& g : groups) {
        const int ell = g.first, cnt = (int)g.second.size();
        launch_key_digest_strided(x.dt, cts[g.second[0]]->d, cnt * ell, 0, ell, 2 * ell, part, dg + 2 * v0, x.stream);
        for (int k = 0; k < cnt; ++k) dg_at[g.second[k]] = v0 + (size_t)k * ell;
        v0 += (size_t)cnt * ell;
    }
    launch_seeded_expand(x.dt, d_tab, n, max_ell, x.stream);
    hip_check(hipGetLastError(), "compact import kernels");
    std::vector<u64> h(2 * v0);
    hip_check(hipMemcpyAsync(h.data(), dg, h.size() * 8, hipMemcpyDeviceToHost, x.stream), "compact digest download");
    hip_check(hipStreamSynchronize(x.stream), "compact import sync");
    // 4. all or nothing: a handle only when every blob passed
    for (int i = 0; i < n; ++i) {
        bool in_range;
        const u64 digest = fold_key_digest(&h[2 * dg_at[i]], (size_t)hs[i].ell, in_range);
        if (!in_range) throw Error(FHELIN_ERR_ARG, "import_compact: blob " + std::to_string(i) + " holds a residue not below its modulus");
        if (digest != hs[i].digest) throw Error(FHELIN_ERR_ARG, "import_compact: blob " + std::to_string(i) + " does not match its digest");
    }
    for (int i = 0; i < n; ++i) outs[i] = wrap(c, cts[i]);   // imported: not a level-plan source, never lowered
    FHELIN_CATCH
}

int fhelin_debug_seeded_expand(fhelin_ctx* c, const uint8_t* seed32, uint64_t nonce0, int32_t ell, int32_t n_ct, int32_t reps,
                               uint64_t* out, float* ms) {
    if (!c || !seed32) return capi_fail(FHELIN_ERR_ARG, "null argument");
    FHELIN_TRY
    Context& x = c->ctx;
    x.require_device();
    if (ell < 1 || ell > x.L + 1 || n_ct < 1 || n_ct > 65535 || reps < 0) throw Error(FHELIN_ERR_ARG, "debug_seeded_expand: bad shape");
    const size_t words = (size_t)ell * x.N;
    Scratch<u64> d = x.scratch<u64>(words * n_ct);
    Scratch<SeededEntry> d_tab = x.scratch<SeededEntry>((size_t)n_ct);
    std::vector<SeededEntry> tab(n_ct);
    for (int i = 0; i < n_ct; ++i) {
        for (int w = 0; w < 8; ++w) tab[i].key.w[w] = get<uint32_t>(seed32, 4 * w);
        tab[i].nonce = nonce0 + (uint64_t)i;
        tab[i].dst = d + words * i;
        tab[i].ell = ell;
    }
    hip_check(hipMemcpyAsync(d_tab, tab.data(), tab.size() * sizeof(SeededEntry), hipMemcpyHostToDevice, x.stream), "seed table upload");
    launch_seeded_expand(x.dt, d_tab, n_ct, ell, x.stream);
    hipEvent_t ev[2] = {};
    float t = 0;
    if (reps > 0) {
        for (auto& e : ev) hip_check(hipEventCreate(&e), "hipEventCreate");
        hip_check(hipEventRecord(ev[0], x.stream), "hipEventRecord");
        for (int r = 0; r < reps; ++r) launch_seeded_expand(x.dt, d_tab, n_ct, ell, x.stream);
        hip_check(hipEventRecord(ev[1], x.stream), "hipEventRecord");
    }
    hip_check(hipGetLastError(), "seeded expand kernel");
    if (out) hip_check(hipMemcpyAsync(out, d, words * n_ct * 8, hipMemcpyDeviceToHost, x.stream), "expansion download");
    hip_check(hipStreamSynchronize(x.stream), "debug_seeded_expand sync");
    if (reps > 0) {
        (void)hipEventElapsedTime(&t, ev[0], ev[1]);
        for (auto& e : ev) (void)hipEventDestroy(e);
    }
    if (ms) *ms = reps > 0 ? t / (float)reps : 0.0f;
    FHELIN_CATCH
}

}  // extern "C"
