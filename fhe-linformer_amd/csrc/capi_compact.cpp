// extern "C" boundary, part 5: seeded secret-key encryption and compact ciphertexts (include/fhelin.h "Compact ciphertexts": the
// expansion and the blob format are documented there).  A seeded encryption's c1 is the expansion of a public (seed, nonce), so a
// compact blob carries c0 alone.  The header codec is wire_header.h (CC_FORMATS: versions 1 and 2); the import is wire.cpp's
// import_blobs, of which a compact payload is the 64-bit case: every c0 uploaded straight into its ciphertext, range-checked and
// digested on the device (kernels_keys.hip), every c1 expanded in one launch (kernels_seeded.hip), one host synchronisation per call.
#include "../../include/fhelin.h"
#include <hip/hip_runtime.h>
#include <vector>
#include "capi_internal.h"
#include "kernels_seeded.h"
#include "wire.h"

using namespace fhelin;

namespace {

const char* const NOT_SEEDED = "compact form: only an unmodified seeded (secret-key) encryption has one";

// the header of ct's compact blob but for the digest: version 2 for a wrapped input
BlobHeader compact_header(const Context& x, const Ciphertext& ct) { return blob_header_of(CC_FORMATS[ct.wrapped() ? 1 : 0], x, ct, 1); }

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
    if (!ct->p || !ct->p->seeded) return capi_fail(FHELIN_ERR_STATE, NOT_SEEDED);
    FHELIN_TRY
    *bytes = compact_header(*ct->p->ctx, *ct->p).bytes();
    FHELIN_CATCH
}

int fhelin_ct_export_compact(fhelin_ctx* c, const fhelin_ct* ct, uint8_t* out, size_t cap) {
    if (!c || !ct || !out) return capi_fail(FHELIN_ERR_ARG, "null argument");
    FHELIN_TRY
    if (!ct->p || !ct->p->seeded) throw Error(FHELIN_ERR_STATE, NOT_SEEDED);
    const bool wrapped = ct->p->wrapped();   // version 2; a wrapped input is not a value of the pass (no level-plan terminal)
    const CtPtr& p = wrapped ? ct->p : terminal_in(c, ct);
    Context& x = c->ctx;
    BlobHeader h = compact_header(x, *p);
    if (cap < h.bytes()) throw Error(FHELIN_ERR_ARG, "export_compact: buffer too small");
    if (x.N % 4096) throw Error(FHELIN_ERR_ARG, "export_compact: ring dimension below 2^12");
    // c0's digest on the device, c0 itself straight into the blob; one synchronisation
    DigestRun run(x, {DigestItem{p->d, (size_t)h.ell, 0, h.ell, h.ell}});
    hip_check(hipMemcpyAsync(out + h.header_bytes(), p->d, h.words_per_poly * 8, hipMemcpyDeviceToHost, x.stream), "compact export");
    hip_check(hipStreamSynchronize(x.stream), "compact export sync");
    bool in_range;
    h.digest = run.fold(0, 0, (size_t)h.ell, in_range);
    if (!in_range) throw Error(FHELIN_ERR_INTERNAL, "export_compact: c0 holds a residue out of range");
    write_blob_header(h, out);
    FHELIN_CATCH
}

int fhelin_compact_info(const uint8_t* blob, size_t bytes, int32_t* log_n, int32_t* ell, int32_t* deg, int32_t* slots) {
    FHELIN_TRY
    const BlobHeader h = read_blob_header(CC_FORMATS, 2, blob, bytes);
    if (log_n) *log_n = h.log_n;
    if (ell) *ell = h.ell;
    if (deg) *deg = h.deg;
    if (slots) *slots = h.slots;
    FHELIN_CATCH
}

int fhelin_ct_import_compact(fhelin_ctx* c, const uint8_t* const* blobs, const size_t* sizes, int32_t n, fhelin_ct** outs) {
    if (!c || (n > 0 && (!blobs || !sizes || !outs)) || n < 0) return capi_fail(FHELIN_ERR_ARG, "null argument");
    FHELIN_TRY
    import_blobs(c, "import_compact", CC_FORMATS, 2, blobs, sizes, n, outs);
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
