// Sanitised replies (include/fhelin.h "Sanitised replies"): what a server hands back is the circuit's last ciphertext with the slots
// that are no answer masked out, the limbs nobody reads dropped, a fresh public-key encryption of zero added and, when asked, a
// flooding term - Client::sanitize: one sampler launch per kind, one forward NTT and ONE fused launch for a whole batch
// (kernels_client.hip sample_flood_kernel, rerandomize_combine_kernel).  The client's counterpart is the flooded decryption.
#include "../../include/fhelin.h"
#include <cstring>
#include <vector>
#include "capi_internal.h"

using namespace fhelin;

#define NEED(x) if (!(x)) return capi_fail(FHELIN_ERR_ARG, "null argument")

extern "C" {

int fhelin_sanitize(fhelin_ctx* c, const fhelin_ct* const* v, int32_t n, const fhelin_pt* mask, int32_t flood_bits, int32_t out_ell,
                    fhelin_ct** outs) {
    NEED(c && v && outs && n > 0);
    FHELIN_TRY
    c->ctx.require_device();
    std::vector<CtPtr> r = c->cl.sanitize(vec_of(c, v, n), mask ? mask->p : PtPtr(), flood_bits, out_ell);
    for (int i = 0; i < n; ++i) outs[i] = wrap(c, r[i]);
    FHELIN_CATCH
}

int fhelin_debug_flood(fhelin_ctx* c, const uint8_t* key, uint64_t stream, int32_t flood_bits, int32_t ell, uint64_t* out, size_t cap_words) {
    NEED(c && key && out);
    FHELIN_TRY
    c->ctx.require_device();
    if (ell < 1 || cap_words < (size_t)ell * c->ctx.N) throw Error(FHELIN_ERR_ARG, "debug_flood: buffer too small");
    std::vector<u64> h = c->cl.debug_flood(key, stream, flood_bits, ell);
    std::memcpy(out, h.data(), h.size() * sizeof(u64));
    FHELIN_CATCH
}

int fhelin_debug_sampler_peek(const fhelin_ctx* c, int32_t n_keys, uint32_t* key_words, uint64_t* sample_calls) {
    NEED(c && (key_words || n_keys == 0));
    FHELIN_TRY
    if (n_keys < 0 || n_keys > 4096) throw Error(FHELIN_ERR_ARG, "debug_sampler_peek: n_keys must lie in [0, 4096]");
    c->cl.debug_sampler_peek(n_keys, key_words, sample_calls);
    FHELIN_CATCH
}

int fhelin_decrypt_flooded(fhelin_ctx* c, const fhelin_ct* ct, int32_t flood_bits, double* out, int32_t slots) {
    NEED(c && ct && out);
    if (c->ctx.device_decode) return fhelin_decrypt_batch(c, &ct, 1, flood_bits, 0, nullptr, 0, out, slots);   // the device decoder
    FHELIN_TRY
    c->ctx.require_device();
    if (c->cl.eval_only()) throw Error(FHELIN_ERR_KEY, "decrypt: an evaluation context holds no secret key");
    if (flood_bits < 0 || flood_bits > 62) throw Error(FHELIN_ERR_ARG, "decrypt_flooded: flood_bits must lie in [0, 62]");
    if (ct->p && ct->p->wrapped()) {   // as fhelin_decrypt: the extra limb left out, the slots in the wrapped layout
        auto v = c->cl.decrypt(ct->p, slots, flood_bits);
        std::memcpy(out, v.data(), v.size() * sizeof(double));
        return FHELIN_OK;
    }
    auto v = c->cl.decrypt(terminal_in(c, ct), slots, flood_bits);
    std::memcpy(out, v.data(), v.size() * sizeof(double));
    FHELIN_CATCH
}

}  // extern "C"
