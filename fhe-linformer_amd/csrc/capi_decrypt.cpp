// Batched decryption (include/fhelin.h "Batched decryption"): a batch of ciphertexts decoded on the device - Client::decrypt_batch: one
// phase launch, one inverse NTT, the lift, the forward special FFT and the gather for the whole batch (kernels_client.hip
// phase_batch_kernel, decode_lift_kernel, fft_special_fwd_*_kernel, decode_gather_kernel), one download, one synchronisation - and the
// knob that sends the single-ciphertext decryptions through the same path.
#include "../../include/fhelin.h"
#include <vector>
#include "capi_internal.h"

using namespace fhelin;

extern "C" {

int fhelin_decrypt_batch(fhelin_ctx* c, const fhelin_ct* const* cts, int32_t n, int32_t flood_bits, int32_t all_lanes, const int32_t* idx,
                         int32_t n_idx, double* out, int32_t slots) {
    if (!c) return capi_fail(FHELIN_ERR_ARG, "null argument");
    if (n < 0) return capi_fail(FHELIN_ERR_ARG, "decrypt_batch: negative count");
    if (n == 0) return FHELIN_OK;
    if (!cts || !out) return capi_fail(FHELIN_ERR_ARG, "null argument");
    FHELIN_TRY
    // what can be refused on the arguments alone comes first, then the context, then the ciphertexts; nothing is drawn before the last
    for (int i = 0; i < n; ++i)
        if (!cts[i]) throw Error(FHELIN_ERR_ARG, "null ciphertext handle in array");
    if (n > 65535) throw Error(FHELIN_ERR_ARG, "decrypt_batch: at most 65535 ciphertexts per call");
    if (flood_bits < 0 || flood_bits > 62) throw Error(FHELIN_ERR_ARG, "decrypt_batch: flood_bits must lie in [0, 62]");
    if (idx && n_idx <= 0) throw Error(FHELIN_ERR_ARG, "decrypt_batch: an index list needs at least one entry");
    if (idx && slots > 0)
        for (int k = 0; k < n_idx; ++k)
            if (idx[k] < 0 || idx[k] >= slots) throw Error(FHELIN_ERR_ARG, "decrypt_batch: slot index outside [0, slots)");
    c->ctx.require_device();
    if (c->cl.eval_only()) throw Error(FHELIN_ERR_KEY, "decrypt: an evaluation context holds no secret key");
    std::vector<CtPtr> in;
    in.reserve(n);
    for (int i = 0; i < n; ++i) {   // per ciphertext what fhelin_decrypt does with its handle, in order
        const fhelin_ct* ct = cts[i];
        if (ct->p && ct->p->wrapped()) {   // a wrapped input: its extra limb left out, the slots in the wrapped layout
            in.push_back(ct->p);
            continue;
        }
        in.push_back(terminal_in(c, ct));
    }
    c->cl.decrypt_batch(in, slots, flood_bits, all_lanes != 0, idx, n_idx, out);
    FHELIN_CATCH
}

int fhelin_ctx_set_device_decode(fhelin_ctx* c, int32_t on) {
    if (!c) return capi_fail(FHELIN_ERR_ARG, "null argument");
    c->ctx.device_decode = on != 0;
    return FHELIN_OK;
}

}  // extern "C"
