// Interleaved samples (include/fhelin.h "Interleaved samples"): the context setting and the client-side entry points that take or
// return one vector per sample.  Everything else reaches the stride through Context::rot_element (rotation indices), Plaintext::stride
// (replicated encodings) and the Bootstrapper's physical scope.
#include "../../include/fhelin.h"
#include <algorithm>
#include <cstring>
#include <vector>
#include "capi_internal.h"

using namespace fhelin;

#define NEED(x) if (!(x)) return capi_fail(FHELIN_ERR_ARG, "null argument")

extern "C" {

int fhelin_ctx_set_interleave(fhelin_ctx* c, int32_t stride) {
    NEED(c);
    FHELIN_TRY
    Context& x = c->ctx;
    if (stride < 1 || (stride & (stride - 1))) throw Error(FHELIN_ERR_ARG, "set_interleave: the stride must be a power of two (1, 2, 4, ...)");
    if (((long)stride << x.prm.log_slots) > x.N / 2)
        throw Error(FHELIN_ERR_ARG, "set_interleave: 2^log_slots x stride exceeds the N/2 slots of the ring");
    if (x.stride_locked)
        throw Error(FHELIN_ERR_STATE, "set_interleave: call it before the first key, plaintext, ciphertext or bootstrap set-up exists");
    x.stride = stride;
    x.stride_explicit = true;
    FHELIN_CATCH
}

int fhelin_ctx_interleave(const fhelin_ctx* c, int32_t* stride) {
    NEED(c && stride);
    *stride = c->ctx.stride;
    return FHELIN_OK;
}

int fhelin_decrypt_interleaved(fhelin_ctx* c, const fhelin_ct* ct, int32_t flood_bits, double* out, int32_t slots) {
    NEED(c && ct && out);
    if (c->ctx.device_decode) return fhelin_decrypt_batch(c, &ct, 1, flood_bits, 1, nullptr, 0, out, slots);   // the device decoder
    FHELIN_TRY
    c->ctx.require_device();
    if (c->cl.eval_only()) throw Error(FHELIN_ERR_KEY, "decrypt: an evaluation context holds no secret key");
    if (flood_bits < 0 || flood_bits > 62) throw Error(FHELIN_ERR_ARG, "decrypt_interleaved: flood_bits must lie in [0, 62]");
    if (ct->p && ct->p->wrapped()) {   // as fhelin_decrypt: the extra limb left out, every lane in the wrapped layout
        auto v = c->cl.decrypt_interleaved(ct->p, slots, flood_bits);
        std::memcpy(out, v.data(), v.size() * sizeof(double));
        return FHELIN_OK;
    }
    auto v = c->cl.decrypt_interleaved(terminal_in(c, ct), slots, flood_bits);
    std::memcpy(out, v.data(), v.size() * sizeof(double));
    FHELIN_CATCH
}

int fhelin_client_ingest_interleaved(fhelin_ctx* c, int32_t n_samples, const double* const* emb, const int32_t* const* tokens,
                                     const double* table, int32_t vocab, int32_t S, const double* cls, const double* pos,
                                     const double* E_w, const double* E_b, const double* F_w, const double* F_b, int32_t w_cols,
                                     int32_t level, fhelin_ct** outs, double* const* proj_out) {
    NEED(c && (emb || (tokens && table)) && cls && pos && E_w && E_b && F_w && F_b && outs);
    FHELIN_TRY
    if (n_samples != c->ctx.stride) throw Error(FHELIN_ERR_ARG, "ingest_interleaved: one sample per lane (n_samples == the interleave stride)");
    if (S < 1) throw Error(FHELIN_ERR_ARG, "ingest: need at least one token");
    if (level < 0 || level > c->ctx.L) throw Error(FHELIN_ERR_ARG, "ingest: level out of range");
    const int n_vec = 64 + S + 1;
    std::vector<int> drop(n_vec);
    for (int i = 0; i < n_vec; ++i) drop[i] = std::max(0, std::min(c->ctx.L - level, c->plan.next_drop(c->ctx.L + 1 - level)));
    const int first_ordinal = c->plan.next_ordinal - n_vec;
    std::vector<std::vector<double>> po;
    std::vector<CtPtr> r = c->cl.ingest_interleaved(emb, tokens, table, vocab, S, cls, pos, E_w, E_b, F_w, F_b, w_cols, level, drop,
                                                    proj_out ? &po : nullptr);
    if (proj_out)
        for (int i = 0; i < n_samples; ++i)
            if (proj_out[i]) std::memcpy(proj_out[i], po[i].data(), po[i].size() * sizeof(double));
    for (int i = 0; i < n_vec; ++i) {
        outs[i] = wrap(c, r[i]);
        if (c->plan.live(outs[i]->node, outs[i]->node_epoch)) c->plan.nodes[outs[i]->node].ordinal = first_ordinal + i;
    }
    FHELIN_CATCH
}

}  // extern "C"
