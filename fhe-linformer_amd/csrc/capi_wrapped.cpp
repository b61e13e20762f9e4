// Wrapped inputs (include/fhelin.h "Wrapped inputs"): the client packs up to 128 inputs of a sample into one ciphertext over one limb
// more than they need; the server unwraps them into the expanded inputs fhelin_client_ingest gives.  Under a slot stride the same
// inputs of every sample of a group share the wrapped ciphertext (fhelin_client_ingest_wrapped_interleaved), and the unwrap below serves
// all lanes at once: its mask is replicated, its rotation indices are logical.
//   unwrap, per input t of a wrapped ciphertext W (column t of the layout):
//     x_t   = drop_last_limb(W * mask_t)      mask_t = the stored mask (slots = 0 mod 128) read through the map of rotation -t,
//                                             encoded at scale q_drop: x_t has the inputs' limbs and exactly their fresh scale
//     out_t = R3(R2(R1(x_t)))                 t = a + 8b + 64c; R1 = id + rot by {a-7..a}\{0}, R2 = id + rot by 8{b-7..b}\{0},
//                                             R3 = id + rot by 64c - 64 or 64c: together sum_{k<128} rot(x_t, t - k)
//   The masked product is ONE launch per call (launch_wrap_mask); the limb drop is the rescale path (INTT of the dropped limb, its
//   centred lift finished in the forward NTT's row pass); R1..R3 are merged key switches (Evaluator::rotate_sum_batch) over all rows
//   that share a, b or c.
#include "../../include/fhelin.h"
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstring>
#include <map>
#include <set>
#include <vector>
#include "capi_internal.h"
#include "kernels_elem.h"

using namespace fhelin;

#define NEED(x) if (!(x)) return capi_fail(FHELIN_ERR_ARG, "null argument")

namespace {

const CtPtr& wrapped_in(const fhelin_ct* h) {
    if (!h || !h->p || !h->p->wrapped()) throw Error(FHELIN_ERR_ARG, "unwrap: not a wrapped input ciphertext");
    return h->p;
}

// the merged key switches of input column t: R1, R2, R3 (offsets without the identity term)
std::vector<int> unwrap_offsets(int step, int t) {
    std::vector<int> r;
    if (step == 0 || step == 1) {
        const int u = step == 0 ? t % 8 : (t / 8) % 8, m = step == 0 ? 1 : 8;
        for (int k = u - 7; k <= u; ++k)
            if (k) r.push_back(m * k);
    } else {
        r.push_back(t >= 64 ? 64 : -64);
    }
    return r;
}

const PtPtr& mask_of(fhelin_ctx* c) {
    if (!c->wrap_mask) {
        auto p = std::make_shared<Plaintext>();
        p->ctx = &c->ctx;
        p->slots = 1 << c->ctx.prm.log_slots;
        p->stride = c->ctx.stride;   // interleaved samples: the same columns in every lane
        p->level = 0;
        p->values.assign(p->slots, 0.0);
        for (int i = 0; i < p->slots; i += 128) p->values[i] = 1.0;
        c->wrap_mask = p;
    }
    return c->wrap_mask;
}

void p0_tables(fhelin_ctx* c) {
    if (c->p0_qlinv) return;
    Context& x = c->ctx;
    const u64 p0 = x.moduli[x.L + 1];
    std::vector<u64> inv(2 * (size_t)(x.L + 1)), mod(x.L + 1);
    for (int t = 0; t <= x.L; ++t) {
        const u64 q = x.chain.q[t];
        mod[t] = p0 % q;
        inv[2 * t] = h_invmod(mod[t], q);
        inv[2 * t + 1] = h_shoup(inv[2 * t], q);
    }
    c->p0_qlinv = x.upload_table(inv);
    c->p0_qlmod = x.upload_table(mod);
}

// the limbs every input is wanted at: the caller's, or n_q - level, or - while a level plan is applied - the plan's targets of the
// sources the unwrap will produce (peeked: the unwrap counts them)
std::vector<int> wrap_targets(fhelin_ctx* c, int n_vec, int level, const int32_t* targets) {
    const int top = c->ctx.L + 1 - level;
    std::vector<int> ell(n_vec, top);
    const LevelPlan& pl = c->plan;
    for (int i = 0; i < n_vec; ++i) {
        if (targets) {
            ell[i] = targets[i];
        } else if (pl.mode == 2) {
            const int k = pl.next_ordinal + i;
            if (k < (int)pl.target.size() && pl.target[k] >= 1) ell[i] = std::max(1, std::min(top, pl.target[k]));
        }
    }
    return ell;
}

}  // namespace

extern "C" {

int fhelin_client_ingest_wrapped(fhelin_ctx* c, const double* emb, const int32_t* tokens, const double* table, int32_t vocab, int32_t S,
                                 const double* cls, const double* pos, const double* E_w, const double* E_b, const double* F_w,
                                 const double* F_b, int32_t w_cols, int32_t level, const int32_t* targets, fhelin_ct** outs,
                                 int32_t* n_out, double* proj_out) {
    NEED(c && (emb || (tokens && table)) && cls && pos && E_w && E_b && F_w && F_b && outs && n_out);
    FHELIN_TRY
    *n_out = 0;
    if (c->ctx.stride > 1)
        throw Error(FHELIN_ERR_STATE, "client_ingest_wrapped: a context with interleaved samples takes its samples through fhelin_client_ingest_wrapped_interleaved: "
                                      "wrapped inputs of interleaved samples are not supported here (interleave stride > 1)");
    if (S < 1) throw Error(FHELIN_ERR_ARG, "ingest: need at least one token");
    if (level < 0 || level > c->ctx.L) throw Error(FHELIN_ERR_ARG, "ingest: level out of range");
    if (c->ctx.K < 1) throw Error(FHELIN_ERR_STATE, "wrapped inputs: a chain without special primes has no p_0 limb");
    const int n_vec = 64 + S + 1;
    const std::vector<int> ell = wrap_targets(c, n_vec, level, targets);
    std::vector<double> po;
    std::vector<CtPtr> r = c->cl.ingest_sample(emb, tokens, table, vocab, S, cls, pos, E_w, E_b, F_w, F_b, w_cols, level,
                                               std::vector<int>(n_vec, 0), proj_out ? &po : nullptr, &ell);
    if (proj_out) std::memcpy(proj_out, po.data(), po.size() * sizeof(double));
    for (size_t i = 0; i < r.size(); ++i) outs[i] = wrap(c, r[i]);
    *n_out = (int32_t)r.size();
    FHELIN_CATCH
}

int fhelin_client_ingest_wrapped_interleaved(fhelin_ctx* c, int32_t n_samples, const double* const* emb, const int32_t* const* tokens,
                                             const double* table, int32_t vocab, int32_t S, const double* cls, const double* pos,
                                             const double* E_w, const double* E_b, const double* F_w, const double* F_b, int32_t w_cols,
                                             int32_t level, const int32_t* targets, fhelin_ct** outs, int32_t* n_out,
                                             double* const* proj_out) {
    NEED(c && (emb || (tokens && table)) && cls && pos && E_w && E_b && F_w && F_b && outs && n_out);
    if (c->ctx.stride == 1 && n_samples == 1 && (emb ? emb[0] != nullptr : tokens[0] != nullptr))   // the single-sample call itself
        return fhelin_client_ingest_wrapped(c, emb ? emb[0] : nullptr, emb ? nullptr : tokens[0], table, vocab, S, cls, pos, E_w, E_b, F_w,
                                            F_b, w_cols, level, targets, outs, n_out, proj_out ? proj_out[0] : nullptr);
    FHELIN_TRY
    *n_out = 0;
    if (n_samples != c->ctx.stride)
        throw Error(FHELIN_ERR_ARG, "ingest_wrapped_interleaved: one sample per lane (n_samples == the interleave stride)");
    if (S < 1) throw Error(FHELIN_ERR_ARG, "ingest: need at least one token");
    if (level < 0 || level > c->ctx.L) throw Error(FHELIN_ERR_ARG, "ingest: level out of range");
    if (c->ctx.K < 1) throw Error(FHELIN_ERR_STATE, "wrapped inputs: a chain without special primes has no p_0 limb");
    const int n_vec = 64 + S + 1;
    const std::vector<int> ell = wrap_targets(c, n_vec, level, targets);
    std::vector<std::vector<double>> po;
    std::vector<CtPtr> r = c->cl.ingest_interleaved(emb, tokens, table, vocab, S, cls, pos, E_w, E_b, F_w, F_b, w_cols, level,
                                                    std::vector<int>(n_vec, 0), proj_out ? &po : nullptr, &ell);
    if (proj_out)
        for (int i = 0; i < n_samples; ++i)
            if (proj_out[i]) std::memcpy(proj_out[i], po[i].data(), po[i].size() * sizeof(double));
    for (size_t i = 0; i < r.size(); ++i) outs[i] = wrap(c, r[i]);
    *n_out = (int32_t)r.size();
    FHELIN_CATCH
}

int fhelin_wrapped_info(const fhelin_ct* ct, int32_t* count, int32_t* total, int32_t* ell, int32_t* positions, int32_t cap) {
    NEED(ct);
    FHELIN_TRY
    const CtPtr& p = wrapped_in(ct);
    if (count) *count = (int32_t)p->wrap_pos.size();
    if (total) *total = p->wrap_total;
    if (ell) *ell = p->ell - 1;
    if (positions)
        for (int t = 0; t < (int)p->wrap_pos.size() && t < cap; ++t) positions[t] = p->wrap_pos[t];
    FHELIN_CATCH
}

int fhelin_unwrap_inputs(fhelin_ctx* c, const fhelin_ct* const* wrapped, int32_t n, fhelin_ct** outs) {
    NEED(c && n >= 0 && (n == 0 || (wrapped && outs)));
    FHELIN_TRY
    Context& x = c->ctx;
    x.require_device();
    if (n == 0) return FHELIN_OK;
    if (x.K < 1) throw Error(FHELIN_ERR_STATE, "unwrap: hybrid key switching needs at least one special prime");
    const int slots = 1 << x.prm.log_slots;
    // rows in output order: sample by sample (consecutive handles whose counts add up to their total), inputs in read order
    struct Row {
        int w, t, pos, sample;
    };
    std::vector<Row> rows;
    std::vector<int> sample_total;
    std::vector<CtPtr> w(n);
    for (int i = 0; i < n;) {
        const int total = wrapped_in(wrapped[i])->wrap_total;
        std::vector<std::pair<int, int>> at(total, {-1, -1});
        int seen = 0, j = i;
        for (; j < n && seen < total; ++j) {
            w[j] = wrapped_in(wrapped[j]);
            const Ciphertext& ct = *w[j];
            if (ct.wrap_total != total || ct.npoly != 2 || ct.deg != 1 || ct.slots != slots || slots != 16384 || ct.ell < 2 ||
                ct.ell > x.L + 2)
                throw Error(FHELIN_ERR_ARG, "unwrap: wrapped ciphertext " + std::to_string(j) + " does not fit (shape, or sample mixed with another)");
            for (int t = 0; t < (int)ct.wrap_pos.size(); ++t) {
                const int p = ct.wrap_pos[t];
                if (p < 0 || p >= total || at[p].first >= 0) throw Error(FHELIN_ERR_ARG, "unwrap: an input occurs twice in one sample");
                at[p] = {j, t};
                ++seen;
            }
        }
        if (seen != total) throw Error(FHELIN_ERR_ARG, "unwrap: the wrapped ciphertexts of a sample do not hold all of its inputs");
        for (int p = 0; p < total; ++p) rows.push_back(Row{at[p].first, at[p].second, p, (int)sample_total.size()});
        sample_total.push_back(total);
        i = j;
    }
    // every rotation key first (nothing is launched when one is missing)
    std::set<int> need;
    for (const Row& r : rows)
        for (int step = 0; step < 3; ++step)
            for (int k : unwrap_offsets(step, r.t)) need.insert(k);
    for (int k : need)
        if (!c->ev.rot_keys.count(x.rot_element(k)))
            throw Error(FHELIN_ERR_KEY, "unwrap: no rotation key for index " + std::to_string(k) + " (EvalRotateKeyGen list)");
    const size_t N = x.N;
    const int R = (int)rows.size();
    // level plan: the outputs are the sources fhelin_client_ingest's outputs are (same ordinals).  Applying, an output whose input was
    // wrapped above its planned limbs tau is made at tau directly: the masked product reads the first tau + 1 limbs and its mask is
    // encoded at Delta_tau q_tau / Delta_ell, so that the drop of q_tau leaves exactly the fresh scale Delta_tau.
    LevelPlan& pl = c->plan;
    std::vector<int> base(sample_total.size());
    for (size_t s = 0; s < sample_total.size(); ++s) {
        base[s] = pl.next_ordinal;
        pl.next_ordinal += sample_total[s];
    }
    std::vector<int> out_ell(R);
    for (int r = 0; r < R; ++r) {
        const int ell = w[rows[r].w]->ell - 1, k = base[rows[r].sample] + rows[r].pos;
        out_ell[r] = ell;
        if (pl.mode == 2 && k < (int)pl.target.size() && pl.target[k] >= 1) out_ell[r] = std::min(ell, pl.target[k]);
    }
    // masked product, one launch: rows grouped by their output limb count (each group one block, rows in output order inside it)
    std::map<int, std::vector<int>> by_ell;   // output limbs + 1 -> rows
    for (int r = 0; r < R; ++r) by_ell[out_ell[r] + 1].push_back(r);
    std::vector<Scratch<u64>> blk;   // the products, one block per limb count: held until the call returns
    std::vector<WrapMaskRow> tab(R);
    std::map<int, u64*> prod;
    const PtPtr& mask = mask_of(c);
    std::map<std::pair<int, int>, std::shared_ptr<Encoding>> encs;   // (output limbs, input limbs) -> mask encoding, held until the launch
    int max_ell = 0;
    for (auto& g : by_ell) {
        const int ell1 = g.first, tau = ell1 - 1;
        blk.push_back(x.scratch<u64>(g.second.size() * 2 * (size_t)ell1 * N));
        u64* d = blk.back();
        prod[ell1] = d;
        for (size_t k = 0; k < g.second.size(); ++k) {
            const Row& r = rows[g.second[k]];
            const int ell = w[r.w]->ell - 1;
            auto& enc = encs[{tau, ell}];
            if (!enc) {   // at scale q_drop (the drop divides it out exactly); lowered: Delta_tau q_tau / Delta_ell
                const long double q = (long double)x.moduli[tau];
                enc = mask->at(ell1, tau == ell ? q : x.sf_real[x.L + 1 - tau] * q / x.sf_real[x.L + 1 - ell]);
            }
            tab[g.second[k]] = WrapMaskRow{w[r.w]->d, d + k * 2 * (size_t)ell1 * N, enc->d, x.automorph_map(x.rot_element(-r.t)), ell1,
                                           w[r.w]->ell};
        }
        max_ell = std::max(max_ell, ell1);
    }
    if (R > 65535) throw Error(FHELIN_ERR_ARG, "unwrap: at most 65535 inputs per call");
    Scratch<WrapMaskRow> d_tab = x.scratch<WrapMaskRow>((size_t)R);
    hip_check(hipMemcpyAsync(d_tab, tab.data(), (size_t)R * sizeof(WrapMaskRow), hipMemcpyHostToDevice, x.stream), "unwrap row table");
    launch_wrap_mask(x.dt, d_tab, R, max_ell, x.stream);
    hip_check(hipGetLastError(), "unwrap mask kernel");
    x.stats.ct_pt_mult += (u64)R;
    // drop the extra limb as a rescale does, at most batch_limit rows per launch set
    std::vector<CtPtr> xs(R);
    for (auto& g : by_ell) {
        const int ell1 = g.first, ell = ell1 - 1;
        const u64 *qlinv = nullptr, *qlm = nullptr;
        if (ell == x.L + 1) {   // the extra limb is p_0
            p0_tables(c);
            qlinv = c->p0_qlinv;
            qlm = c->p0_qlmod;
        }
        const long double scale = x.sf_real[x.L + 1 - ell];   // exactly a fresh encryption's at ell limbs
        for (size_t k0 = 0; k0 < g.second.size(); k0 += (size_t)c->ev.batch_limit) {
            const int B = (int)std::min(g.second.size() - k0, (size_t)c->ev.batch_limit), P = 2 * B;
            const u64* base_d = prod[ell1] + k0 * 2 * (size_t)ell1 * N;
            Scratch<u64> last = x.scratch<u64>((size_t)P * N);
            LimbBatch lb{last, P, nullptr, ell1 - 1, 1, base_d + (size_t)(ell1 - 1) * N};
            lb.src_group = 1;
            lb.src_group_stride = (size_t)ell1 * N;
            x.ntt(lb, true);
            std::vector<CtPtr> o = c->ev.new_ct_batch(B, 2, ell, 1, scale, slots);
            c->ev.rescale_finish(o[0]->d, base_d, last, P, ell1, qlinv, qlm);
            hip_check(hipGetLastError(), "unwrap limb drop");
            last.reset();
            x.stats.rescale += (u64)B;
            x.stats.rescale_limbs += (u64)B * ell1;
            for (int b = 0; b < B; ++b) xs[g.second[k0 + b]] = o[b];
        }
    }
    // replication: R1, R2, R3, each one merged key switch per row, rows that share their offsets batched together
    for (int step = 0; step < 3; ++step) {
        std::map<std::vector<int>, std::vector<int>> by_off;
        for (int r = 0; r < R; ++r) by_off[unwrap_offsets(step, rows[r].t)].push_back(r);
        for (auto& g : by_off) {
            std::vector<CtPtr> in;
            for (int r : g.second) in.push_back(xs[r]);
            std::vector<CtPtr> o = c->ev.rotate_sum_batch(in, g.first);
            for (size_t k = 0; k < g.second.size(); ++k) xs[g.second[k]] = o[k];
        }
    }
    for (int r = 0; r < R; ++r) {
        outs[r] = wrap(c, xs[r]);
        if (pl.live(outs[r]->node, outs[r]->node_epoch)) pl.nodes[outs[r]->node].ordinal = base[rows[r].sample] + rows[r].pos;
    }
    FHELIN_CATCH
}

}  // extern "C"
