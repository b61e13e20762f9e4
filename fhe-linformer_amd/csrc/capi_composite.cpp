// extern "C" boundary, part 3: one entry point per FHEController composite method.
#include "../../include/fhelin.h"
#include <algorithm>
#include "capi_internal.h"

using namespace fhelin;

#define NEED(x) if (!(x)) return capi_fail(FHELIN_ERR_ARG, "null argument")

static void emit(fhelin_ctx* c, const CtVec& v, fhelin_ct** outs) {
    for (size_t i = 0; i < v.size(); ++i) outs[i] = wrap(c, v[i]);
}
static PtPtr opt(const fhelin_pt* p) { return p ? p->p : PtPtr(); }
// generate_containers: every one of the `total` inputs is an unread row of matmulRElarge with one set of weights, bias and mask, so the
// two calls can run as one (Composite::relarge_containers).  Returns that common description, or null.  On success the call in progress
// consumes, for the level plan, what the rows of matmulRElarge would have consumed.
static const LazyRows* unread_relarge_rows(fhelin_ctx* c, const fhelin_ct* const* inputs, int total) {
    if (total <= 0 || !c->comp.fuse_relarge) return nullptr;
    const LazyRows* g0 = nullptr;
    for (int i = 0; i < total; ++i) {
        const fhelin_ct* h = inputs[i];
        if (!h) throw Error(FHELIN_ERR_ARG, "null ciphertext handle in array");
        const LazyRows* g = (!h->p && !h->heavy && h->lazy) ? h->lazy.get() : nullptr;
        if (!g || g->kind != LazyRows::RElarge || g->done[h->lazy_idx] || g->rows.size() != g->done.size()) return nullptr;
        if (!g0) g0 = g;
        if (!(g->weights == g0->weights && g->bias == g0->bias && g->mask_val == g0->mask_val)) return nullptr;
    }
    for (int i = 0; i < total; ++i)
        if (c->plan.live(inputs[i]->node, inputs[i]->node_epoch))
            for (int in : c->plan.nodes[inputs[i]->node].in) plan_inputs().push_back(in);
    return g0;
}
static const CtPtr& relarge_input(const fhelin_ct* h) { return h->lazy->rows[h->lazy_idx]; }   // of a handle unread_relarge_rows accepted

// ---- bootstraps and the level plan: a bootstrap is a terminal for its input (two limbs are all it reads) and a source for its output
static void bootstrap_reads(fhelin_ctx* c, const fhelin_ct* h) {
    if (c->plan.live(h->node, h->node_epoch)) c->plan.terminal(h->node, 2);
}
// outs of one call as sources of the level plan, in call order from first_ordinal
static void emit_sources(fhelin_ctx* c, const CtVec& r, int first_ordinal, fhelin_ct** outs) {
    plan_inputs().clear();
    for (size_t i = 0; i < r.size(); ++i) {
        outs[i] = wrap(c, r[i]);
        if (c->plan.live(outs[i]->node, outs[i]->node_epoch)) c->plan.nodes[outs[i]->node].ordinal = first_ordinal + (int)i;
    }
}
// the one output of a call that has just taken its source number (LevelPlan::next_drop)
static fhelin_ct* emit_source(fhelin_ctx* c, const CtPtr& r) {
    fhelin_ct* out;
    emit_sources(c, CtVec{r}, c->plan.next_ordinal - 1, &out);
    return out;
}
// The batched bootstrap entry points.  Every ciphertext is a source of the level plan of its own, numbered in call order: next_drop()
// gives the planned drop of the next one.  Those with the same planned drop share one run(sub, drop), groups in first-seen order.
template <class NextDrop, class Run>
static void bootstrap_by_drop(fhelin_ctx* c, const fhelin_ct* const* v, int n, fhelin_ct** outs, NextDrop&& next_drop, Run&& run) {
    const CtVec in = vec_of(c, v, n);
    std::vector<int> drop(n);
    for (int i = 0; i < n; ++i) {
        drop[i] = next_drop();
        bootstrap_reads(c, v[i]);
    }
    const int first_ordinal = c->plan.next_ordinal - n;
    CtVec r(n);
    std::vector<char> done(n, 0);
    for (int i = 0; i < n; ++i) {
        if (done[i]) continue;
        std::vector<int> pick;
        CtVec sub;
        for (int k = i; k < n; ++k)
            if (!done[k] && drop[k] == drop[i]) {
                pick.push_back(k);
                sub.push_back(in[k]);
                done[k] = 1;
            }
        const CtVec o = run(sub, drop[i]);
        for (size_t k = 0; k < pick.size(); ++k) r[pick[k]] = o[k];
    }
    emit_sources(c, r, first_ordinal, outs);
}

extern "C" {

int fhelin_ct_force(fhelin_ctx* c, const fhelin_ct* const* v, int32_t n) {
    NEED(c && (v || n == 0) && n >= 0);
    FHELIN_TRY
    LazyGroups groups = lazy_groups(c, v, n, true);
    force_rows_multi(c, groups);   // exactly these rows (force_group would widen a second partial read); same calls on several samples merged
    FHELIN_CATCH
}
int fhelin_rotate_batch(fhelin_ctx* c, const fhelin_ct* const* v, int32_t n, int32_t index, fhelin_ct** outs) {
    NEED(c && v && outs && n >= 0);
    FHELIN_TRY
    emit(c, c->ev.rotate_batch(vec_of(c, v, n), index), outs);
    FHELIN_CATCH
}
int fhelin_rescale_batch(fhelin_ctx* c, const fhelin_ct* const* v, int32_t n, fhelin_ct** outs) {
    NEED(c && v && outs && n >= 0);
    FHELIN_TRY
    emit(c, c->ev.rescale_batch(vec_of(c, v, n)), outs);
    FHELIN_CATCH
}
int fhelin_mult_plain_batch(fhelin_ctx* c, const fhelin_ct* const* v, int32_t n, const fhelin_pt* p, fhelin_ct** outs) {
    NEED(c && v && p && outs && n >= 0);
    FHELIN_TRY
    emit(c, c->ev.mult_plain_batch(vec_of(c, v, n), p->p), outs);
    FHELIN_CATCH
}
int fhelin_mult_batch(fhelin_ctx* c, const fhelin_ct* const* a, const fhelin_ct* const* b, int32_t n, fhelin_ct** outs) {
    NEED(c && a && b && outs && n >= 0);
    FHELIN_TRY
    emit(c, c->ev.mult_batch(vec_of(c, a, n), vec_of(c, b, n)), outs);
    FHELIN_CATCH
}
int fhelin_mult_affine_batch(fhelin_ctx* c, const fhelin_ct* const* a, const fhelin_ct* const* b, int32_t n, const int32_t* f, const double* cadd,
                             const fhelin_ct* const* addend, const int32_t* negate, fhelin_ct** outs) {
    NEED(c && a && b && f && cadd && outs && n >= 0 && (!addend || negate));
    FHELIN_TRY
    std::vector<Evaluator::AffineSpec> spec(n);
    for (int i = 0; i < n; ++i) {
        spec[i].f = f[i];
        spec[i].cadd = cadd[i];
        if (addend && addend[i]) {
            force_many(c, &addend[i], 1);
            spec[i].addend = ct_in(c, addend[i]);
            spec[i].negate = negate[i] != 0;
        }
    }
    emit(c, c->ev.mult_affine_batch(vec_of(c, a, n), vec_of(c, b, n), spec), outs);
    FHELIN_CATCH
}
int fhelin_add_batch(fhelin_ctx* c, const fhelin_ct* const* a, const fhelin_ct* const* b, int32_t n, fhelin_ct** outs) {
    NEED(c && a && b && outs && n >= 0);
    FHELIN_TRY
    emit(c, c->ev.add_batch(vec_of(c, a, n), vec_of(c, b, n)), outs);
    FHELIN_CATCH
}
int fhelin_fc_mult_const(fhelin_ctx* c, const fhelin_ct* a, double d, fhelin_ct** out) {
    NEED(c && a && out);
    FHELIN_TRY
    *out = wrap(c, c->comp.mult_const(ct_in(c, a), d));
    FHELIN_CATCH
}
int fhelin_fc_mask(fhelin_ctx* c, const fhelin_ct* a, int32_t kind, int32_t x, int32_t y, double v, fhelin_ct** out) {
    NEED(c && a && out);
    FHELIN_TRY
    switch (kind) {
        case 0: *out = wrap(c, c->comp.mask_block(ct_in(c, a), x, y, v)); break;
        case 1: *out = wrap(c, c->comp.mask_heads(ct_in(c, a), v)); break;
        case 2: *out = wrap(c, c->comp.mask_heads_128(ct_in(c, a), v)); break;
        case 3: *out = wrap(c, c->comp.mask_mod_n(ct_in(c, a), x, y)); break;
        case 4: *out = wrap(c, c->comp.mask_first_n(ct_in(c, a), x, v)); break;
        default: throw Error(FHELIN_ERR_ARG, "unknown mask kind");
    }
    FHELIN_CATCH
}
int fhelin_fc_rotsum(fhelin_ctx* c, const fhelin_ct* a, int32_t slots, int32_t padding, fhelin_ct** out) {
    NEED(c && a && out);
    FHELIN_TRY
    *out = wrap(c, c->comp.rotsum(ct_in(c, a), slots, padding));
    FHELIN_CATCH
}
int fhelin_fc_repeat(fhelin_ctx* c, const fhelin_ct* a, int32_t slots, int32_t padding, fhelin_ct** out) {
    NEED(c && a && out);
    FHELIN_TRY
    *out = wrap(c, c->comp.repeat(ct_in(c, a), slots, padding));
    FHELIN_CATCH
}
int fhelin_fc_add_many(fhelin_ctx* c, const fhelin_ct* const* v, int32_t n, fhelin_ct** out) {
    NEED(c && v && out);
    FHELIN_TRY
    *out = wrap(c, c->comp.add_many(vec_of(c, v, n)));
    FHELIN_CATCH
}
int fhelin_fc_matmul_pt(fhelin_ctx* c, const fhelin_ct* const* rows, int32_t n, const fhelin_pt* w, const fhelin_pt* bias,
                        int32_t slots, int32_t padding, fhelin_ct** outs) {
    NEED(c && rows && w && outs);
    FHELIN_TRY
    if (c->lazy_rows && n > 1) {
        auto g = std::make_shared<LazyRows>();
        g->kind = LazyRows::MatmulPt;
        g->rows = vec_of(c, rows, n);
        g->w = w->p;
        g->bias = opt(bias);
        g->slots = slots;
        g->padding = padding;
        emit_lazy(c, g, n, outs);
    } else {
        emit(c, c->comp.matmul_pt(vec_of(c, rows, n), w->p, opt(bias), slots, padding), outs);
    }
    FHELIN_CATCH
}
int fhelin_fc_matmul_ct(fhelin_ctx* c, const fhelin_ct* const* rows, int32_t n, const fhelin_ct* w, int32_t slots,
                        int32_t padding, fhelin_ct** outs) {
    NEED(c && rows && w && outs);
    FHELIN_TRY
    emit(c, c->comp.matmul_ct(vec_of(c, rows, n), ct_in(c, w), slots, padding), outs);
    FHELIN_CATCH
}
int fhelin_fc_matmulRElarge(fhelin_ctx* c, const fhelin_ct* const* rows, int32_t n, const fhelin_pt* const* weights, int32_t nw,
                            const fhelin_pt* bias, double mask_val, fhelin_ct** outs) {
    NEED(c && rows && weights && outs);
    FHELIN_TRY
    std::vector<PtPtr> w;
    for (int i = 0; i < nw; ++i) {
        if (!weights[i]) throw Error(FHELIN_ERR_ARG, "null weight");
        w.push_back(weights[i]->p);
    }
    if (c->lazy_rows && n >= 1) {      // rows that generate_containers reads next are never evaluated on their own (deferred.h)
        auto g = std::make_shared<LazyRows>();
        g->kind = LazyRows::RElarge;
        g->rows = vec_of(c, rows, n);
        g->weights = w;
        g->bias = opt(bias);
        g->mask_val = mask_val;
        emit_lazy(c, g, n, outs);
    } else {
        emit(c, c->comp.matmulRElarge(vec_of(c, rows, n), w, opt(bias), mask_val), outs);
    }
    FHELIN_CATCH
}
int fhelin_fc_matmulCRlarge(fhelin_ctx* c, const fhelin_ct* const* rows, int32_t n, const fhelin_pt* const* weights,
                            const fhelin_pt* bias, fhelin_ct** outs) {
    NEED(c && rows && weights && outs);
    FHELIN_TRY
    std::vector<PtPtr> w;
    for (int i = 0; i < 4; ++i) {
        if (!weights[i]) throw Error(FHELIN_ERR_ARG, "null weight");
        w.push_back(weights[i]->p);
    }
    std::vector<CtVec> r;
    for (int i = 0; i < n; ++i) r.push_back(vec_of(c, rows + 4 * i, 4));
    emit(c, c->comp.matmulCRlarge(r, w, opt(bias)), outs);
    FHELIN_CATCH
}
int fhelin_fc_matmulScores(fhelin_ctx* c, const fhelin_ct* const* queries, int32_t n, const fhelin_ct* key, fhelin_ct** out) {
    NEED(c && queries && key && out);
    FHELIN_TRY
    *out = wrap(c, c->comp.matmulScores(vec_of(c, queries, n), ct_in(c, key)));
    FHELIN_CATCH
}
int fhelin_fc_wrapUpRepeated(fhelin_ctx* c, const fhelin_ct* const* v, int32_t n, fhelin_ct** out) {
    NEED(c && v && out);
    FHELIN_TRY
    *out = wrap(c, c->comp.wrapUpRepeated(vec_of(c, v, n)));
    FHELIN_CATCH
}
int fhelin_fc_wrapUpExpanded(fhelin_ctx* c, const fhelin_ct* const* v, int32_t n, fhelin_ct** out) {
    NEED(c && v && out);
    FHELIN_TRY
    *out = wrap(c, c->comp.wrapUpExpanded(vec_of(c, v, n)));
    FHELIN_CATCH
}
int fhelin_fc_unwrapExpanded(fhelin_ctx* c, const fhelin_ct* a, int32_t n, fhelin_ct** outs) {
    NEED(c && a && outs);
    FHELIN_TRY
    if (c->lazy_rows && n > 1) {
        auto g = std::make_shared<LazyRows>();
        g->kind = LazyRows::UnwrapExpanded;
        g->src = ct_in(c, a);
        g->n = n;
        emit_lazy(c, g, n, outs);
    } else {
        emit(c, c->comp.unwrapExpanded(ct_in(c, a), n), outs);
    }
    FHELIN_CATCH
}
int fhelin_fc_unwrapScoresExpanded(fhelin_ctx* c, const fhelin_ct* a, int32_t n, fhelin_ct** outs) {
    NEED(c && a && outs);
    FHELIN_TRY
    emit(c, c->comp.unwrapScoresExpanded(ct_in(c, a), n), outs);
    FHELIN_CATCH
}
int fhelin_fc_unwrap_512_in_4_128(fhelin_ctx* c, const fhelin_ct* a, int32_t index, fhelin_ct** outs4) {
    NEED(c && a && outs4);
    FHELIN_TRY
    emit(c, c->comp.unwrap_512_in_4_128(ct_in(c, a), index), outs4);
    FHELIN_CATCH
}
int fhelin_fc_unwrapRepeatedLarge(fhelin_ctx* c, const fhelin_ct* const* containers, int32_t nc, int32_t input_number,
                                  fhelin_ct** outs) {
    NEED(c && containers && outs);
    FHELIN_TRY
    auto r = c->comp.unwrapRepeatedLarge(vec_of(c, containers, nc), input_number);
    for (size_t i = 0; i < r.size(); ++i) emit(c, r[i], outs + 4 * i);
    FHELIN_CATCH
}
int fhelin_fc_unwrapRepeatedLarge_range(fhelin_ctx* c, const fhelin_ct* const* containers, int32_t nc, int32_t input_number,
                                        int32_t first, int32_t count, fhelin_ct** outs) {
    NEED(c && containers && outs);
    FHELIN_TRY
    auto r = c->comp.unwrapRepeatedLarge(vec_of(c, containers, nc), input_number, first, count);
    for (size_t i = 0; i < r.size(); ++i) emit(c, r[i], outs + 4 * i);
    FHELIN_CATCH
}
int fhelin_fc_generate_containers(fhelin_ctx* c, const fhelin_ct* const* inputs, int32_t n, const fhelin_pt* bias,
                                  fhelin_ct** outs, int32_t* n_out) {
    NEED(c && inputs && outs);
    FHELIN_TRY
    CtVec r;
    if (const LazyRows* g0 = unread_relarge_rows(c, inputs, n)) {
        CtVec x;
        for (int i = 0; i < n; ++i) x.push_back(relarge_input(inputs[i]));
        r = c->comp.relarge_containers(x, g0->weights, g0->bias, g0->mask_val, opt(bias));
    } else {
        r = c->comp.generate_containers(vec_of(c, inputs, n), opt(bias));
    }
    emit(c, r, outs);
    if (n_out) *n_out = (int)r.size();
    FHELIN_CATCH
}
int fhelin_fc_wrap_containers(fhelin_ctx* c, const fhelin_ct* const* v, int32_t n, int32_t inputs_number, fhelin_ct** out) {
    NEED(c && v && out);
    FHELIN_TRY
    *out = wrap(c, c->comp.wrap_containers(vec_of(c, v, n), inputs_number));
    FHELIN_CATCH
}

/* ---- the composite calls on a BATCH OF SAMPLES (include/fhelin.h: fhelin_fcb_*) ---- */
static std::vector<CtVec> groups_of(fhelin_ctx* c, const fhelin_ct* const* v, int n, int B) {
    if (n < 0 || B < 0) throw Error(FHELIN_ERR_ARG, "negative count");
    const CtVec flat = vec_of(c, v, n * B);     // the deferred rows of ALL samples are evaluated together (force_many)
    std::vector<CtVec> g(B);
    for (int x = 0; x < B; ++x) g[x].assign(flat.begin() + (size_t)x * n, flat.begin() + (size_t)(x + 1) * n);
    return g;
}
int fhelin_fcb_matmulScores(fhelin_ctx* c, const fhelin_ct* const* queries, int32_t n, const fhelin_ct* const* keys, int32_t B, fhelin_ct** outs) {
    NEED(c && queries && keys && outs);
    FHELIN_TRY
    emit(c, c->comp.matmulScores_multi(groups_of(c, queries, n, B), vec_of(c, keys, B)), outs);
    FHELIN_CATCH
}
int fhelin_fcb_matmul_ct(fhelin_ctx* c, const fhelin_ct* const* rows, const fhelin_ct* const* ws, int32_t n, int32_t slots, int32_t padding,
                         fhelin_ct** outs) {
    NEED(c && rows && ws && outs && n >= 0);
    FHELIN_TRY
    emit(c, c->comp.matmul_ct_each(vec_of(c, rows, n), vec_of(c, ws, n), slots, padding), outs);
    FHELIN_CATCH
}
int fhelin_fcb_wrapUpRepeated(fhelin_ctx* c, const fhelin_ct* const* v, int32_t n, int32_t B, fhelin_ct** outs) {
    NEED(c && v && outs);
    FHELIN_TRY
    CtVec r;
    for (const CtVec& g : groups_of(c, v, n, B)) r.push_back(c->comp.wrapUpRepeated(g));   // one inner-product pass per sample fills the GPU
    emit(c, r, outs);
    FHELIN_CATCH
}
int fhelin_fcb_wrapUpExpanded(fhelin_ctx* c, const fhelin_ct* const* v, int32_t n, int32_t B, fhelin_ct** outs) {
    NEED(c && v && outs);
    FHELIN_TRY
    emit(c, c->comp.wrapUpExpanded_multi(groups_of(c, v, n, B)), outs);
    FHELIN_CATCH
}
int fhelin_fcb_unwrapExpanded(fhelin_ctx* c, const fhelin_ct* const* cs, int32_t B, int32_t n, fhelin_ct** outs) {
    NEED(c && cs && outs && B >= 0 && n >= 0);
    FHELIN_TRY
    if (c->lazy_rows && n > 1) {
        // one deferred group per sample, as B calls of fhelin_fc_unwrapExpanded make them: each keeps the read pattern of its own sample
        // (which rows, how many together - that decides the form), and groups read together are evaluated together (force_rows_multi)
        for (int x = 0; x < B; ++x) {
            if (!cs[x]) throw Error(FHELIN_ERR_ARG, "null ciphertext handle in array");
            auto g = std::make_shared<LazyRows>();
            g->kind = LazyRows::UnwrapExpanded;
            plan_inputs().clear();
            g->src = ct_in(c, cs[x]);
            g->n = n;
            emit_lazy(c, g, n, outs + (size_t)x * n);
        }
    } else {
        std::vector<int> all(n);
        for (int i = 0; i < n; ++i) all[i] = i;
        const std::vector<CtVec> r = c->comp.unwrapExpanded_rows_multi(vec_of(c, cs, B), n, all);
        for (int x = 0; x < B; ++x) emit(c, r[x], outs + (size_t)x * n);
    }
    FHELIN_CATCH
}
int fhelin_fcb_unwrapRepeatedLarge(fhelin_ctx* c, const fhelin_ct* const* containers, int32_t nc, int32_t B, int32_t input_number,
                                   fhelin_ct** outs) {
    NEED(c && containers && outs);
    FHELIN_TRY
    const auto r = c->comp.unwrapRepeatedLarge_multi(groups_of(c, containers, nc, B), input_number);
    for (int x = 0; x < B; ++x)
        for (size_t i = 0; i < r[x].size(); ++i) emit(c, r[x][i], outs + ((size_t)x * input_number + i) * 4);
    FHELIN_CATCH
}
int fhelin_fcb_generate_containers(fhelin_ctx* c, const fhelin_ct* const* inputs, int32_t n, int32_t B, const fhelin_pt* bias,
                                   fhelin_ct** outs, int32_t* n_out) {
    NEED(c && inputs && outs && n >= 0 && B >= 0);
    FHELIN_TRY
    std::vector<CtVec> r;
    if (const LazyRows* g0 = unread_relarge_rows(c, inputs, n * B)) {   // as fhelin_fc_generate_containers, per sample
        std::vector<CtVec> x(B);
        for (int i = 0; i < n * B; ++i) x[i / n].push_back(relarge_input(inputs[i]));
        r = c->comp.relarge_containers_multi(x, g0->weights, g0->bias, g0->mask_val, opt(bias));
    } else {
        r = c->comp.generate_containers_multi(groups_of(c, inputs, n, B), opt(bias));
    }
    const size_t per = r.empty() ? 0 : r[0].size();
    for (int x = 0; x < B; ++x) emit(c, r[x], outs + (size_t)x * per);
    if (n_out) *n_out = (int)per;
    FHELIN_CATCH
}
int fhelin_fc_rotsum_batch(fhelin_ctx* c, const fhelin_ct* const* v, int32_t n, int32_t slots, int32_t padding, int32_t repeat, fhelin_ct** outs) {
    NEED(c && v && outs && n >= 0);
    FHELIN_TRY
    emit(c, repeat ? c->comp.repeat_batch(vec_of(c, v, n), slots, padding) : c->comp.rotsum_batch(vec_of(c, v, n), slots, padding), outs);
    FHELIN_CATCH
}
int fhelin_add_plain_batch(fhelin_ctx* c, const fhelin_ct* const* v, int32_t n, const fhelin_pt* p, fhelin_ct** outs) {
    NEED(c && v && p && outs && n >= 0);
    FHELIN_TRY
    emit(c, c->ev.add_plain_batch(vec_of(c, v, n), p->p), outs);
    FHELIN_CATCH
}
int fhelin_eval_poly_batch(fhelin_ctx* c, const fhelin_ct* const* xs, int32_t n, const double* coeffs, int32_t n_coeffs, fhelin_ct** outs) {
    NEED(c && xs && coeffs && outs && n >= 0);
    FHELIN_TRY
    emit(c, c->ev.eval_poly_many(vec_of(c, xs, n), std::vector<double>(coeffs, coeffs + n_coeffs)), outs);
    FHELIN_CATCH
}
int fhelin_mult_many_batch(fhelin_ctx* c, const fhelin_ct* const* v, int32_t n, int32_t B, fhelin_ct** outs) {
    NEED(c && v && outs);
    FHELIN_TRY
    // handles that are the SAME object repeat as the same ciphertext (EvalMultMany({r, r, ...}) squares)
    emit(c, c->ev.mult_many_rows(groups_of(c, v, n, B)), outs);
    FHELIN_CATCH
}

int fhelin_mult_real(fhelin_ctx* c, const fhelin_ct* a, double k, fhelin_ct** out) {
    NEED(c && a && out);
    FHELIN_TRY
    *out = wrap(c, c->ev.mult_real(ct_in(c, a), k));
    FHELIN_CATCH
}
int fhelin_add_real(fhelin_ctx* c, const fhelin_ct* a, double k, fhelin_ct** out) {
    NEED(c && a && out);
    FHELIN_TRY
    *out = wrap(c, c->ev.add_real(ct_in(c, a), k));
    FHELIN_CATCH
}
int fhelin_mult_many(fhelin_ctx* c, const fhelin_ct* const* v, int32_t n, fhelin_ct** out) {
    NEED(c && v && out);
    FHELIN_TRY
    *out = wrap(c, c->ev.mult_many(vec_of(c, v, n)));
    FHELIN_CATCH
}
int fhelin_lincomb(fhelin_ctx* c, const fhelin_ct* const* v, const double* coeffs, int32_t n, double c0, fhelin_ct** out) {
    NEED(c && v && coeffs && out && n >= 1);
    FHELIN_TRY
    *out = wrap(c, c->ev.lincomb(vec_of(c, v, n), std::vector<double>(coeffs, coeffs + n), c0));
    FHELIN_CATCH
}
int fhelin_eval_poly(fhelin_ctx* c, const fhelin_ct* x, const double* coeffs, int32_t n, fhelin_ct** out) {
    NEED(c && x && coeffs && out);
    FHELIN_TRY
    const std::vector<double> cf(coeffs, coeffs + n);
    *out = wrap(c, run_heavy(c, x, [&](const CtPtr& in) { return c->ev.eval_poly(in, cf); }));
    FHELIN_CATCH
}
int fhelin_eval_chebyshev(fhelin_ctx* c, const fhelin_ct* x, const double* coeffs, int32_t n, double a, double b, fhelin_ct** out) {
    NEED(c && x && coeffs && out);
    FHELIN_TRY
    const std::vector<double> cf(coeffs, coeffs + n);
    if (n < 2) throw Error(FHELIN_ERR_ARG, "eval_chebyshev: need degree >= 1");
    if (defer_allowed(c)) {
        auto op = std::make_shared<LazyHeavy>();
        op->kind = LazyHeavy::Cheb;
        op->coeffs = cf;
        op->a = a;
        op->b = b;
        *out = defer_heavy(c, x, op);
    } else {
        *out = wrap(c, run_heavy(c, x, [&](const CtPtr& in) { return c->ev.eval_chebyshev(in, cf, a, b); }));
    }
    FHELIN_CATCH
}
int fhelin_eval_chebyshev_batch(fhelin_ctx* c, const fhelin_ct* const* xs, int32_t n, const double* coeffs, int32_t n_coeffs, double a,
                                double b, fhelin_ct** outs) {
    NEED(c && xs && coeffs && outs && n >= 0);
    FHELIN_TRY
    const std::vector<double> cf(coeffs, coeffs + n_coeffs);
    emit(c, c->ev.eval_chebyshev_many(vec_of(c, xs, n), cf, a, b), outs);
    FHELIN_CATCH
}
int fhelin_bootstrap_setup(fhelin_ctx* c, int32_t budget_enc, int32_t budget_dec, int32_t slots) {
    NEED(c);
    FHELIN_TRY
    c->boot.setup(budget_enc, budget_dec, slots);
    FHELIN_CATCH
}
int fhelin_bootstrap(fhelin_ctx* c, const fhelin_ct* a, fhelin_ct** out) {
    NEED(c && a && out);
    FHELIN_TRY
    const int drop = c->plan.next_drop(c->boot.out_ell());
    bootstrap_reads(c, a);
    if (defer_allowed(c)) {
        if (!c->boot.ready()) throw Error(FHELIN_ERR_STATE, "EvalBootstrapSetup has not been called");
        auto op = std::make_shared<LazyHeavy>();
        op->kind = LazyHeavy::Boot;
        op->drop = drop;
        *out = defer_heavy(c, a, op);
        return FHELIN_OK;
    }
    *out = emit_source(c, run_heavy(c, a, [&](const CtPtr& in) { return c->boot.bootstrap(in, drop); }));
    FHELIN_CATCH
}
int fhelin_bootstrap_batch(fhelin_ctx* c, const fhelin_ct* const* v, int32_t n, fhelin_ct** outs) {
    NEED(c && v && outs && n >= 0);
    FHELIN_TRY
    bootstrap_by_drop(c, v, n, outs, [&] { return c->plan.next_drop(c->boot.out_ell()); },
                      [&](const CtVec& sub, int drop) { return c->boot.bootstrap_batch(sub, drop); });
    FHELIN_CATCH
}
int fhelin_bootstrap_partial(fhelin_ctx* c, const fhelin_ct* a, int32_t stage, fhelin_ct** out) {
    NEED(c && a && out);
    FHELIN_TRY
    *out = wrap(c, c->boot.partial(ct_in(c, a), stage));
    FHELIN_CATCH
}
int fhelin_bootstrap_drop(fhelin_ctx* c, const fhelin_ct* a, int32_t drop, fhelin_ct** out) {
    NEED(c && a && out);
    FHELIN_TRY
    *out = wrap(c, c->boot.bootstrap(ct_in(c, a), drop));
    FHELIN_CATCH
}
// ---- paired bootstrapping (include/fhelin.h "Paired bootstrapping")
int fhelin_bootstrap_pair(fhelin_ctx* c, const fhelin_ct* a, const fhelin_ct* b, fhelin_ct** out_a, fhelin_ct** out_b) {
    NEED(c && a && b && out_a && out_b);
    FHELIN_TRY
    const CtPtr x = ct_in(c, a), y = ct_in(c, b);
    // two sources of the level plan, a's first; one pipeline serves both, so it raises to what the larger target asks for
    const int da = c->plan.next_drop(c->boot.out_ell()), db = c->plan.next_drop(c->boot.out_ell());
    bootstrap_reads(c, a);
    bootstrap_reads(c, b);
    const std::pair<CtPtr, CtPtr> o = c->boot.bootstrap_pair(x, y, std::min(da, db));
    fhelin_ct* outs[2];
    emit_sources(c, CtVec{o.first, o.second}, c->plan.next_ordinal - 2, outs);
    *out_a = outs[0];
    *out_b = outs[1];
    FHELIN_CATCH
}
int fhelin_bootstrap_paired_batch(fhelin_ctx* c, const fhelin_ct* const* v, int32_t n, fhelin_ct** outs) {
    NEED(c && v && outs && n >= 0);
    FHELIN_TRY
    // as fhelin_bootstrap_batch; those with the same planned drop share a pipeline and are paired inside it
    bootstrap_by_drop(c, v, n, outs, [&] { return c->plan.next_drop(c->boot.out_ell()); },
                      [&](const CtVec& sub, int drop) { return c->boot.bootstrap_pairs(sub, drop); });
    FHELIN_CATCH
}
int fhelin_bootstrap_pair_drop(fhelin_ctx* c, const fhelin_ct* a, const fhelin_ct* b, int32_t drop, fhelin_ct** out_a, fhelin_ct** out_b) {
    NEED(c && a && b && out_a && out_b);
    FHELIN_TRY
    const CtPtr x = ct_in(c, a), y = ct_in(c, b);
    const std::pair<CtPtr, CtPtr> o = c->boot.bootstrap_pair(x, y, drop);
    *out_a = wrap(c, o.first);
    *out_b = wrap(c, o.second);
    FHELIN_CATCH
}
int fhelin_bootstrap_pair_partial(fhelin_ctx* c, const fhelin_ct* a, const fhelin_ct* b, int32_t stage, fhelin_ct** out) {
    NEED(c && a && b && out);
    FHELIN_TRY
    const CtPtr x = ct_in(c, a), y = ct_in(c, b);
    *out = wrap(c, c->boot.pair_partial(x, y, stage));
    FHELIN_CATCH
}
static void check_precision(int32_t precision) {
    if (precision < 1 || precision > Bootstrapper::MAX_ITER_PRECISION)
        throw Error(FHELIN_ERR_ARG, "bootstrap_iter: precision must be in [1, 30]");
}
// the planned drop of the next iterative bootstrap: its full output has out_ell() - 1 limbs, and one bootstrap must keep three
static int iter_drop(fhelin_ctx* c) {
    return std::min(c->plan.next_drop(c->boot.out_ell() - 1), std::max(0, c->boot.out_ell() - 3));
}
int fhelin_bootstrap_iter(fhelin_ctx* c, const fhelin_ct* a, int32_t precision, fhelin_ct** out) {
    NEED(c && a && out);
    FHELIN_TRY
    check_precision(precision);
    // like fhelin_bootstrap: a terminal reading two limbs of its input and a source of the level plan, whose full output has one
    // limb fewer than a single bootstrap's
    const int drop = iter_drop(c);
    bootstrap_reads(c, a);
    if (defer_allowed(c)) {
        if (!c->boot.ready()) throw Error(FHELIN_ERR_STATE, "EvalBootstrapSetup has not been called");
        auto op = std::make_shared<LazyHeavy>();
        op->kind = LazyHeavy::Boot;
        op->drop = drop;
        op->precision = precision;
        if (c->boot.out_ell() - drop < 3)
            throw Error(FHELIN_ERR_STATE, "bootstrap_iter: the first bootstrap must leave at least three limbs (one for the final scaling)");
        *out = defer_heavy(c, a, op);
        return FHELIN_OK;
    }
    *out = emit_source(c, run_heavy(c, a, [&](const CtPtr& in) { return c->boot.bootstrap_iter(in, precision, drop); }));
    FHELIN_CATCH
}
int fhelin_bootstrap_iter_batch(fhelin_ctx* c, const fhelin_ct* const* v, int32_t n, int32_t precision, fhelin_ct** outs) {
    NEED(c && v && outs && n >= 0);
    FHELIN_TRY
    check_precision(precision);
    bootstrap_by_drop(c, v, n, outs, [&] { return iter_drop(c); },
                      [&](const CtVec& sub, int drop) { return c->boot.bootstrap_iter_batch(sub, precision, drop); });
    FHELIN_CATCH
}
int fhelin_bootstrap_iter_drop(fhelin_ctx* c, const fhelin_ct* a, int32_t precision, int32_t drop, fhelin_ct** out) {
    NEED(c && a && out);
    FHELIN_TRY
    check_precision(precision);
    *out = wrap(c, c->boot.bootstrap_iter(ct_in(c, a), precision, drop));
    FHELIN_CATCH
}
int fhelin_bootstrap_describe(fhelin_ctx* c, int32_t* out, int32_t cap, int32_t* n) {
    NEED(c && n && (out || cap == 0));
    FHELIN_TRY
    if (!c->boot.ready()) throw Error(FHELIN_ERR_STATE, "EvalBootstrapSetup has not been called");
    const Bootstrapper& b = c->boot;
    std::vector<int32_t> d = {b.packed() ? 1 : 0, b.slots(), b.K, b.R, b.cheb_degree, b.correction, b.depth(),
                              (int32_t)b.stages(false).size(), (int32_t)b.stages(true).size()};
    for (int which = 0; which < 2; ++which)
        for (const LinStage& st : b.stages(which != 0)) {
            d.push_back(st.terms.empty() ? 0 : st.terms[0].diag->slots);
            d.push_back((int32_t)st.terms.size());
            for (const auto& t : st.terms) {
                d.push_back(t.giant);
                d.push_back(t.baby);
            }
        }
    if (b.lt()) {   // the engine path's trailer (absent with the knob off): 1, the n1 asked for, (n1, n2) per stage, the encodings' bytes
        d.push_back(1);
        d.push_back(b.lt_n1());
        for (int which = 0; which < 2; ++which)
            for (const LinStage& st : b.stages(which != 0)) {
                d.push_back(st.bsz);
                d.push_back((int32_t)st.lt_giant.size());
            }
        const uint64_t bytes = b.lt_encoding_bytes();
        d.push_back((int32_t)(bytes & 0xffffffffu));
        d.push_back((int32_t)(bytes >> 32));
    }
    if (b.sparse_h()) {   // sparse-secret bootstrapping's trailer (absent with the knob off): 2, the Hamming weight of s~
        d.push_back(2);
        d.push_back(b.sparse_h());
    }
    *n = (int32_t)d.size();
    for (int i = 0; i < std::min(cap, *n); ++i) out[i] = d[i];
    FHELIN_CATCH
}
int fhelin_bootstrap_diag(fhelin_ctx* c, int32_t which, int32_t stage, int32_t term, fhelin_pt** out) {
    NEED(c && out);
    FHELIN_TRY
    if (!c->boot.ready()) throw Error(FHELIN_ERR_STATE, "EvalBootstrapSetup has not been called");
    const auto& sts = c->boot.stages(which != 0);
    if (which < 0 || which > 1 || stage < 0 || stage >= (int)sts.size() || term < 0 || term >= (int)sts[stage].terms.size())
        throw Error(FHELIN_ERR_ARG, "bootstrap_diag: no such term");
    auto* h = new fhelin_pt;
    h->p = sts[stage].terms[term].diag;
    *out = h;
    FHELIN_CATCH
}
int fhelin_bootstrap_cheb(fhelin_ctx* c, double* out, int32_t cap, int32_t* n) {
    NEED(c && n && (out || cap == 0));
    FHELIN_TRY
    if (!c->boot.ready()) throw Error(FHELIN_ERR_STATE, "EvalBootstrapSetup has not been called");
    const std::vector<double>& cf = c->boot.cheb();
    *n = (int32_t)cf.size();
    for (int i = 0; i < std::min(cap, *n); ++i) out[i] = cf[i];
    FHELIN_CATCH
}
int fhelin_bootstrap_config(fhelin_ctx* c, int32_t K, int32_t R, int32_t cheb_degree, int32_t correction) {
    NEED(c);
    FHELIN_TRY
    if (K < 1 || R < 0 || R > 8 || cheb_degree < 3 || cheb_degree > 255 || correction < 0 || correction > 20)
        throw Error(FHELIN_ERR_ARG, "bootstrap_config: parameter out of range");
    c->boot.K = K;
    c->boot.R = R;
    c->boot.cheb_degree = cheb_degree;
    c->boot.correction = correction;
    FHELIN_CATCH
}

}  // extern "C"
