// extern "C" boundary, linear transforms (include/fhelin.h "Linear transforms"): the plan object of a baby-step/giant-step matrix x
// ciphertext product and its application (Evaluator::linear_transform_rows).  A plan is host data - the split, the index lists and one
// plaintext handle per term; the device encodings are made by the plaintexts on first use.
#include "../../include/fhelin.h"
#include <algorithm>
#include <cmath>
#include <memory>
#include <set>
#include <vector>
#include "capi_internal.h"

using namespace fhelin;

#define NEED(x) if (!(x)) return capi_fail(FHELIN_ERR_ARG, "null argument")

struct fhelin_lt {
    int n1 = 0, n2 = 0, slots = 0, n_terms = 0;
    std::vector<int> baby, giant;                 // as given (fhelin_lt_create gives them reduced to [0, slots))
    std::vector<std::vector<PtPtr>> pts;          // [n2][n1], null = absent
};

namespace {
int mod_slots(long d, int slots) { return (int)(((d % slots) + slots) % slots); }

}  // namespace

extern "C" {

int fhelin_lt_create_pts(fhelin_ctx* c, const fhelin_pt* const* pts, const int32_t* baby, const int32_t* giant, int32_t n1, int32_t n2,
                         fhelin_lt** out) {
    NEED(c && pts && baby && giant && out);
    FHELIN_TRY
    if (n1 < 1 || n1 > LtDot::MAX_STEPS || n2 < 1) throw Error(FHELIN_ERR_ARG, "lt_create_pts: 1 <= n1 <= 32, n2 >= 1");
    if (c->ctx.stride != 1) throw Error(FHELIN_ERR_STATE, "lt_create_pts: interleaved samples (slot stride != 1) are not supported");
    const int slots = 1 << c->ctx.prm.log_slots;
    std::unique_ptr<fhelin_lt> lt(new fhelin_lt);
    lt->n1 = n1;
    lt->n2 = n2;
    lt->slots = slots;
    std::set<int> seen;
    for (int b = 0; b < n1; ++b) {
        lt->baby.push_back(baby[b]);
        if (b == 0 ? baby[0] != 0 : mod_slots(baby[b], slots) == 0) throw Error(FHELIN_ERR_ARG, "lt_create_pts: baby[0] is 0 and no other baby step is");
        if (!seen.insert(mod_slots(baby[b], slots)).second) throw Error(FHELIN_ERR_ARG, "lt_create_pts: duplicate baby step");
    }
    seen.clear();
    for (int g = 0; g < n2; ++g) {
        lt->giant.push_back(giant[g]);
        if (!seen.insert(mod_slots(giant[g], slots)).second) throw Error(FHELIN_ERR_ARG, "lt_create_pts: duplicate giant step");
    }
    lt->pts.assign(n2, std::vector<PtPtr>(n1));
    for (int g = 0; g < n2; ++g)
        for (int b = 0; b < n1; ++b)
            if (const fhelin_pt* p = pts[(size_t)g * n1 + b]) {
                if (p->p->slots != slots || p->p->stride != 1) throw Error(FHELIN_ERR_ARG, "lt_create_pts: a plaintext of another packing");
                lt->pts[g][b] = p->p;
                ++lt->n_terms;
            }
    if (lt->n_terms < 1) throw Error(FHELIN_ERR_ARG, "lt_create_pts: no term");
    *out = lt.release();
    FHELIN_CATCH
}

int fhelin_lt_create(fhelin_ctx* c, const double* diags, const int32_t* diag_idx, int32_t n_diag, int32_t slots, int32_t n1, fhelin_lt** out) {
    NEED(c && out && (n_diag < 1 || (diags && diag_idx)));
    FHELIN_TRY
    if (n_diag < 1) throw Error(FHELIN_ERR_ARG, "lt_create: at least one diagonal");
    if (slots != (1 << c->ctx.prm.log_slots)) throw Error(FHELIN_ERR_ARG, "lt_create: slots must be the context's packing");
    if (n1 < 0 || n1 > LtDot::MAX_STEPS) throw Error(FHELIN_ERR_ARG, "lt_create: 0 <= n1 <= 32");
    if (c->ctx.stride != 1) throw Error(FHELIN_ERR_STATE, "lt_create: interleaved samples (slot stride != 1) are not supported");
    std::vector<int> idx(n_diag);
    std::set<int> seen;
    for (int i = 0; i < n_diag; ++i) {
        idx[i] = mod_slots(diag_idx[i], slots);
        if (!seen.insert(idx[i]).second) throw Error(FHELIN_ERR_ARG, "lt_create: duplicate diagonal index");
    }
    if (n1 == 0) {
        n1 = 1;
        for (int k = 2; k <= LtDot::MAX_STEPS; ++k)
            if (Evaluator::lt_split_cost(idx, k) < Evaluator::lt_split_cost(idx, n1)) n1 = k;   // the planner's cost; ties go to the smaller n1
    }
    std::vector<int> giant;
    for (int d : seen)
        if (giant.empty() || giant.back() != d - d % n1) giant.push_back(d - d % n1);   // ascending: groups come out in order
    const int n2 = (int)giant.size();
    std::vector<int> baby(n1);
    for (int b = 0; b < n1; ++b) baby[b] = b;
    // V_{g,b} = rot(diag_{g+b}, -g): slot i holds diag[i - g].  Plaintexts of the plan's own, never handles of the content-keyed cache
    // (a matrix's diagonals would push a model's weights out of it); a NaN or an infinity is refused by the encoder (FHELIN_ERR_ARG)
    std::vector<std::unique_ptr<fhelin_pt>> hold;
    std::vector<const fhelin_pt*> pts((size_t)n2 * n1, nullptr);
    std::vector<double> v(slots);
    for (int i = 0; i < n_diag; ++i) {
        const int b = idx[i] % n1, g = idx[i] - b;
        const double* d = diags + (size_t)i * slots;
        for (int s = 0; s < slots; ++s) v[s] = d[mod_slots((long)s - g, slots)];
        hold.emplace_back(new fhelin_pt);
        hold.back()->p = c->cl.encode(v.data(), slots, 0, slots);
        pts[(size_t)(std::lower_bound(giant.begin(), giant.end(), g) - giant.begin()) * n1 + b] = hold.back().get();
    }
    const int rc = fhelin_lt_create_pts(c, pts.data(), baby.data(), giant.data(), n1, n2, out);
    if (rc != FHELIN_OK) return rc;
    FHELIN_CATCH
}

int fhelin_lt_info(const fhelin_lt* lt, int32_t* n1, int32_t* n2, int32_t* n_terms, int32_t* slots) {
    NEED(lt);
    if (n1) *n1 = lt->n1;
    if (n2) *n2 = lt->n2;
    if (n_terms) *n_terms = lt->n_terms;
    if (slots) *slots = lt->slots;
    return FHELIN_OK;
}

int fhelin_lt_rotations(const fhelin_lt* lt, int32_t* out, int32_t cap, int32_t* n) {
    NEED(lt && n && (out || cap <= 0));
    // the baby steps that carry a term and the rotated giant steps, each index once
    std::set<int> need;
    for (int b = 1; b < lt->n1; ++b)
        for (int g = 0; g < lt->n2; ++g)
            if (lt->pts[g][b]) need.insert(lt->baby[b]);
    for (int g : lt->giant)
        if (mod_slots(g, lt->slots)) need.insert(g);
    *n = (int32_t)need.size();
    int k = 0;
    for (int r : need)
        if (k < cap) out[k++] = r;
    return FHELIN_OK;
}

int fhelin_lt_apply(fhelin_ctx* c, const fhelin_lt* lt, const fhelin_ct* const* v, int32_t n, int32_t rescale, fhelin_ct** outs) {
    NEED(c && lt && n >= 0 && (n == 0 || (v && outs)));
    FHELIN_TRY
    c->ctx.require_device();
    if (c->ctx.stride != 1) throw Error(FHELIN_ERR_STATE, "lt_apply: interleaved samples (slot stride != 1) are not supported");
    if (lt->slots != (1 << c->ctx.prm.log_slots)) throw Error(FHELIN_ERR_ARG, "lt_apply: the plan was made for another packing");
    const CtVec in = vec_of(c, v, n);
    // no handle exists before the whole call has succeeded; nothing here makes a source of the level plan
    std::vector<CtPtr> r = c->ev.linear_transform_rows(in, lt->pts, lt->baby, lt->giant, rescale != 0);
    for (int i = 0; i < n; ++i) outs[i] = wrap(c, r[i]);
    FHELIN_CATCH
}

int fhelin_lt_encoding_bytes(const fhelin_lt* lt, uint64_t* bytes) {
    NEED(lt && bytes);
    uint64_t b = 0;
    for (const auto& row : lt->pts)
        for (const PtPtr& p : row)
            if (p) b += p->sliced_bytes();
    *bytes = b;
    return FHELIN_OK;
}

void fhelin_lt_free(fhelin_lt* lt) { delete lt; }

}  // extern "C"
