// extern "C" boundary, test-only part: the plaintext inner-product kernels (kernels_elem.h launch_ew_dot, launch_ew_dot_groups,
// launch_ew_cyclic_dot, launch_ew_window_dot) and the two kernels of a paired bootstrap (launch_ew_pair_pack, launch_ew_pair_split) reached
// directly, with operands the caller chooses residue by residue.  Thin forwards to the Evaluator / Bootstrapper methods as they stand:
// nothing here is on a driver's path.
#include "../../include/fhelin.h"
#include <hip/hip_runtime.h>
#include <algorithm>
#include <vector>
#include "capi_internal.h"

using namespace fhelin;

#define NEED(x) if (!(x)) return capi_fail(FHELIN_ERR_ARG, "null argument")

namespace {
std::vector<CtPtr> cts_in(fhelin_ctx* c, const fhelin_ct* const* v, int n, bool nullable = false) {
    std::vector<CtPtr> in(n);
    for (int i = 0; i < n; ++i) {
        if (!v[i]) {
            if (!nullable) throw Error(FHELIN_ERR_ARG, "null ciphertext in array");
            continue;
        }
        const CtPtr& p = ct_in(c, v[i]);
        if (p->npoly != 2 || p->deg != 1) throw Error(FHELIN_ERR_ARG, "debug_dot: operands are degree-1 ciphertexts of two components");
        in[i] = p;
    }
    return in;
}
std::vector<PtPtr> pts_in(const fhelin_pt* const* v, int n, bool nullable = false) {
    std::vector<PtPtr> in(n);
    for (int i = 0; i < n; ++i) {
        if (!v[i] && !nullable) throw Error(FHELIN_ERR_ARG, "null plaintext in array");
        if (v[i]) in[i] = v[i]->p;
    }
    return in;
}
// a plaintext whose one encoding is residues [ell][N] at `scale`; ell = L + 1 + K: over the full key basis (limb ids 0 .. L + K)
fhelin_pt* pt_from_residues(Context& x, const uint64_t* residues, int ell, long double scale) {
    const size_t N = x.N;
    for (int l = 0; l < ell; ++l)
        for (size_t n = 0; n < N; ++n)
            if (residues[(size_t)l * N + n] >= x.moduli[l]) throw Error(FHELIN_ERR_ARG, "pt_from_residues: a residue is not below its limb's modulus");
    auto e = std::make_shared<Encoding>();
    e->ctx = &x;
    e->ell = ell;
    e->scale = scale;
    e->d = x.dalloc<u64>((size_t)ell * N);
    hip_check(hipMemcpyAsync(e->d, residues, (size_t)ell * N * 8, hipMemcpyHostToDevice, x.stream), "pt import");
    e->made_lane = x.pool.cur_lane;
    e->lanes_ordered = 1u << e->made_lane;
    if (x.n_lanes > 0) {
        hip_check(hipEventCreateWithFlags(&e->ready, hipEventDisableTiming), "hipEventCreate(encoding)");
        hip_check(hipEventRecord(e->ready, x.stream), "hipEventRecord(encoding)");
    }
    x.sync();
    // a plaintext of its own, never a handle of the content-keyed cache (PtCache): no values to key it by, nothing shared
    auto p = std::make_shared<Plaintext>();
    p->ctx = &x;
    p->slots = 1 << x.prm.log_slots;
    p->level = std::max(0, x.L + 1 - ell);
    p->fixed = true;
    p->cache.push_back(e);
    auto* h = new fhelin_pt;
    h->p = p;
    return h;
}
}  // namespace

extern "C" {

int fhelin_debug_pt_from_residues(fhelin_ctx* c, const uint64_t* residues, int32_t ell, fhelin_pt** out) {
    NEED(c && residues && out);
    FHELIN_TRY
    Context& x = c->ctx;
    x.require_device();
    if (ell < 1 || ell > x.L + 1) throw Error(FHELIN_ERR_ARG, "pt_from_residues: bad limb count");
    *out = pt_from_residues(x, residues, ell, x.sf_real[x.L + 1 - ell]);   // the scale dot_plain* asks for at this limb count
    FHELIN_CATCH
}

int fhelin_debug_pt_from_residues_full(fhelin_ctx* c, const uint64_t* residues, double scale_hi, double scale_lo, fhelin_pt** out) {
    NEED(c && residues && out);
    FHELIN_TRY
    Context& x = c->ctx;
    x.require_device();
    if (!(scale_hi > 0)) throw Error(FHELIN_ERR_ARG, "pt_from_residues_full: the full-basis encoding needs an explicit scale");
    *out = pt_from_residues(x, residues, x.L + 1 + x.K, (long double)scale_hi + (long double)scale_lo);
    FHELIN_CATCH
}

int fhelin_debug_dot_plain(fhelin_ctx* c, const fhelin_ct* const* cts, const fhelin_pt* const* pts, int32_t n, fhelin_ct** out) {
    NEED(c && cts && pts && out);
    FHELIN_TRY
    if (n < 1) throw Error(FHELIN_ERR_ARG, "debug_dot_plain: at least one term");
    *out = wrap(c, c->ev.dot_plain(cts_in(c, cts, n), pts_in(pts, n)));
    FHELIN_CATCH
}

int fhelin_debug_dot_groups(fhelin_ctx* c, const fhelin_ct* const* cts, int32_t nb, int32_t na, const fhelin_pt* const* pts, int32_t ng,
                            fhelin_ct** outs) {
    NEED(c && cts && pts && outs);
    FHELIN_TRY
    if (nb < 1 || na < 1 || na > EwDotGroups::MAX_A || ng < 1 || ng > EwDotGroups::MAX_G)
        throw Error(FHELIN_ERR_ARG, "debug_dot_groups: 1 <= na <= 16, 1 <= ng <= 8, nb >= 1");
    std::vector<CtPtr> flat = cts_in(c, cts, nb * na);
    std::vector<std::vector<PtPtr>> p(ng);
    for (int g = 0; g < ng; ++g) p[g] = pts_in(pts + (size_t)g * na, na, true);
    const CtPtr& f = flat[0];
    for (const CtPtr& x : flat)
        if (x->ell != f->ell) throw Error(FHELIN_ERR_ARG, "debug_dot_groups: operands of one limb count");
    std::vector<CtPtr> dest = c->ev.new_ct_batch(nb * ng, 2, f->ell, f->deg + 1, f->scale, f->slots);
    bool ok;
    if (nb == 1) {
        ok = c->ev.dot_plain_groups(flat, p, 0, dest);
    } else {
        // batch element x, column b at x * na + b of one block: every column equally spaced over the batch, and so is every output
        flat = c->ev.make_contiguous(flat);
        std::vector<std::vector<CtPtr>> in(nb), o(nb);
        for (int x = 0; x < nb; ++x) {
            in[x].assign(flat.begin() + (size_t)x * na, flat.begin() + (size_t)(x + 1) * na);
            o[x].assign(dest.begin() + (size_t)x * ng, dest.begin() + (size_t)(x + 1) * ng);
        }
        ok = c->ev.dot_plain_groups_batch(in, p, 0, o);
    }
    if (!ok) throw Error(FHELIN_ERR_STATE, "debug_dot_groups: the evaluator refused the operands (no fall-back here)");
    for (int i = 0; i < nb * ng; ++i) outs[i] = wrap(c, dest[i]);
    FHELIN_CATCH
}

int fhelin_debug_dot_cyclic(fhelin_ctx* c, const fhelin_ct* const* cts, int32_t n, const fhelin_pt* const* pts, fhelin_ct** outs) {
    NEED(c && cts && pts && outs);
    FHELIN_TRY
    constexpr int P = EwCyclic::PERIOD;
    if (n < 1 || n > P) throw Error(FHELIN_ERR_ARG, "debug_dot_cyclic: 1 <= n <= 32");
    std::vector<CtPtr> in = cts_in(c, cts, n);
    std::vector<CtPtr> dest = c->ev.new_ct_batch(P, 2, in[0]->ell, in[0]->deg + 1, in[0]->scale, in[0]->slots);
    if (!c->ev.dot_plain_cyclic(in, pts_in(pts, P), dest))
        throw Error(FHELIN_ERR_STATE, "debug_dot_cyclic: the evaluator refused the operands (no fall-back here)");
    for (int k = 0; k < P; ++k) outs[k] = wrap(c, dest[k]);
    FHELIN_CATCH
}

int fhelin_debug_dot_window(fhelin_ctx* c, const fhelin_ct* const* cur, const fhelin_ct* const* prev, const fhelin_pt* const* pts,
                            fhelin_ct* const* dest, int32_t accumulate) {
    NEED(c && cur && prev && pts && dest);
    FHELIN_TRY
    constexpr int W = EwWindow::W;
    std::vector<CtPtr> d(W);
    for (int t = 0; t < W; ++t) {
        if (!dest[t]) throw Error(FHELIN_ERR_ARG, "null ciphertext in array");
        d[t] = ct_in(c, dest[t]);   // in/out: the kernel writes into the handle's own residues
    }
    if (!c->ev.dot_plain_window(cts_in(c, cur, W, true), cts_in(c, prev, W, true), pts_in(pts, W), d, accumulate != 0))
        throw Error(FHELIN_ERR_STATE, "debug_dot_window: the evaluator refused the operands (no fall-back here)");
    FHELIN_CATCH
}

int fhelin_debug_rotate_many_batch(fhelin_ctx* c, const fhelin_ct* const* cts, int32_t n_ct, const int32_t* indices, int32_t n,
                                   fhelin_ct** outs) {
    NEED(c && cts && indices && outs);
    FHELIN_TRY
    if (n_ct < 1 || n < 1) throw Error(FHELIN_ERR_ARG, "debug_rotate_many_batch: at least one ciphertext and one index");
    std::vector<CtPtr> in(n_ct);
    for (int i = 0; i < n_ct; ++i) {
        if (!cts[i]) throw Error(FHELIN_ERR_ARG, "null ciphertext in array");
        in[i] = ct_in(c, cts[i]);
    }
    const std::vector<std::vector<CtPtr>> o = c->ev.rotate_many_batch(in, std::vector<int>(indices, indices + n));
    for (int i = 0; i < n_ct; ++i)
        for (int k = 0; k < n; ++k) outs[(size_t)i * n + k] = wrap(c, o[i][k]);
    FHELIN_CATCH
}

int fhelin_debug_ks_accp(fhelin_ctx* c, const uint64_t* digits, int32_t ell, int32_t batch, const int32_t* indices, int32_t n_rot,
                         uint64_t* out) {
    NEED(c && digits && out && (indices || n_rot == 0));
    FHELIN_TRY
    Context& x = c->ctx;
    x.require_device();
    if (ell < 1 || ell > x.L + 1 || batch < 1) throw Error(FHELIN_ERR_ARG, "debug_ks_accp: bad shape");
    const size_t N = x.N;
    const size_t nd = (size_t)batch * x.lvl[ell].beta * (ell + x.K) * N, no = (size_t)batch * 2 * x.K * N;
    for (size_t i = 0; i < nd; ++i)
        if (digits[i] >> 60) throw Error(FHELIN_ERR_ARG, "debug_ks_accp: a digit is not below 2^60");
    Scratch<u64> ext = x.scratch<u64>(nd);
    hip_check(hipMemcpyAsync(ext, digits, nd * 8, hipMemcpyHostToDevice, x.stream), "debug_ks_accp upload");
    Scratch<u64> acc = c->ev.debug_ks_accp(ext, ell, batch, indices, n_rot);
    hip_check(hipMemcpyAsync(out, acc, no * 8, hipMemcpyDeviceToHost, x.stream), "debug_ks_accp download");
    x.sync();
    FHELIN_CATCH
}

int fhelin_debug_ks_accq(fhelin_ctx* c, const uint64_t* digits, const uint64_t* own, const uint64_t* conv, int32_t ell, int32_t batch,
                         int32_t index, uint64_t* out) {
    NEED(c && digits && own && conv && out);
    FHELIN_TRY
    Context& x = c->ctx;
    x.require_device();
    if (ell < 1 || ell > x.L + 1 || batch < 1) throw Error(FHELIN_ERR_ARG, "debug_ks_accq: bad shape");
    const size_t N = x.N;
    const size_t nd = (size_t)batch * x.lvl[ell].beta * (ell + x.K) * N, nw = (size_t)batch * ell * N, no = 2 * nw;
    for (size_t i = 0; i < nd; ++i)
        if (digits[i] >> 60) throw Error(FHELIN_ERR_ARG, "debug_ks_accq: a digit is not below 2^60");
    for (size_t i = 0; i < no; ++i)
        if (conv[i] >= x.moduli[(i / N) % ell]) throw Error(FHELIN_ERR_ARG, "debug_ks_accq: conv is not canonical");
    for (size_t i = 0; i < nw; ++i)
        if (own[i] >= x.moduli[(i / N) % ell]) throw Error(FHELIN_ERR_ARG, "debug_ks_accq: the own limb is not canonical");
    Scratch<u64> ext = x.scratch<u64>(nd);
    Scratch<u64> down = x.scratch<u64>(nw);
    Scratch<u64> dconv = x.scratch<u64>(no);
    Scratch<u64> res = x.scratch<u64>(no);
    hip_check(hipMemcpyAsync(ext, digits, nd * 8, hipMemcpyHostToDevice, x.stream), "debug_ks_accq upload");
    hip_check(hipMemcpyAsync(down, own, nw * 8, hipMemcpyHostToDevice, x.stream), "debug_ks_accq upload");
    hip_check(hipMemcpyAsync(dconv, conv, no * 8, hipMemcpyHostToDevice, x.stream), "debug_ks_accq upload");
    c->ev.debug_ks_accq(ext, down, dconv, ell, batch, index, res);
    hip_check(hipMemcpyAsync(out, res, no * 8, hipMemcpyDeviceToHost, x.stream), "debug_ks_accq download");
    x.sync();
    FHELIN_CATCH
}

int fhelin_debug_pair_pack(fhelin_ctx* c, const fhelin_ct* const* a, const fhelin_ct* const* b, const uint64_t* k0_a, const uint64_t* k0_b,
                           int32_t n, fhelin_ct** outs) {
    NEED(c && a && b && k0_a && k0_b && outs);
    FHELIN_TRY
    c->ctx.require_device();
    if (n < 1 || n > EwPairPack::MAX_PAIRS) throw Error(FHELIN_ERR_ARG, "debug_pair_pack: 1 to 32 pairs");
    std::vector<CtPtr> va(n), vb(n);
    for (int i = 0; i < n; ++i) {
        if (!a[i] || !b[i]) throw Error(FHELIN_ERR_ARG, "null ciphertext in array");
        va[i] = ct_in(c, a[i]);
        vb[i] = ct_in(c, b[i]);
    }
    const std::vector<CtPtr> o = c->boot.pack_pairs(va, vb, std::vector<u64>(k0_a, k0_a + n), std::vector<u64>(k0_b, k0_b + n));
    for (int i = 0; i < n; ++i) outs[i] = wrap(c, o[i]);
    FHELIN_CATCH
}

int fhelin_debug_pair_split(fhelin_ctx* c, const fhelin_ct* const* w, const fhelin_ct* const* wc, int32_t n, fhelin_ct** out_a,
                            fhelin_ct** out_b) {
    NEED(c && w && wc && out_a && out_b);
    FHELIN_TRY
    c->ctx.require_device();
    if (n < 1 || n > EwPairSplit::MAX_PAIRS) throw Error(FHELIN_ERR_ARG, "debug_pair_split: 1 to 32 pairs");
    std::vector<CtPtr> vw(n), vc(n), oa, ob;
    for (int i = 0; i < n; ++i) {
        if (!w[i] || !wc[i]) throw Error(FHELIN_ERR_ARG, "null ciphertext in array");
        vw[i] = ct_in(c, w[i]);
        vc[i] = ct_in(c, wc[i]);
    }
    c->boot.split_pairs(vw, vc, oa, ob);
    for (int i = 0; i < n; ++i) {
        out_a[i] = wrap(c, oa[i]);
        out_b[i] = wrap(c, ob[i]);
    }
    FHELIN_CATCH
}

}  // extern "C"
