#include "bootstrap.h"
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <numeric>
#include <set>

namespace fhelin {

namespace {

const double PI = 3.14159265358979323846264338327950288;

void add_diag(DiagMap& m, int r, int n, int pos, cplx v) {
    r = ((r % n) + n) % n;
    auto& d = m[r];
    if (d.empty()) d.assign(n, cplx(0, 0));
    d[pos] += v;
}

// one radix-2 stage of the special FFT as a 3-diagonal map (see ckks_fft_special in client.cpp)
DiagMap stage_map(int n, int len, bool inverse, const std::vector<u32>& rot, const std::vector<std::pair<double, double>>& ksi) {
    DiagMap m;
    const int lenh = len >> 1, lenq = len << 2, gap = (4 * n) / lenq;
    for (int p = 0; p < n; ++p) {
        const int jj = p % len;
        if (inverse) {
            if (jj < lenh) {
                add_diag(m, 0, n, p, 1.0);
                add_diag(m, lenh, n, p, 1.0);
            } else {
                const int j = jj - lenh;
                const auto& k = ksi[(lenq - (rot[j] % lenq)) * gap];
                const cplx w(k.first, k.second);
                add_diag(m, -lenh, n, p, w);
                add_diag(m, 0, n, p, -w);
            }
        } else {
            if (jj < lenh) {
                const auto& k = ksi[(rot[jj] % lenq) * gap];
                add_diag(m, 0, n, p, 1.0);
                add_diag(m, lenh, n, p, cplx(k.first, k.second));
            } else {
                const int j = jj - lenh;
                const auto& k = ksi[(rot[j] % lenq) * gap];
                add_diag(m, -lenh, n, p, 1.0);
                add_diag(m, 0, n, p, -cplx(k.first, k.second));
            }
        }
    }
    return m;
}

// (B after A): out = sum_s e_s * rot_s( sum_r d_r * rot_r(x) ) = sum_{r,s} e_s * rot_s(d_r) * rot_{r+s}(x)
DiagMap compose(const DiagMap& B, const DiagMap& A, int n) {
    DiagMap C;
    for (const auto& be : B)
        for (const auto& ae : A) {
            const int s = be.first, r = ae.first;
            auto& c = C[(r + s) % n];
            if (c.empty()) c.assign(n, cplx(0, 0));
            for (int j = 0; j < n; ++j) c[j] += be.second[j] * ae.second[(j + s) % n];
        }
    // drop numerically empty diagonals
    for (auto it = C.begin(); it != C.end();) {
        double mx = 0;
        for (const auto& v : it->second) mx = std::max(mx, std::abs(v));
        if (mx < 1e-300) it = C.erase(it);
        else ++it;
    }
    return C;
}

// Sparse packing (2 slots <= N/2): a ciphertext with n slots has room for 2n.  The LAST CoeffsToSlots stage written over 2n
// slots with the diagonals [d_r | -i d_r] leaves w on the left half and -i w on the right one, so that after adding the
// conjugate the left half holds the real parts (t_k) and the right half the imaginary parts (t_{k+n}): ONE ciphertext goes
// through the modular reduction instead of two.
DiagMap pack_last_c2s(const DiagMap& m, int n) {
    DiagMap out;
    for (const auto& e : m) {
        std::vector<cplx> d(2 * n);
        for (int j = 0; j < n; ++j) {
            d[j] = e.second[j];
            d[j + n] = cplx(0, -1) * e.second[j];
        }
        out[e.first] = d;
    }
    return out;
}
// ... and the FIRST SlotsToCoeffs stage takes u = [L | R] (2n real slots) in place of the n-slot vector z = L + i R it is
// defined on: out_j = sum_r e_r[j mod n] z_{(j + r) mod n} for all 2n positions j (the result has period n again), with
// z_q = u_q + i u_{q+n}: every diagonal r becomes two, at offsets r and r + n of the 2n-slot rotation group.
DiagMap unpack_first_s2c(const DiagMap& m, int n) {
    DiagMap out;
    for (const auto& e : m) {
        const int r = ((e.first % n) + n) % n;
        std::vector<cplx> a(2 * n), b(2 * n);
        for (int j = 0; j < 2 * n; ++j) {
            const int jj = j % n;
            const bool wraps = jj + r >= n;             // (jj + r) mod n came around: the halves of u trade places
            const bool left = (j < n) != wraps;         // rot_r(u)_j is the L entry (else rot_{r+n}(u)_j is)
            const cplx v = e.second[jj];
            a[j] = left ? v : cplx(0, 1) * v;           // coefficient of rot_r(u)_j
            b[j] = left ? cplx(0, 1) * v : v;           // coefficient of rot_{r+n}(u)_j
        }
        out[r] = a;
        out[r + n] = b;
    }
    return out;
}

void scale_map(DiagMap& m, double f) {
    for (auto& e : m)
        for (auto& v : e.second) v *= f;
}

}  // namespace

Bootstrapper::~Bootstrapper() {
    if (mono_i_) {
        try { ev_.ctx().pool.free(mono_i_); } catch (...) {}
    }
}

void Bootstrapper::set_lt(bool on, int n1) {
    if (n1 < 0 || n1 > LtDot::MAX_STEPS) throw Error(FHELIN_ERR_ARG, "bootstrap_lt: n1 is 0 (the planner chooses) or 1..32");
    if (ready()) throw Error(FHELIN_ERR_STATE, "bootstrap_lt: the split binds at bootstrap_setup - set the knob before it");
    lt_ = on;
    lt_n1_ = n1;
}

void Bootstrapper::set_sparse(int hamming) {
    if (hamming != 0 && (hamming < 8 || hamming > ev_.ctx().N)) throw Error(FHELIN_ERR_ARG, "bootstrap_sparse_secret: the Hamming weight is 0 (off) or 8 .. N");
    if (ready()) throw Error(FHELIN_ERR_STATE, "bootstrap_sparse_secret: the ephemeral secret and its keys are made by bootstrap_setup - set the knob before it");
    if (hamming == 0) {
        if (sparse_h_) {   // back to the default approximation
            K = 28;
            R = 3;
            cheb_degree = 47;
        }
        sparse_h_ = 0;
        return;
    }
    sparse_h_ = hamming;
    // |I| has standard deviation sqrt((h + 1) / 12): the default's K = 28 at h = 192 is 7.0 sigma, and K keeps that ratio
    K = (int)std::ceil(28.0 * std::sqrt((hamming + 1) / 193.0) - 1e-12);
    R = 3;
    cheb_degree = K <= SPARSE_MAX_K ? SPARSE_CHEB_DEGREE : 47;
}

size_t Bootstrapper::lt_encoding_bytes() const {
    size_t b = 0;
    for (const auto* v : {&c2s_, &s2c_})
        for (const auto& st : *v)
            for (const auto& t : st.terms) b += t.diag->sliced_bytes();
    return b;
}

LinStage Bootstrapper::prepare(const DiagMap& m, int n) {
    LinStage st;
    int g = n;
    for (const auto& e : m)
        if (e.first) g = std::gcd(g, e.first);
    st.g0 = g;
    const int span = n / g;  // number of possible multiples
    const int count = (int)m.size();
    int bsz = 1;
    while (bsz * bsz < count) bsz <<= 1;
    st.bsz = std::min(bsz, span);
    if (lt_) {   // the engine's split: at most LtDot::MAX_STEPS baby steps, forced or by the linear-transform planner's cost
        const int cap = std::min((int)LtDot::MAX_STEPS, span);
        std::vector<int> ks;
        for (const auto& e : m) ks.push_back(e.first / g);
        int n1 = std::min(lt_n1_, cap);
        if (lt_n1_ == 0) {
            n1 = 1;
            for (int k = 2; k <= cap; ++k)
                if (Evaluator::lt_split_cost(ks, k) < Evaluator::lt_split_cost(ks, n1)) n1 = k;   // ties go to the smaller n1 (fewer keys)
        }
        st.bsz = n1;
    }
    for (const auto& e : m) {
        const int k = e.first / g;
        const int G = k / st.bsz, B = k % st.bsz;
        const int sG = G * st.bsz * g;
        auto p = std::make_shared<Plaintext>();
        p->ctx = &ev_.ctx();
        p->slots = n;
        p->level = 0;
        p->values.resize(n);
        p->imag.resize(n);
        for (int j = 0; j < n; ++j) {
            const cplx v = e.second[((j - sG) % n + n) % n];  // rot_{-sG}(d)
            p->values[j] = v.real();
            p->imag[j] = v.imag();
        }
        st.terms.push_back({sG, B * g, p});
    }
    if (lt_) {
        for (int b = 0; b < st.bsz; ++b) st.lt_baby.push_back(b * g);
        for (const auto& t : st.terms)   // the map runs in ascending index order: so do the giant steps
            if (st.lt_giant.empty() || st.lt_giant.back() != t.giant) st.lt_giant.push_back(t.giant);
        st.lt_pts.assign(st.lt_giant.size(), std::vector<PtPtr>(st.bsz));
        for (const auto& t : st.terms)
            st.lt_pts[std::lower_bound(st.lt_giant.begin(), st.lt_giant.end(), t.giant) - st.lt_giant.begin()][t.baby / g] = t.diag;
    }
    return st;
}

// Interleaved samples (context.h Context::stride): `slots` is logical; the stages, their diagonals and every rotation of the bootstrap
// (baby and giant steps, SubSum, conjugation) belong to the PHYSICAL packing of slots * stride slots, so the public entry points run
// under a Context::PhysicalScope and nothing below multiplies an index by the stride.
void Bootstrapper::setup(int budget_enc, int budget_dec, int slots) {
    Context& c = ev_.ctx();
    c.require_device();
    if (slots <= 0) slots = 1 << c.prm.log_slots;
    const int logical = slots;
    if (c.stride > 1) {
        if ((long)slots * c.stride > c.N / 2) throw Error(FHELIN_ERR_ARG, "bootstrap: slots x interleave stride must be <= N/2");
        slots *= c.stride;
    }
    c.stride_locked = true;
    Context::PhysicalScope physical(c);
    // an evaluation context (no secret) builds its stages from the imported keys: a missing one is named below (FHELIN_ERR_KEY)
    if (!cl_.has_keys() && !cl_.eval_only()) throw Error(FHELIN_ERR_KEY, "bootstrap setup needs the secret key (keygen first)");
    if (slots <= 0) slots = 1 << c.prm.log_slots;
    if (slots & (slots - 1) || slots > c.N / 2 || slots < 4) throw Error(FHELIN_ERR_ARG, "bootstrap: slots must be a power of two in [4, N/2]");
    if (budget_enc < 1 || budget_dec < 1) throw Error(FHELIN_ERR_ARG, "bootstrap: level budget must be >= 1");
    // sparse-secret encapsulation: s~, the to-sparse and the from-sparse key, in front of every other draw of this call
    if (sparse_h_) cl_.gen_sparse_keys(sparse_h_);
    slots_ = slots;
    logical_slots_ = logical;
    budget_enc_ = budget_enc;
    budget_dec_ = budget_dec;
    const int n = slots;
    int logn = 0;
    while ((1 << logn) < n) ++logn;
    budget_enc = std::min(budget_enc, logn);
    budget_dec = std::min(budget_dec, logn);
    std::vector<u32> rot;
    std::vector<std::pair<double, double>> ksi;
    ckks_fft_tables(n, rot, ksi);

    const int gapN = (c.N / 2) / n;
    packed_ = gapN >= 2;
    if (const char* e = std::getenv("FHELIN_BOOT_PACKED")) packed_ = packed_ && std::atoi(e) != 0;
    if (const char* e = std::getenv("FHELIN_BOOT_STAGES_LEGACY")) stage_order_legacy_ = std::atoi(e) != 0;
    const double q0 = (double)c.chain.q[0];
    // CoeffsToSlots: inverse-FFT stages (len = n .. 2), total constant Delta_r / (gapN q0 K 2n) spread over the levels
    auto build = [&](bool inverse, int budget, double total_factor, std::vector<LinStage>& out) {
        std::vector<int> lens;
        if (inverse) for (int len = n; len >= 2; len >>= 1) lens.push_back(len);
        else for (int len = 2; len <= n; len <<= 1) lens.push_back(len);
        const double f = std::pow(total_factor, 1.0 / budget);
        size_t pos = 0;
        for (int g = 0; g < budget; ++g) {
            // radix levels per stage: the remainder goes to the LATER stages.  The first CoeffsToSlots stage runs at the top of
            // the chain (the dearest key switches) and the first SlotsToCoeffs stage has its diagonals doubled under sparse
            // packing: both should be the small ones (14 levels, budget 3: 4 + 5 + 5 rather than 5 + 5 + 4)
            int cnt = logn / budget + (budget - 1 - g < logn % budget ? 1 : 0);
            if (stage_order_legacy_) cnt = logn / budget + (g < logn % budget ? 1 : 0);
            DiagMap m = stage_map(n, lens[pos], inverse, rot, ksi);
            for (int i = 1; i < cnt; ++i) m = compose(stage_map(n, lens[pos + i], inverse, rot, ksi), m, n);
            pos += cnt;
            scale_map(m, f);
            if (packed_ && inverse && g == budget - 1) out.push_back(prepare(pack_last_c2s(m, n), 2 * n));
            else if (packed_ && !inverse && g == 0) out.push_back(prepare(unpack_first_s2c(m, n), 2 * n));
            else out.push_back(prepare(m, n));
        }
    };
    c2s_.clear();
    s2c_.clear();
    const double delta_r = (double)c.sf_real[0];
    build(true, budget_enc, delta_r / ((double)gapN * q0 * K * 2.0 * n), c2s_);
    build(false, budget_dec, 1.0 / (2.0 * PI), s2c_);

    // rotation keys: baby/giant shifts of every stage, SubSum shifts, conjugation
    std::set<int> idx;
    for (const auto* v : {&c2s_, &s2c_})
        for (const auto& st : *v)
            for (const auto& t : st.terms) {
                if (t.giant) idx.insert(t.giant);
                if (t.baby) idx.insert(t.baby);
            }
    for (int r : idx) cl_.gen_rotation_key(r);
    for (int j = 1; j < gapN; j <<= 1) cl_.gen_rotation_key(n * j);
    if (!ev_.conj_key) cl_.gen_conj_key();

    // cosine fit: f(y) = cos((2 pi K y - pi/2) / 2^R) on [-1,1]; R double-angle steps give sin(2 pi K y).  The interpolant at the
    // d + 1 Chebyshev nodes; under a sparse ephemeral secret the series itself, truncated at d, from twice the nodes: the degree that
    // fits five levels is 28, where aliasing costs the interpolant a third of its accuracy (1.8e-12 against 1.2e-12)
    const int d = cheb_degree, nn = sparse_h_ ? 2 * (d + 1) : d + 1;
    cheb_.assign(d + 1, 0.0);
    std::vector<double> fx(nn);
    const double sc = 1.0 / (double)(1 << R);
    for (int j = 0; j < nn; ++j) fx[j] = std::cos((2.0 * PI * K * std::cos(PI * (j + 0.5) / nn) - PI / 2) * sc);
    for (int k = 0; k <= d; ++k) {
        double s = 0;
        for (int j = 0; j < nn; ++j) s += fx[j] * std::cos(PI * k * (j + 0.5) / nn);
        cheb_[k] = 2.0 * s / nn;
    }

    ensure_mono_i();
    depth_ = budget_enc + budget_dec + R + Evaluator::cheb_depth(cheb_degree);
}

// multiplication by i == multiplication by the monomial X^{N/2}.  Depends on the ring alone: made once, by setup() or by the first use of
// the pair kernels on their own (pack_pairs / split_pairs need no keys)
void Bootstrapper::ensure_mono_i() {
    if (mono_i_) return;
    Context& c = ev_.ctx();
    c.require_device();
    const int L1 = c.L + 1;
    const size_t N = c.N;
    u64* m = c.dalloc<u64>((size_t)L1 * N);
    std::vector<u64> h((size_t)L1 * N, 0);
    for (int l = 0; l < L1; ++l) h[(size_t)l * N + N / 2] = 1;
    hip_check(hipMemcpyAsync(m, h.data(), h.size() * 8, hipMemcpyHostToDevice, c.stream), "monomial upload");
    hip_check(hipStreamSynchronize(c.stream), "monomial sync");
    launch_ntt(c.dt, LimbBatch{m, L1, nullptr, 0, L1}, false, c.stream);
    hip_check(hipGetLastError(), "monomial ntt");
    mono_i_ = m;
}

CtPtr Bootstrapper::mult_i(const CtPtr& x) {
    Context& c = ev_.ctx();
    CtPtr o = ev_.new_ct(x->npoly, x->ell, x->deg, x->scale, x->slots);
    launch_ew_mul(c.dt, o->d, x->d, mono_i_, x->npoly * x->ell, x->ell, 0, x->ell, c.stream);
    hip_check(hipGetLastError(), "mult_i");
    return o;
}

// the scale a stage takes its diagonals at: an input whose scale is not its level's own (the first stage after a ModRaise to fewer limbs
// than the chain has: run(drop > 0)) takes them at the scale that makes the product land on the next level's scale again; 0: the level's
static long double stage_pt_scale(const Context& c, const CtPtr& x) {
    const int lvl = x->level();
    if (x->ell >= 2 && fabsl(x->scale / c.sf_real[lvl] - 1.0L) > 1e-12L) return c.sf_real[lvl + 1] * (long double)c.chain.q[x->ell - 1] / x->scale;
    return 0;
}

CtPtr Bootstrapper::apply(const LinStage& st, const CtPtr& xin) {
    CtPtr x = xin->deg >= 2 ? ev_.rescale(xin) : xin;
    if (lt_) return ev_.linear_transform_rows({x}, st.lt_pts, st.lt_baby, st.lt_giant, false, stage_pt_scale(ev_.ctx(), x))[0];
    // baby steps: every rotation of x in ONE hoisted key switch (one ModUp of x, per-index inner product + ModDown)
    std::vector<int> bidx;
    for (const auto& t : st.terms)
        if (std::find(bidx.begin(), bidx.end(), t.baby) == bidx.end()) bidx.push_back(t.baby);
    std::vector<CtPtr> brot = ev_.rotate_many(x, bidx);
    std::map<int, CtPtr> babies;
    for (size_t i = 0; i < bidx.size(); ++i) babies[bidx[i]] = brot[i];
    // per giant step: sum_b diag_{g,b} * rot_b(x) as ONE inner-product pass (Evaluator::dot_plain) instead of a product
    // launch per term and a tree of additions
    std::map<int, std::pair<std::vector<CtPtr>, std::vector<PtPtr>>> groups;
    for (const auto& t : st.terms) {
        groups[t.giant].first.push_back(babies[t.baby]);
        groups[t.giant].second.push_back(t.diag);
    }
    const long double pt_scale = stage_pt_scale(ev_.ctx(), x);
    // the inner sums land in ONE block, in giant-step order (the shared-ModDown key switch below takes them as they stand), and
    // all of them come out of ONE pass over the rotated ciphertexts (Evaluator::dot_plain_groups); per-group passes otherwise
    std::map<int, CtPtr> inner;
    {
        CtPtr f = groups.begin()->second.first[0];
        const int ell_in = f->deg >= 2 ? f->ell - 1 : f->ell;
        std::vector<CtPtr> slab = ev_.new_ct_batch((int)groups.size(), 2, ell_in, 2, 0, f->slots);
        std::vector<int> order;   // unrotated group first, then the rotated ones in ascending order (= rotate_each_sum's order)
        for (auto& g : groups)
            if (g.first % f->slots == 0) order.push_back(g.first);
        for (auto& g : groups)
            if (g.first % f->slots != 0) order.push_back(g.first);
        std::vector<CtPtr> cts;
        for (int b : bidx) cts.push_back(babies[b]);
        std::vector<std::vector<PtPtr>> pts(order.size(), std::vector<PtPtr>(bidx.size()));
        for (const auto& t : st.terms) {
            const size_t gi = std::find(order.begin(), order.end(), t.giant) - order.begin();
            const size_t bi = std::find(bidx.begin(), bidx.end(), t.baby) - bidx.begin();
            pts[gi][bi] = t.diag;
        }
        if (ev_.dot_plain_groups(cts, pts, pt_scale, slab)) {
            for (size_t k = 0; k < order.size(); ++k) inner[order[k]] = slab[k];
        } else {
            size_t k = 0;
            for (int g : order) {
                auto& grp = groups[g];
                inner[g] = ev_.dot_plain(grp.first, grp.second, pt_scale, slab[k++]);
            }
        }
    }
    // giant steps: different inputs, different keys, same shape
    std::vector<CtPtr> gin;
    std::vector<int> gidx;
    for (auto& g : inner) {
        gin.push_back(g.second);
        gidx.push_back(g.first);
    }
    // sum_g rot(inner_g, g): own ModUp per term, ONE shared ModDown (Evaluator::rotate_each_sum)
    return ev_.rotate_each_sum(gin, gidx);
}

CtPtr Bootstrapper::mod_raise(const CtPtr& ct, long double& rho, int top_ell) {
    Context& c = ev_.ctx();
    CtPtr x = ct->deg >= 2 ? ev_.rescale(ct) : ct;
    if (x->npoly != 2) throw Error(FHELIN_ERR_STATE, "bootstrap: ciphertext must be relinearised");
    if (x->ell < 2) throw Error(FHELIN_ERR_STATE, "bootstrap: need at least two limbs to set the message scale (bootstrap one level earlier)");
    if (x->ell > 2) x = ev_.level_reduce(x, 2);
    const long double q0 = (long double)c.chain.q[0], q1 = (long double)c.chain.q[1];
    const long double target = q0 / (long double)(1ull << correction);
    const u64 k0 = (u64)llroundl(target * q1 / x->scale);
    if (k0 < 2) throw Error(FHELIN_ERR_STATE, "bootstrap: ciphertext scale too large for the correction factor");
    x = ev_.mult_int(x, k0, true, x->scale * (long double)k0);
    if (sparse_h_) x = ev_.switch_key(x, *ev_.to_sparse_key);   // to s~ at two limbs: the rescale divides the switch's noise
    x = ev_.rescale(x);  // one limb (q0), scale ~ q0 / 2^correction
    rho = x->scale * (long double)(1ull << correction) / q0;

    c.stats.bootstrap += 1;
    CtPtr up = ev_.raw_modraise(x, top_ell);
    up->deg = 1;
    up->scale = c.sf_real[0];   // the scale the CoeffsToSlots constants were built for (setup), whatever the start level
    up->slots = slots_;
    if (sparse_h_) up = ev_.switch_key(up, *ev_.from_sparse_key);   // I is now that of s~: back to s before anything reads a key of s
    // SubSum: project onto the subring of X^{N/(2 slots)} (sparse packing)
    const int gapN = (c.N / 2) / slots_;
    for (int j = 1; j < gapN; j <<= 1) {
        const u64 g = c.galois_element(slots_ * j);
        auto it = ev_.rot_keys.find(g);
        if (it == ev_.rot_keys.end()) throw Error(FHELIN_ERR_KEY, "bootstrap: SubSum rotation key missing");
        up = ev_.add(up, ev_.raw_rotate(up, g, *it->second));
    }
    return up;
}

// EvalMod of the real and the imaginary half together: both go through the same Chebyshev fit and double-angle steps,
// so every multiplication is one batched relinearisation over the pair
std::vector<CtPtr> Bootstrapper::eval_mod(const std::vector<CtPtr>& xs) {
    std::vector<CtPtr> u = ev_.eval_chebyshev_many(xs, cheb_, -1.0, 1.0);
    for (int i = 0; i < R; ++i) {
        if (ev_.merged_products) {     // rescale(2 u^2 - 1) in one go: the next step (or the first SlotsToCoeffs stage) rescales it anyway
            u = ev_.mult_affine_rescale_batch(u, u, 2, -1.0, {});
            continue;
        }
        // a step whose result the NEXT step squares is rescaled by that step's operand preparation, as it stands: rescaling it here gives
        // those residues, and the exact merged form does it inside the ModDown (Evaluator::mult_affine_batch; FHELIN_EXACT_PRODUCTS=0 keeps
        // the sequence below).  The last step's result stays at degree 2 for its consumer.
        if (i + 1 < R && ev_.exact_products_on()) {
            Evaluator::AffineSpec sq;
            sq.f = 2;
            sq.cadd = -1.0;
            u = ev_.mult_affine_batch(u, u, std::vector<Evaluator::AffineSpec>(u.size(), sq));
            continue;
        }
        std::vector<CtPtr> t = ev_.mult_batch(u, u);
        t = ev_.add_batch(t, t);
        for (size_t k = 0; k < t.size(); ++k) u[k] = ev_.add_real(t[k], -1.0);
    }
    return u;
}

CtPtr Bootstrapper::run(const CtPtr& ct, int stop_after, int drop) {
    if (!ready()) throw Error(FHELIN_ERR_STATE, "EvalBootstrapSetup has not been called");
    Context& c = ev_.ctx();
    if (drop < 0 || c.L + 1 - drop - depth_ < 1) throw Error(FHELIN_ERR_ARG, "bootstrap: level plan leaves no limb for the result");
    long double rho = 1;
    CtPtr w = mod_raise(ct, rho, c.L + 1 - drop);
    if (stop_after == 1) return w;
    for (const auto& st : c2s_) w = apply(st, w);
    if (packed_) w->slots = 2 * slots_;          // the last stage wrote [w | -i w] over 2n slots
    CtPtr wc = ev_.conjugate(w);
    CtPtr a = ev_.add(w, wc);                    // real parts  t_k / (q0 K)  (1/2 folded into the DFT constants); packed: [t_k | t_{k+n}]
    if (stop_after == 2) return a;
    CtPtr v;
    if (packed_) {
        v = eval_mod({a})[0];                    // one modular reduction for both halves
        if (stop_after == 3) return v;
    } else {
        CtPtr b = mult_i(ev_.sub(wc, w));        // imaginary   t_{k+n}   / (q0 K)
        if (stop_after == 3) return eval_mod({a})[0];
        std::vector<CtPtr> ab = eval_mod({a, b});
        v = ev_.add(ab[0], mult_i(ab[1]));
    }
    for (size_t i = 0; i < s2c_.size(); ++i) {
        v = apply(s2c_[i], v);
        if (packed_ && i == 0) v->slots = slots_;   // the first stage reads [L | R] over 2n slots and leaves an n-periodic vector
    }
    // slots now hold m * rho / 2^correction: undo the correction exactly and absorb rho in the scale
    v = ev_.mult_int(v, 1ull << correction, false, v->scale);
    v->scale = v->scale * rho;
    if (v->deg >= 2) v = ev_.rescale(v);
    v->slots = ct->slots > 0 ? ct->slots : logical_slots_;
    return v;
}

// ---- the same pipeline over a batch of independent ciphertexts ----------------------------------------------------------
// Every step below is the batched form of the step of run() / apply() above it stands for; each ciphertext goes through
// exactly the same residue operations (the batched evaluator entry points return the residues of the single ones).
std::vector<CtPtr> Bootstrapper::apply_batch(const LinStage& st, const std::vector<CtPtr>& xin) {
    Context& c = ev_.ctx();
    const size_t B = xin.size();
    std::vector<CtPtr> xs = xin[0]->deg >= 2 ? ev_.rescale_batch(xin) : xin;
    // every ciphertext of the batch in the launches of ONE engine call (they share a shape: one pipeline raised them together)
    if (lt_) return ev_.linear_transform_rows(xs, st.lt_pts, st.lt_baby, st.lt_giant, false, stage_pt_scale(c, xs[0]));
    std::vector<int> bidx;
    for (const auto& t : st.terms)
        if (std::find(bidx.begin(), bidx.end(), t.baby) == bidx.end()) bidx.push_back(t.baby);
    // baby steps: ONE ModUp over the batch, per ciphertext the inner products of all indices, ONE ModDown over everything
    std::vector<std::vector<CtPtr>> brot = ev_.rotate_many_batch(xs, bidx);
    const CtPtr& x = xs[0];
    const long double pt_scale = stage_pt_scale(c, x);
    // giant-step groups: the unrotated one first, then ascending (= rotate_each_sum's order)
    std::vector<int> order;
    {
        std::set<int> gs;
        for (const auto& t : st.terms) gs.insert(t.giant);
        for (int g : gs)
            if (g % x->slots == 0) order.push_back(g);
        for (int g : gs)
            if (g % x->slots != 0) order.push_back(g);
    }
    const size_t G = order.size();
    size_t n_plain = 0;
    for (int g : order) n_plain += g % x->slots == 0 ? 1 : 0;
    std::vector<std::vector<PtPtr>> pts(G, std::vector<PtPtr>(bidx.size()));
    for (const auto& t : st.terms) {
        const size_t gi = std::find(order.begin(), order.end(), t.giant) - order.begin();
        const size_t bi = std::find(bidx.begin(), bidx.end(), t.baby) - bidx.begin();
        pts[gi][bi] = t.diag;
    }
    // inner sums: the rotated groups of ALL ciphertexts in one block (the batched giant-step key switch takes them as they
    // stand), the unrotated groups in another
    std::vector<CtPtr> slab_plain, slab_rot;
    if (n_plain) slab_plain = ev_.new_ct_batch((int)(B * n_plain), 2, x->ell, 2, 0, x->slots);
    if (G > n_plain) slab_rot = ev_.new_ct_batch((int)(B * (G - n_plain)), 2, x->ell, 2, 0, x->slots);
    std::vector<std::vector<CtPtr>> rows(B), dests(B);
    for (size_t i = 0; i < B; ++i)
        for (size_t k = 0; k < G; ++k)
            dests[i].push_back(k < n_plain ? slab_plain[i * n_plain + k] : slab_rot[i * (G - n_plain) + (k - n_plain)]);
    // ONE pass for the whole batch where the operands are equally spaced (they are: the babies come out of one block per index,
    // the inputs out of one rescale): every diagonal is fetched once for all ciphertexts
    const bool batched = G <= (size_t)EwDotGroups::MAX_G && ev_.dot_plain_groups_batch(brot, pts, pt_scale, dests);
    for (size_t i = 0; i < B; ++i) {
        std::vector<CtPtr>& dest = dests[i];
        if (!batched && !ev_.dot_plain_groups(brot[i], pts, pt_scale, dest)) {
            for (size_t k = 0; k < G; ++k) {
                std::vector<CtPtr> cts;
                std::vector<PtPtr> ps;
                for (size_t b = 0; b < bidx.size(); ++b)
                    if (pts[k][b]) {
                        cts.push_back(brot[i][b]);
                        ps.push_back(pts[k][b]);
                    }
                dest[k] = ev_.dot_plain(cts, ps, pt_scale, dest[k]);
            }
        }
        // ascending giant shift, as apply() hands them to rotate_each_sum
        std::vector<std::pair<int, CtPtr>> byg;
        for (size_t k = 0; k < G; ++k) byg.push_back({order[k], dest[k]});
        std::sort(byg.begin(), byg.end(), [](const auto& a, const auto& b) { return a.first < b.first; });
        for (auto& e : byg) rows[i].push_back(e.second);
    }
    std::vector<int> gidx = order;
    std::sort(gidx.begin(), gidx.end());
    return ev_.rotate_each_sum_rows(rows, gidx);
}

// ---- the two kernels of a paired bootstrap ------------------------------------------------------------------------------------------
std::vector<CtPtr> Bootstrapper::pack_pairs(const std::vector<CtPtr>& a, const std::vector<CtPtr>& b, const std::vector<u64>& ka,
                                            const std::vector<u64>& kb) {
    Context& c = ev_.ctx();
    const size_t n = a.size();
    if (b.size() != n || ka.size() != n || kb.size() != n) throw Error(FHELIN_ERR_ARG, "pair pack: one partner and two constants per pair");
    if (n == 0) return {};
    for (size_t i = 0; i < n; ++i) {
        if (a[i]->npoly != 2 || b[i]->npoly != 2) throw Error(FHELIN_ERR_STATE, "bootstrap: ciphertext must be relinearised");
        if (a[i]->ell < 2 || b[i]->ell < 2)
            throw Error(FHELIN_ERR_STATE, "bootstrap: need at least two limbs to set the message scale (bootstrap one level earlier)");
    }
    ensure_mono_i();
    std::vector<u64> consts(n * 2 * 4);
    for (size_t i = 0; i < n; ++i)
        for (int l = 0; l < 2; ++l) {
            const u64 q = c.chain.q[l], ra = ka[i] % q, rb = kb[i] % q;
            u64* k = &consts[(i * 2 + l) * 4];
            k[0] = ra;
            k[1] = h_shoup(ra, q);
            k[2] = rb;
            k[3] = h_shoup(rb, q);
        }
    Scratch<u64> dk = c.scratch<u64>(consts.size());
    for (size_t off = 0; off < consts.size(); off += 2 * c.N)   // upload_async takes <= 2N words per call
        c.upload_async(dk + off, consts.data() + off, std::min(consts.size() - off, (size_t)2 * c.N));
    std::vector<CtPtr> out = ev_.new_ct_batch((int)n, 2, 2, 2, 0, a[0]->slots);
    for (size_t lo = 0; lo < n; lo += EwPairPack::MAX_PAIRS) {
        EwPairPack d;
        d.n = (int)std::min(n - lo, (size_t)EwPairPack::MAX_PAIRS);
        for (int k = 0; k < d.n; ++k) {
            d.a[k] = a[lo + k]->d;
            d.b[k] = b[lo + k]->d;
            d.ell_a[k] = a[lo + k]->ell;
            d.ell_b[k] = b[lo + k]->ell;
        }
        launch_ew_pair_pack(c.dt, d, out[lo]->d, mono_i_, dk + lo * 8, c.stream);
    }
    hip_check(hipGetLastError(), "pair pack");
    dk.reset();
    for (size_t i = 0; i < n; ++i) {
        out[i]->deg = a[i]->deg + 1;
        out[i]->scale = a[i]->scale * (long double)ka[i];
        out[i]->slots = a[i]->slots;
    }
    return out;
}

void Bootstrapper::split_pairs(const std::vector<CtPtr>& w, const std::vector<CtPtr>& wc, std::vector<CtPtr>& out_a, std::vector<CtPtr>& out_b) {
    Context& c = ev_.ctx();
    const size_t n = w.size();
    if (wc.size() != n) throw Error(FHELIN_ERR_ARG, "pair split: one conjugate per ciphertext");
    out_a.clear();
    out_b.clear();
    if (n == 0) return;
    const int ell = w[0]->ell;
    for (size_t i = 0; i < n; ++i)
        if (w[i]->npoly != 2 || wc[i]->npoly != 2 || w[i]->ell != ell || wc[i]->ell != ell)
            throw Error(FHELIN_ERR_STATE, "pair split: operands of different shapes");
    ensure_mono_i();
    std::vector<CtPtr> o = ev_.new_ct_batch((int)(2 * n), 2, ell, 1, 0, w[0]->slots);
    for (size_t lo = 0; lo < n; lo += EwPairSplit::MAX_PAIRS) {
        EwPairSplit d;
        d.n = (int)std::min(n - lo, (size_t)EwPairSplit::MAX_PAIRS);
        d.ell = ell;
        for (int k = 0; k < d.n; ++k) {
            d.w[k] = w[lo + k]->d;
            d.wc[k] = wc[lo + k]->d;
            d.a[k] = o[2 * (lo + k)]->d;
            d.b[k] = o[2 * (lo + k) + 1]->d;
        }
        launch_ew_pair_split(c.dt, d, mono_i_, c.stream);
    }
    hip_check(hipGetLastError(), "pair split");
    for (size_t i = 0; i < n; ++i)
        for (int h = 0; h < 2; ++h) {
            const CtPtr& x = o[2 * i + h];
            x->deg = w[i]->deg;
            x->scale = w[i]->scale;
            x->slots = w[i]->slots;
            (h ? out_b : out_a).push_back(x);
        }
}

// Per-item prologue, shared core, per-item epilogue.  A single goes through what run() does to it; a pair (a, b) enters as
// rescale(k0_a a + i k0_b b) - one pack launch over all pairs, the bottom limbs of both inputs read in place - and leaves through half of
// the exact 2^correction, one conjugation at the output level and the split (w + conj(w), i (conj(w) - w)) = (a, b) up to rho_a, rho_b,
// which go into the scales as a single's rho does.  Everything in between is message-agnostic and runs once over all items.
std::vector<CtPtr> Bootstrapper::run_items(const std::vector<Item>& items, int drop, int stop_after) {
    if (!ready()) throw Error(FHELIN_ERR_STATE, "EvalBootstrapSetup has not been called");
    Context& c = ev_.ctx();
    if (drop < 0 || c.L + 1 - drop - depth_ < 1) throw Error(FHELIN_ERR_ARG, "bootstrap: level plan leaves no limb for the result");
    const size_t B = items.size();
    if (B == 0) return {};
    const int top_ell = c.L + 1 - drop;
    // ---- prologue.  Inputs: item i has in[2 i] and, a pair, in[2 i + 1]; degree 2 is rescaled first (one batch over all of them)
    std::vector<CtPtr> in(2 * B);
    size_t n_pairs = 0;
    {
        std::vector<CtPtr> need;
        std::vector<size_t> pos;
        for (size_t i = 0; i < B; ++i) {
            in[2 * i] = items[i].a;
            in[2 * i + 1] = items[i].b;
            if (items[i].b) {
                ++n_pairs;
                const int sa = items[i].a->slots > 0 ? items[i].a->slots : logical_slots_;
                const int sb = items[i].b->slots > 0 ? items[i].b->slots : logical_slots_;
                if (sa != sb) throw Error(FHELIN_ERR_ARG, "bootstrap pair: the two ciphertexts must have the same slot count");
            }
        }
        if (n_pairs && correction < 1)
            throw Error(FHELIN_ERR_STATE, "bootstrap pair: correction 0 leaves no bit for the 1/2 of the split (bootstrap_config)");
        for (size_t k = 0; k < 2 * B; ++k)
            if (in[k] && in[k]->deg >= 2) {
                need.push_back(in[k]);
                pos.push_back(k);
            }
        if (!need.empty()) {
            std::vector<CtPtr> r = ev_.rescale_batch(need);
            for (size_t k = 0; k < pos.size(); ++k) in[pos[k]] = r[k];
        }
    }
    const long double q0 = (long double)c.chain.q[0], q1 = (long double)c.chain.q[1];
    const long double two_corr = (long double)(1ull << correction);
    const long double target = q0 / two_corr;
    std::vector<u64> k0(2 * B, 0);
    for (size_t k = 0; k < 2 * B; ++k) {
        if (!in[k]) continue;
        const CtPtr& x = in[k];
        if (x->npoly != 2) throw Error(FHELIN_ERR_STATE, "bootstrap: ciphertext must be relinearised");
        if (x->ell < 2) throw Error(FHELIN_ERR_STATE, "bootstrap: need at least two limbs to set the message scale (bootstrap one level earlier)");
        k0[k] = (u64)llroundl(target * q1 / x->scale);
        if (k0[k] < 2) throw Error(FHELIN_ERR_STATE, "bootstrap: ciphertext scale too large for the correction factor");
    }
    std::vector<CtPtr> xs(B);
    std::vector<long double> rho(B), rho_b(B, 1);
    if (n_pairs) {
        std::vector<CtPtr> pa, pb;
        std::vector<u64> ka, kb;
        for (size_t i = 0; i < B; ++i)
            if (in[2 * i + 1]) {
                pa.push_back(in[2 * i]);
                pb.push_back(in[2 * i + 1]);
                ka.push_back(k0[2 * i]);
                kb.push_back(k0[2 * i + 1]);
            }
        std::vector<CtPtr> packed = pack_pairs(pa, pb, ka, kb);
        size_t k = 0;
        for (size_t i = 0; i < B; ++i)
            if (in[2 * i + 1]) xs[i] = packed[k++];
    }
    for (size_t i = 0; i < B; ++i) {
        if (in[2 * i + 1]) {
            // the partner's rho: what mod_raise would compute for it alone (the scale of rescale(k0_b b), times 2^correction / q0)
            const CtPtr& y = in[2 * i + 1];
            rho_b[i] = y->scale * (long double)k0[2 * i + 1] / q1 * two_corr / q0;
            continue;
        }
        CtPtr x = in[2 * i];
        if (x->ell > 2) x = ev_.level_reduce(x, 2);
        xs[i] = ev_.mult_int(x, k0[2 * i], true, x->scale * (long double)k0[2 * i]);
    }
    if (sparse_h_) xs = ev_.switch_key_batch(xs, *ev_.to_sparse_key);   // mod_raise's switch to s~, one batched key switch over the items
    xs = ev_.rescale_batch(xs);
    for (size_t i = 0; i < B; ++i) rho[i] = xs[i]->scale * two_corr / q0;
    // ---- the shared core: ModRaise, SubSum, CoeffsToSlots, conjugation, EvalMod, SlotsToCoeffs
    c.stats.bootstrap += B;
    std::vector<CtPtr> w = ev_.raw_modraise_batch(xs, top_ell);
    for (CtPtr& u : w) {
        u->deg = 1;
        u->scale = c.sf_real[0];
        u->slots = slots_;
    }
    if (sparse_h_) w = ev_.switch_key_batch(w, *ev_.from_sparse_key);   // ... and its switch back to s
    const int gapN = (c.N / 2) / slots_;
    for (int j = 1; j < gapN; j <<= 1) {
        const u64 g = c.galois_element(slots_ * j);
        auto it = ev_.rot_keys.find(g);
        if (it == ev_.rot_keys.end()) throw Error(FHELIN_ERR_KEY, "bootstrap: SubSum rotation key missing");
        w = ev_.rotate_galois_batch(w, g, *it->second, true);     // u + sigma_g(u), the sum in the key switch's epilogue
    }
    if (stop_after == 1) return w;
    for (const auto& st : c2s_) w = apply_batch(st, w);
    if (packed_)
        for (CtPtr& u : w) u->slots = 2 * slots_;
    std::vector<CtPtr> wc = ev_.conjugate_batch(w);
    std::vector<CtPtr> a = ev_.add_batch(w, wc);
    if (stop_after == 2) return a;
    std::vector<CtPtr> v;
    if (packed_) {
        v = eval_mod(a);
        if (stop_after == 3) return v;
    } else {
        if (stop_after == 3) return eval_mod(a);
        std::vector<CtPtr> d = ev_.sub_batch(wc, w), all = a;
        for (const CtPtr& t : d) all.push_back(mult_i(t));
        std::vector<CtPtr> ab = eval_mod(all);
        std::vector<CtPtr> im;
        for (size_t i = 0; i < B; ++i) im.push_back(mult_i(ab[B + i]));
        v = ev_.add_batch(std::vector<CtPtr>(ab.begin(), ab.begin() + B), im);
    }
    for (size_t k = 0; k < s2c_.size(); ++k) {
        v = apply_batch(s2c_[k], v);
        if (packed_ && k == 0)
            for (CtPtr& u : v) u->slots = slots_;
    }
    // ---- epilogue.  A single: the exact 2^correction, rho into the scale.  A pair: half of it, so that the slots hold (a + i b) / 2 and
    // the split's sums come out at a and b themselves; its rhos go into the scales of the two halves
    std::vector<CtPtr> fin(B);
    for (size_t i = 0; i < B; ++i) {
        const bool pair = (bool)items[i].b;
        fin[i] = ev_.mult_int(v[i], 1ull << (pair ? correction - 1 : correction), false, v[i]->scale);
        if (!pair) fin[i]->scale = fin[i]->scale * rho[i];
    }
    if (fin[0]->deg >= 2) fin = ev_.rescale_batch(fin);
    std::vector<CtPtr> half_a, half_b;
    if (n_pairs) {
        std::vector<CtPtr> pv;
        for (size_t i = 0; i < B; ++i)
            if (items[i].b) pv.push_back(fin[i]);
        split_pairs(pv, ev_.conjugate_batch(pv), half_a, half_b);
    }
    auto slots_of = [&](const CtPtr& ct) { return ct->slots > 0 ? ct->slots : logical_slots_; };
    std::vector<CtPtr> out;
    size_t k = 0;
    for (size_t i = 0; i < B; ++i) {
        if (!items[i].b) {
            fin[i]->slots = slots_of(items[i].a);
            out.push_back(fin[i]);
            continue;
        }
        const long double s = fin[i]->scale;
        half_a[k]->scale = s * rho[i];
        half_b[k]->scale = s * rho_b[i];
        half_a[k]->slots = slots_of(items[i].a);
        half_b[k]->slots = slots_of(items[i].b);
        out.push_back(half_a[k]);
        out.push_back(half_b[k]);
        ++k;
    }
    return out;
}

std::vector<CtPtr> Bootstrapper::run_batch(const std::vector<CtPtr>& cts, int drop) {
    std::vector<Item> items;
    for (const CtPtr& ct : cts) items.push_back(Item{ct, CtPtr()});
    return run_items(items, drop);
}

std::vector<CtPtr> Bootstrapper::bootstrap_pairs(const std::vector<CtPtr>& cts, int drop) {
    if (cts.empty()) return {};
    Context::PhysicalScope physical(ev_.ctx());
    if (cts.size() == 1) return {run(cts[0], 0, drop)};
    if (!ready()) throw Error(FHELIN_ERR_STATE, "EvalBootstrapSetup has not been called");
    auto slots_of = [&](const CtPtr& ct) { return ct->slots > 0 ? ct->slots : logical_slots_; };
    std::vector<Item> items;
    for (size_t i = 0; i < cts.size(); i += 2) {
        if (i + 1 < cts.size() && slots_of(cts[i]) == slots_of(cts[i + 1])) {
            items.push_back(Item{cts[i], cts[i + 1]});
            continue;
        }
        items.push_back(Item{cts[i], CtPtr()});
        if (i + 1 < cts.size()) items.push_back(Item{cts[i + 1], CtPtr()});
    }
    return run_items(items, drop);   // item order is input order: two results per pair, one per single
}

std::pair<CtPtr, CtPtr> Bootstrapper::bootstrap_pair(const CtPtr& a, const CtPtr& b, int drop) {
    Context::PhysicalScope physical(ev_.ctx());
    std::vector<CtPtr> o = run_items({Item{a, b}}, drop);
    return {o[0], o[1]};
}

CtPtr Bootstrapper::pair_partial(const CtPtr& a, const CtPtr& b, int stage) {
    if (stage < 1 || stage > 3) throw Error(FHELIN_ERR_ARG, "bootstrap pair: stage must be 1, 2 or 3");
    Context::PhysicalScope physical(ev_.ctx());
    return run_items({Item{a, b}}, 0, stage)[0];
}

std::vector<CtPtr> Bootstrapper::bootstrap_batch(const std::vector<CtPtr>& cts, int drop) {
    if (cts.empty()) return {};
    Context::PhysicalScope physical(ev_.ctx());
    if (cts.size() == 1) return {run(cts[0], 0, drop)};
    return run_batch(cts, drop);
}

// ---- iterative bootstrapping ------------------------------------------------------------------------------------------------
std::vector<CtPtr> Bootstrapper::bootstrap_iter_batch(const std::vector<CtPtr>& cts, int p, int drop) {
    if (p < 1 || p > MAX_ITER_PRECISION) throw Error(FHELIN_ERR_ARG, "bootstrap_iter: precision must be in [1, 30]");
    if (!ready()) throw Error(FHELIN_ERR_STATE, "EvalBootstrapSetup has not been called");
    Context& c = ev_.ctx();
    if (drop < 0) throw Error(FHELIN_ERR_ARG, "bootstrap: level plan leaves no limb for the result");
    const int ell_y = c.L + 1 - drop - depth_;
    if (ell_y < 3) throw Error(FHELIN_ERR_STATE, "bootstrap_iter: the first bootstrap must leave at least three limbs (one for the final scaling)");
    const size_t B = cts.size();
    if (B == 0) return {};
    Context::PhysicalScope physical(c);
    // x2: exactly what ModRaise reads (rescaled if degree 2, two limbs); bootstrapping it gives the residues of bootstrapping x
    std::vector<CtPtr> x2(B);
    {
        std::vector<CtPtr> need;
        std::vector<size_t> pos;
        for (size_t i = 0; i < B; ++i) {
            if (cts[i]->npoly != 2) throw Error(FHELIN_ERR_STATE, "bootstrap: ciphertext must be relinearised");
            if (cts[i]->deg >= 2) {
                need.push_back(cts[i]);
                pos.push_back(i);
            } else {
                x2[i] = cts[i];
            }
        }
        if (!need.empty()) {
            std::vector<CtPtr> r = ev_.rescale_batch(need);
            for (size_t k = 0; k < pos.size(); ++k) x2[pos[k]] = r[k];
        }
        for (CtPtr& x : x2) {
            if (x->ell < 2) throw Error(FHELIN_ERR_STATE, "bootstrap: need at least two limbs to set the message scale (bootstrap one level earlier)");
            x = ev_.level_reduce(x, 2);
        }
    }
    const std::vector<CtPtr> y = bootstrap_batch(x2, drop);
    // e' = 2^p (y - x2): y brought to x2's two limbs and exact scale (FLEXIBLEAUTO, Evaluator::adjust), then one scaled difference
    std::vector<long double> xs_scale(B);
    for (size_t i = 0; i < B; ++i) xs_scale[i] = x2[i]->scale;
    const std::vector<CtPtr> ya = ev_.adjust_deg1_batch(y, 2, xs_scale);
    const u128 two_p = (u128)1 << p;
    const std::vector<CtPtr> e = ev_.scaled_diff_batch(ya, x2, std::vector<u128>(B, two_p), std::vector<u128>(B, two_p), false, xs_scale);
    const std::vector<CtPtr> z = bootstrap_batch(e, drop);
    // out = rescale(k (2^p y - z)): the scaled difference at 2^p s_y k, rescaled to the next level's standard scale
    std::vector<u128> ka(B), kc(B);
    std::vector<long double> w_scale(B);
    for (size_t i = 0; i < B; ++i) {
        if (z[i]->ell != y[i]->ell || z[i]->scale != y[i]->scale || z[i]->deg != y[i]->deg)
            throw Error(FHELIN_ERR_INTERNAL, "bootstrap_iter: the two bootstraps ended at different levels or scales");
        const long double s_w = y[i]->scale * (long double)two_p;
        const u64 k = (u64)llroundl(c.sf_real[y[i]->level() + 1] * (long double)c.chain.q[y[i]->ell - 1] / s_w);
        if (k < 1) throw Error(FHELIN_ERR_STATE, "bootstrap_iter: precision too large for the ciphertext scale");
        ka[i] = (u128)k << p;
        kc[i] = k;
        w_scale[i] = s_w * (long double)k;
    }
    std::vector<CtPtr> out = ev_.rescale_batch(ev_.scaled_diff_batch(y, z, ka, kc, true, w_scale));
    for (size_t i = 0; i < B; ++i) out[i]->slots = y[i]->slots;
    return out;
}

CtPtr Bootstrapper::bootstrap_iter(const CtPtr& ct, int p, int drop) { return bootstrap_iter_batch({ct}, p, drop)[0]; }

CtPtr Bootstrapper::bootstrap(const CtPtr& ct, int drop) {
    Context::PhysicalScope physical(ev_.ctx());
    return run(ct, 0, drop);
}
CtPtr Bootstrapper::partial(const CtPtr& ct, int stage) {
    Context::PhysicalScope physical(ev_.ctx());
    return run(ct, stage);
}

}  // namespace fhelin
