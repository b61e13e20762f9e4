#include "evaluator.h"
#include <map>
#include <set>
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstring>

namespace fhelin {

DevBlock::~DevBlock() {
    if (d && ctx) {
        try { ctx->pool.free(d); } catch (...) {}
    }
}
Ciphertext::~Ciphertext() {
    if (async_ev) (void)hipEventDestroy(async_ev);
    if (d && ctx && !block) {
        try { ctx->pool.free(d); } catch (...) {}
    }
}
Encoding::~Encoding() {
    if (ready) (void)hipEventDestroy(ready);
    if (d && ctx) {
        try { ctx->pool.free(d, lanes_ordered); } catch (...) {}   // every lane that used it may still have reads queued
    }
}
EvalKey::~EvalKey() {
    if (d && ctx) {
        try { ctx->pool.free(d); } catch (...) {}
    }
    if (d_perm && ctx) {
        try { ctx->pool.free(d_perm); } catch (...) {}
    }
}

static void launch_ok(const char* what) { hip_check(hipGetLastError(), what); }

namespace {
// consecutive runs of operands with the same (components, limbs): one output block and one launch per <= 32 of them
template <class SameShape, class Emit>
void for_runs(size_t n, SameShape same, Emit emit) {
    size_t lo = 0;
    while (lo < n) {
        size_t hi = lo + 1;
        while (hi < n && hi - lo < (size_t)EwItems::MAX_ITEMS && same(lo, hi)) ++hi;
        emit(lo, hi);
        lo = hi;
    }
}

// groups of operands that share one launch set, wherever they stand in the list: the leader of a group is the first index not yet
// done, its members the leader and the later indices not yet done for which same(leader, i) holds, in ascending order, until `limit`
// are collected - each is compared with the leader, never with another member.  run(idx) returns one output per member, in the
// order of idx; output k goes to out[idx[k]].
template <class Same, class Run>
std::vector<CtPtr> for_groups(size_t n, int limit, Same same, Run run) {
    std::vector<CtPtr> out(n);
    std::vector<char> done(n, 0);
    for (size_t first = 0; first < n; ++first) {
        if (done[first]) continue;
        std::vector<size_t> idx{first};
        for (size_t i = first + 1; i < n && (int)idx.size() < limit; ++i)
            if (!done[i] && same(first, i)) idx.push_back(i);
        std::vector<CtPtr> o = run(idx);
        for (size_t k = 0; k < idx.size(); ++k) {
            out[idx[k]] = std::move(o[k]);
            done[idx[k]] = 1;
        }
    }
    return out;
}

std::vector<CtPtr> pick(const std::vector<CtPtr>& v, const std::vector<size_t>& idx) {
    std::vector<CtPtr> o;
    o.reserve(idx.size());
    for (size_t i : idx) o.push_back(v[i]);
    return o;
}
}  // namespace

CtPtr Evaluator::new_ct(int npoly, int ell, int deg, long double scale, int slots) {
    c_.require_device();
    if (ell < 1 || ell > c_.L + 1 || npoly < 1 || npoly > 3) throw Error(FHELIN_ERR_ARG, "new_ct: bad shape");
    auto ct = std::make_shared<Ciphertext>();
    ct->ctx = &c_;
    ct->npoly = npoly;
    ct->ell = ell;
    ct->deg = deg;
    ct->scale = scale;
    ct->slots = slots;
    ct->d = c_.dalloc<u64>(ct->words());
    c_.stride_locked = true;
    return ct;
}

CtPtr Evaluator::clone(const CtPtr& a) {
    CtPtr o = new_ct(a->npoly, a->ell, a->deg, a->scale, a->slots);
    hip_check(hipMemcpyAsync(o->d, a->d, a->words() * 8, hipMemcpyDeviceToDevice, c_.stream), "clone");
    return o;
}

std::vector<CtPtr> Evaluator::new_ct_batch(int count, int npoly, int ell, int deg, long double scale, int slots) {
    c_.require_device();
    // ell = L + 2: wrapped inputs over q_0..q_L, p_0 (include/fhelin.h "Wrapped inputs")
    if (count < 1 || ell < 1 || ell > c_.L + 1 + (c_.K > 0 ? 1 : 0) || npoly < 1 || npoly > 3) throw Error(FHELIN_ERR_ARG, "new_ct_batch: bad shape");
    auto blk = std::make_shared<DevBlock>();
    blk->ctx = &c_;
    const size_t words = (size_t)npoly * ell * c_.N;
    blk->d = c_.dalloc<u64>(words * count);
    c_.stride_locked = true;
    std::vector<CtPtr> v;
    for (int i = 0; i < count; ++i) {
        auto ct = std::make_shared<Ciphertext>();
        ct->ctx = &c_;
        ct->npoly = npoly;
        ct->ell = ell;
        ct->deg = deg;
        ct->scale = scale;
        ct->slots = slots;
        ct->block = blk;
        ct->d = blk->d + words * i;
        v.push_back(ct);
    }
    return v;
}

u64* Evaluator::contiguous_base(const std::vector<CtPtr>& v) {
    if (v.empty() || !v[0]->block) return nullptr;
    const size_t words = v[0]->words();
    for (size_t i = 0; i < v.size(); ++i)
        if (v[i]->block != v[0]->block || v[i]->d != v[0]->d + words * i || v[i]->words() != words) return nullptr;
    return v[0]->d;
}

std::vector<CtPtr> Evaluator::make_contiguous(const std::vector<CtPtr>& v, int site) {
    if (v.size() <= 1 || contiguous_base(v)) return v;
    if (site >= 0 && site < 8) gather_copies[site] += v.size();   // FHELIN_COPY_STATS=1 prints these when the context goes away
    std::vector<CtPtr> o = new_ct_batch((int)v.size(), v[0]->npoly, v[0]->ell, v[0]->deg, v[0]->scale, v[0]->slots);
    for (size_t lo = 0; lo < v.size(); lo += EwItems::MAX_ITEMS) {   // one launch per 32 ciphertexts (a copy each costs 6.5 us in the stream)
        EwItems it;
        it.n = (int)std::min<size_t>(EwItems::MAX_ITEMS, v.size() - lo);
        it.vecs = v[0]->npoly * v[0]->ell;
        it.b_vecs = 0;
        for (int i = 0; i < it.n; ++i) {
            if (v[lo + i]->words() != v[0]->words()) throw Error(FHELIN_ERR_INTERNAL, "make_contiguous: operands of different shapes");
            it.out[i] = o[lo + i]->d;
            it.a[i] = v[lo + i]->d;
            it.b[i] = nullptr;
        }
        launch_ew_items(c_.dt, it, 4, v[0]->ell, c_.stream);
    }
    hip_check(hipGetLastError(), "batch gather");
    return o;
}

KeyPtr Evaluator::new_key(int max_ell) {
    c_.require_device();
    if (max_ell < 0 || max_ell > c_.L + 1) throw Error(FHELIN_ERR_ARG, "new_key: max_ell out of range");
    auto k = std::make_shared<EvalKey>();
    k->ctx = &c_;
    k->max_ell = max_ell ? max_ell : c_.L + 1;
    k->digits = c_.digits_at(k->max_ell);
    k->d = c_.dalloc<u64>(k->words());
    if (k->capped()) {   // the absent Q rows of the digits held: zero once, here; the makers write present rows only
        hip_check(hipMemsetAsync(k->d, 0, k->words() * sizeof(u64), c_.stream), "hipMemsetAsync(capped key)");
    }
    c_.stride_locked = true;
    return k;
}

void Evaluator::bind_key(const EvalKey& key, int ell) {
    if (ell > key.max_ell) {
        std::string who = key.kind == 1 ? "relinearisation key" : key.kind == 3 ? "conjugation key" : key.kind == 4 ? "to-sparse key" :
                          key.kind == 5 ? "from-sparse key" : "rotation key";
        if (key.kind != 1 && key.has_index) who += " for index " + std::to_string(key.index);
        if (key.kind == 2 || key.kind == 3) who += " (Galois element " + std::to_string((unsigned long long)key.galois) + ")";
        throw Error(FHELIN_ERR_KEY, who + " is capped at " + std::to_string(key.max_ell) + " limbs: a key switch at " + std::to_string(ell) +
                                        " limbs was asked for");
    }
    if (usage_on) {
        int& m = usage[{key.kind, key.galois}];
        m = std::max(m, ell);
    }
}

void Evaluator::bind_rotations(const Rotations& rot, const std::vector<CtPtr>& v, bool rescales_first) {
    for (const CtPtr& x : v)
        for (int r = 0; r < rot.n; ++r) bind_key(*rot.key[r], rescales_first && x->deg >= 2 ? x->ell - 1 : x->ell);
}

// ------------------------------------------------------------------------------------------------
void Evaluator::keyswitch(const u64* c_ntt, int ell, const EvalKey& key, u64* out, const u64* add0, const u64* add1,
                          const u32* map, const u64* post) {
    keyswitch_batch(1, c_ntt, 0, ell, key, out, 0, add0, add1, 0, map, post, 0);
}

void Evaluator::keyswitch_batch(int B, const u64* c_ntt, size_t c_stride, int ell, const EvalKey& key, u64* out, size_t out_stride,
                                const u64* add0, const u64* add1, size_t add_stride, const u32* map, const u64* post,
                                size_t post_stride) {
    keyswitch_impl(B, nullptr, c_ntt, c_stride, ell, &key, out, out_stride, add0, add1, add_stride, map, post, post_stride);
}

void Evaluator::keyswitch_rows(const KsRows& rows, const u64* c_ntt, size_t c_stride, int ell, u64* out, size_t out_stride,
                               const u64* add0, size_t add_stride) {
    const int B = (int)rows.keys.size();
    if (B < 1) return;
    if (B > KsShape::MAX_ROWS || rows.maps.size() != rows.keys.size()) throw Error(FHELIN_ERR_ARG, "keyswitch_rows: bad row count");
    keyswitch_impl(B, &rows, c_ntt, c_stride, ell, nullptr, out, out_stride, add0, nullptr, add_stride, nullptr, nullptr, 0);
}

void Evaluator::keyswitch_impl(int B, const KsRows* rows, const u64* c_ntt, size_t c_stride, int ell, const EvalKey* key, u64* out,
                               size_t out_stride, const u64* add0, const u64* add1, size_t add_stride, const u32* map, const u64* post,
                               size_t post_stride) {
    c_.require_device();
    if (c_.K < 1) throw Error(FHELIN_ERR_STATE, "hybrid key switching needs at least one special prime");
    if (B < 1) return;
    if (key) bind_key(*key, ell);
    else
        for (int b = 0; b < B; ++b) bind_key(*rows->keys[b], ell);
    KsShape sh = ks_shape(ell, B, {c_stride, out_stride, add_stride, post_stride});
    const bool shared = rows && rows->shared_input;
    if (rows) {
        sh.per_row = 1;
        sh.shared_input = shared ? 1 : 0;
        for (int b = 0; b < B; ++b) {
            sh.evk_row[b] = rows->keys[b]->d;
            sh.map_row[b] = rows->maps[b];
        }
    }
    KsShape shu = sh;
    shu.batch = shared ? 1 : B;  // polynomials that go through ModUp
    c_.stats.keyswitch += (u64)B;
    c_.stats.keyswitch_limbs += (u64)B * ell;
    const bool identity = !map && !rows;
    const bool gather = !identity && !add1 && rot_in_gather();
    const u64* evk = key ? key->d : nullptr;
    // the rotation is applied while the inner product loads its operands; c0 (add0) enters accQ there, times P
    if (gather) evk = set_gather(sh, rows ? rows->keys.data() : &key, rows ? rows->maps.data() : &map, add0, add_stride);
    Scratch<u64> ext = modup(shu, c_ntt, !gather);   // digits times 2^64 for the keys as they are stored: launch_ks_inner ends in redc128
    KsAcc acc = inner_product(sh, ext, evk, c_ntt, moddown_tail(gather ? KsOutput::Gathered : identity ? KsOutput::Identity : KsOutput::Scattered));
    moddown(acc, gather ? KsOut{out, nullptr, nullptr, post} : KsOut{out, add0, add1, post, map});
    launch_ok("keyswitch");
}

// ------------------------------------------------------------------------------------------------ key-switch stages
// Every hybrid key switch of this file is ks_shape -> modup -> inner_product -> one of the tails moddown / moddown_rescale /
// moddown_rescale_exact.  inner_product is told the tail (KsTail) and returns the accumulator (KsAcc): the shape as decided, accQ / accP
// as far as they exist, and what the tail's row pass needs where the Q-limb sums are left to it.  It alone allocates them and asks
// accp_in_rows / accq_in_rows; a tail takes that object and where its output goes (KsOut), nothing else.  A caller with an inner-product
// kernel of its own takes the same object from accumulators().  A merged rotation sum is set_rotations, modup and rotation_sum; a plain
// rotation that gathers puts set_gather in front.  A change to the pipeline (what the conversions compute, where a transform's epilogue
// takes over a finish or a product, how a merged sum feeds its ModDown) belongs HERE, once.  Which operands share a launch set is
// decided before that, also once: for_groups (top of this file) with same_shape (evaluator.h).

KsShape Evaluator::ks_shape(int ell, int batch, const KsStrides& st) const {
    return KsShape{ell, c_.K, c_.alpha, c_.lvl[ell].beta, c_.L + 1, batch, st.c, st.out, st.add, st.post};
}

// Does a plain ModDown finish in the row pass of NTT(conv) (RowPass), or in launch_moddown_finish over the stored transform (Finish)?
//   output of the ModDown                          RowPass when
//   Identity   (relinearisation, linear transform)  FHELIN_FUSE_MODDOWN=1 or FHELIN_FUSE_FINISH=1
//   Gathered   (set_gather)                         always: callers gather only under rot_in_gather(), FUSE_FINISH && ROT_GATHER && !FUSE_MODDOWN
//   Scattered  (through the rotation's map)         FHELIN_FUSE_MODDOWN=1
//   MergedSum  (rotation_sum, hoisted_dot_rows)     FHELIN_FUSE_FINISH=1 and FHELIN_ROT_GATHER=1 (c0 parts then enter accQ times P)
Evaluator::KsTail Evaluator::moddown_tail(KsOutput o) const {
    const bool rows = o == KsOutput::Gathered || (o == KsOutput::Identity && (c_.fuse_moddown || c_.fuse_finish)) ||
                      (o == KsOutput::Scattered && c_.fuse_moddown) || (o == KsOutput::MergedSum && c_.fuse_finish && c_.rot_gather);
    return rows ? KsTail::RowPass : KsTail::Finish;
}

const u64* Evaluator::set_gather(KsShape& sh, const EvalKey* const* keys, const u32* const* maps, const u64* c0, size_t c0_stride) {
    const u64* evk = nullptr;
    for (int b = 0; b < (sh.per_row ? (sh.row_mod ? sh.row_mod : sh.batch) : 1); ++b) bind_key(*keys[b], sh.ell);
    sh.gather = 1;
    if (sh.per_row) {
        for (int b = 0; b < (sh.row_mod ? sh.row_mod : sh.batch); ++b) {
            sh.evk_row[b] = permuted(*keys[b], maps[b]);
            sh.ginv_row[b] = c_.automorph_ginv_of(maps[b]);
        }
    } else {
        evk = permuted(*keys[0], maps[0]);
        sh.map_row[0] = maps[0];
        sh.ginv = c_.automorph_ginv_of(maps[0]);
    }
    if (c0) {
        sh.gsrc = c0;
        sh.gsrc_stride = c0_stride;
        sh.gsrc_pmod = c_.d_pmod;
    }
    return evk;
}

// ModUp of up.batch polynomials of up.ell limbs, NTT form at src, up.c_stride words apart (group2 > 0: only within runs of group2
// polynomials; the runs lie group2_stride apart): coefficient form, basis conversion of every digit to the other limbs of QP, forward NTT
// of the converted limbs.  Returns the digits [up.batch][beta][ell+K][N], lazily reduced (below 2^60: only the inner products
// read them); times_r2: times 2^64, for launch_ks_inner over the keys as they are stored.
Scratch<u64> Evaluator::modup(const KsShape& up, const u64* src, bool times_r2, int group2, size_t group2_stride) {
    const size_t N = c_.N;
    const int n = up.batch, ell = up.ell, nt = ell + c_.K;
    const LevelTables& lt = c_.lvl[ell];
    Scratch<u64> cc = c_.scratch<u64>((size_t)n * ell * N);
    {
        // out of place: cc = INTT(src); the inputs of a batch are strided (c1 of consecutive ciphertexts)
        LimbBatch ib{cc, n * ell, nullptr, 0, ell, src};
        if (n > 1 && up.c_stride != (size_t)ell * N) {
            ib.src_group = ell;
            ib.src_group_stride = up.c_stride;
        }
        if (group2 > 0) {
            ib.src_group2 = group2;
            ib.src_group2_stride = group2_stride;
        }
        c_.ntt(ib, true);
    }
    Scratch<u64> ext = c_.scratch<u64>((size_t)n * lt.beta * nt * N);
    launch_modup_conv(c_.dt, up, ext, cc, src, lt.up_hatinv, times_r2 ? lt.up_hatmod_r2 : lt.up_hatmod, c_.stream);
    LimbBatch eb{ext, n * lt.beta * nt, lt.ext_limb_tab, 0, 1};
    eb.tab_len = lt.beta * nt;
    eb.lazy_out = true;  // only the inner products read the digits: they take any residue below 2^60
    c_.ntt(eb, false, n * (lt.beta * nt - ell));
    return ext;
}

// The inner product of a key switch.  With FHELIN_FUSE_ACCP_ROWS the inner-product launch covers the Q limbs only and the special-limb
// sums are formed by the inverse row pass of their own transform (launch_ntt_rows_product): accP is never stored in NTT form, read back
// and stored again, and the ModDown starts at the column pass.  The same residues bit for bit.  Left on the separate launches: the merged
// rotation sums unless the knob is 2 (Context::fuse_accp_rows: measured slower), the exact-products tail (its accP carries a K+1-th limb
// that launch_affine_acc_items writes), a caller that works on accP before its tail (KsTail::EditsAccP) and, below
// Context::accp_rows_min_vecs vectors, the small accumulators.
bool Evaluator::accp_in_rows(const KsShape& sh, KsTail tail) const {
    const int K = c_.K, nvec = sh.batch * 2 * K;
    const bool measured_faster = !sh.n_rot && sh.beta <= 8;   // the single-key classes of tools/accp_rows_probe.py where the fused form wins
    const bool want = c_.fuse_accp_rows >= 2 || (c_.fuse_accp_rows == 1 && measured_faster);
    return tail != KsTail::EditsAccP && want && !sh.accp_limbs && sh.k == K && nvec >= c_.accp_rows_min_vecs;
}

// FHELIN_FUSE_ACCQ_ROWS: the Q-limb half of a single-key inner product whose ModDown ends in the row pass of NTT(conv) is
// formed by that row pass, where it used to read accQ back: launch_ks_inner does not run and accQ does not exist.  Only together with the
// special-limb half (inner_product asks accp_in_rows first).  Left alone: the merged sums, moddown_rescale and the exact-products tail
// (they work on accQ), the linear transforms' dot kernel, every ModDown that ends in launch_moddown_finish.
bool Evaluator::accq_in_rows(const KsShape& sh, KsTail tail) const {
    const bool measured_faster = sh.beta <= 8 && sh.batch * 2 * sh.ell >= c_.accq_rows_min_vecs;   // tools/accq_rows_probe.py
    const bool want = c_.fuse_accq_rows >= 2 || (c_.fuse_accq_rows == 1 && measured_faster);
    return tail == KsTail::RowPass && !sh.n_rot && want;
}

Evaluator::KsAcc Evaluator::accumulators(const KsShape& sh, KsTail tail) {
    const size_t pairs = (size_t)sh.batch * 2 * c_.N;
    return KsAcc{sh, tail, c_.scratch<u64>(pairs * sh.ell), c_.scratch<u64>(pairs * (sh.accp_limbs ? sh.accp_limbs : sh.k)), {}};
}

// The two rules above, the launches they leave to the inner product, and the special-limb row pass; the Q-limb row pass is the ModDown's
// (moddown_rows), which acc.qprod describes to it - accQ is then not even allocated.
Evaluator::KsAcc Evaluator::inner_product(const KsShape& shape, const u64* ext, const u64* evk, const u64* c_ntt, KsTail tail) {
    const int K = c_.K, nvec = shape.batch * 2 * K;
    KsAcc acc{shape, tail, {}, {}, {}};
    KsShape& sh = acc.sh;
    sh.accp_rows = accp_in_rows(sh, tail) ? 1 : 0;
    sh.accq_rows = sh.accp_rows && accq_in_rows(sh, tail) ? 1 : 0;
    if (!sh.accq_rows) acc.accQ = c_.scratch<u64>((size_t)sh.batch * 2 * sh.ell * c_.N);
    acc.accP = c_.scratch<u64>((size_t)nvec * c_.N);
    if (sh.n_rot) launch_ks_inner_multi(c_.dt, sh, acc.accQ, acc.accP, ext, c_ntt, c_.stream);   // a merged sum
    else if (!sh.accq_rows) launch_ks_inner(c_.dt, sh, acc.accQ, acc.accP, ext, evk, c_ntt, c_.stream);
    if (!sh.accp_rows) return acc;
    acc.qprod = NttProduct{sh, ext, evk, sh.n_rot ? 1 : 0, c_ntt};
    c_.stats.limb_ntt += (u64)nvec;   // the transform of accP is counted here, where its first pass runs
    launch_ntt_rows_product(c_.dt, LimbBatch{acc.accP, nvec, nullptr, c_.L + 1, K}, acc.qprod, c_.stream);
    return acc;
}

void Evaluator::accp_inverse(KsAcc& acc) {
    const LimbBatch b{acc.accP, acc.sh.batch * 2 * c_.K, nullptr, c_.L + 1, c_.K};
    if (acc.sh.accp_rows) launch_ntt_cols_inverse(c_.dt, b, c_.stream);
    else c_.ntt(b, true);
}

static void made_for(bool ok, const char* tail) {   // what inner_product left to a tail's transforms is left to THAT tail's
    if (!ok) throw Error(FHELIN_ERR_INTERNAL, std::string(tail) + ": the accumulator was made for another tail");
}

// ModDown of the accumulator pair accQ [sh.batch][2][ell][N], accP [sh.batch][2][K][N] (accP is transformed in place):
// o.out = (accQ - NTT(conv(INTT(accP)))) * P^-1 + add0/add1 (+ post), written through o.map / the rows' maps.
// sh.gather: the pair was gathered through the rotation's map by launch_ks_inner (c0 included): the conversion takes the signs of the
// automorphism into account (launch_moddown_conv) and the output map is the identity - tail RowPass, no map, no add0.
// KsTail::RowPass: the finish rides in the row pass of NTT(conv) - (accQ - NTT(conv)) * P^-1 + add (+ post) is formed in registers and
// NTT(conv) never goes to memory; else launch_moddown_finish reads the stored transform.  The row pass knows no gather: the c0 parts
// of a merged rotation sum (sh.gsrc) must then be in accQ already, times P (sh.gsrc_pmod, launch_ks_inner_multi).
Scratch<u64> Evaluator::moddown_conv(KsAcc& acc) {
    const KsShape& sh = acc.sh;
    made_for(acc.tail == KsTail::RowPass || acc.tail == KsTail::Finish, "moddown");
    if (acc.tail == KsTail::RowPass && sh.gsrc && !sh.gsrc_pmod) throw Error(FHELIN_ERR_INTERNAL, "moddown: the row pass cannot gather");
    accp_inverse(acc);
    Scratch<u64> conv = c_.scratch<u64>((size_t)sh.batch * 2 * sh.ell * c_.N);
    launch_moddown_conv(c_.dt, sh, conv, acc.accP, c_.d_phatinv, c_.d_phatmod, c_.stream);
    if (acc.tail != KsTail::RowPass) c_.ntt(LimbBatch{conv, sh.batch * 2 * sh.ell, nullptr, 0, sh.ell}, false);
    return conv;
}

void Evaluator::moddown(KsAcc& acc, const KsOut& o) {
    Scratch<u64> conv = moddown_conv(acc);
    if (acc.tail == KsTail::RowPass) moddown_rows(acc, conv, o);
    else launch_moddown_finish(c_.dt, acc.sh, o.out, acc.accQ, conv, c_.d_pinv, o.add0, o.add1, o.map, o.post, c_.stream);
}

void Evaluator::moddown_rows(const KsAcc& acc, u64* conv, const KsOut& o) {
    const KsShape& sh = acc.sh;
    const int B = sh.batch, ell = sh.ell;
    const LimbBatch cb{conv, B * 2 * ell, nullptr, 0, ell};
    NttEpilogue ep;
    ep.acc = acc.accQ;
    ep.acc_poly_stride = (size_t)ell * c_.N;
    ep.out = o.out;
    ep.out_stride = sh.out_stride;
    ep.w = c_.d_pinv;
    ep.ell = ell;
    ep.add0 = o.add0;
    ep.add1 = o.add1;
    ep.add_stride = sh.add_stride;
    ep.post = o.post;
    ep.post_stride = sh.post_stride;
    if (sh.gather) {
        // the accumulator pair and the conversion are sigma_g of the ungathered ones already: identity output
    } else if (sh.per_row) {
        ep.per_row = 1;
        for (int b = 0; b < B; ++b) ep.invmap_row[b] = c_.automorph_inverse_of(sh.map_row[b]);
    } else if (o.map) {
        ep.invmap = c_.automorph_inverse_of(o.map);
    }
    if (sh.accq_rows) c_.ntt_epilogue_product(cb, ep, acc.qprod);   // ep.acc is null: formed by the row pass from the key switch's own operands
    else c_.ntt_epilogue(cb, ep);
}

// ModDown and rescale as ONE basis conversion (sh.ell >= 2, K + 1 <= 16): P and the top limb of the accumulator pair are dropped together,
// out [sh.batch][2][ell-1][N] (sh.out_stride apart) = (accQ - NTT(conv(INTT(accP), INTT(top limb of accQ)))) * (P q_top)^-1
void Evaluator::moddown_rescale(KsAcc& acc, u64* out) {
    const KsShape& sh = acc.sh;
    const size_t N = c_.N;
    const int B = sh.batch, ell = sh.ell;
    const LevelTables& lt = c_.lvl[ell];
    made_for(acc.tail == KsTail::Rescale || acc.tail == KsTail::EditsAccP, "moddown_rescale");
    accp_inverse(acc);
    Scratch<u64> top = c_.scratch<u64>((size_t)B * 2 * N);
    {
        LimbBatch tb{top, B * 2, nullptr, ell - 1, 1, acc.accQ + (size_t)(ell - 1) * N};
        tb.src_group = 1;
        tb.src_group_stride = (size_t)ell * N;
        c_.ntt(tb, true);
    }
    Scratch<u64> conv = c_.scratch<u64>((size_t)B * 2 * (ell - 1) * N);
    launch_moddown_rescale_conv(c_.dt, sh, conv, acc.accP, top, lt.md_hatinv, lt.md_hatmod, lt.md_mmod, c_.stream);
    moddown_rescale_finish(acc, out, conv, lt.md_minv);
}

// ModDown, the affine step and the rescale of a relinearised product with their own two roundings, from ONE inverse and ONE forward
// transform (sh.ell >= 2, K + 1 <= 16; kernels_elem.h "the EXACT merged tail").  accQ [sh.batch][2][ell][N] holds X_Q on the limbs below
// the top one, accP [sh.batch][2][K+1][N] the special limbs as the inner product left them and X_Q,top (launch_affine_acc_items); f2: the
// items whose factor is 2.  out [sh.batch][2][ell-1][N] = the residues of rescale(ModDown + affine step).
void Evaluator::moddown_rescale_exact(KsAcc& acc, u64* out, u32 f2) {
    const KsShape& sh = acc.sh;
    const int B = sh.batch, ell = sh.ell, K = c_.K;
    const LevelTables& lt = c_.lvl[ell];
    made_for(acc.tail == KsTail::Exact, "moddown_rescale_exact");
    {
        LimbBatch ib{acc.accP, B * 2 * (K + 1), lt.mdx_limb_tab, 0, 1};
        ib.tab_len = K + 1;
        c_.ntt(ib, true);
    }
    Scratch<u64> conv = c_.scratch<u64>((size_t)B * 2 * (ell - 1) * c_.N);
    launch_moddown_rescale_exact_conv(c_.dt, sh, f2, conv, acc.accP, c_.d_phatinv, c_.d_phatmod, c_.d_pinv, c_.d_pmod,
                                      c_.d_qlmod + (size_t)(ell - 1) * (c_.L + 1), c_.stream);
    moddown_rescale_finish(acc, out, conv, lt.md_minv);   // md_minv = (P q_top)^-1 mod q_t
}

// the row pass of NTT(conv) finishes (accQ - NTT(conv)) * minv into out (FHELIN_FUSE_FINISH=0: moddown_rescale_finish_kernel)
void Evaluator::moddown_rescale_finish(const KsAcc& acc, u64* out, u64* conv, const u64* minv) {
    const KsShape& sh = acc.sh;
    const int e1 = sh.ell - 1;
    const LimbBatch cb{conv, sh.batch * 2 * e1, nullptr, 0, e1};
    if (c_.fuse_finish) {
        NttEpilogue ep;
        ep.acc = acc.accQ;
        ep.acc_poly_stride = (size_t)sh.ell * c_.N;
        ep.out = out;
        ep.out_stride = sh.out_stride;
        ep.w = minv;
        ep.ell = e1;
        c_.ntt_epilogue(cb, ep);
        return;
    }
    c_.ntt(cb, false);
    launch_moddown_rescale_finish(c_.dt, sh, out, acc.accQ, conv, minv, c_.stream);
}

Evaluator::Rotations Evaluator::rotations(const int* indices, int n) {
    Rotations rot;
    rot.n = n;
    for (int r = 0; r < n; ++r) {
        const RotKey k = rotation_key(indices[r]);
        rot.key[r] = k.key.get();
        rot.map[r] = k.map;
        // the automorphism of g keeps every 512-coefficient tile in place iff g = 1 mod N/256 (index bits above the tile
        // correspond to the low bits of the odd exponent 2 bitrev(j) + 1, which multiplication by such a g leaves alone)
        if (k.g % (u64)(c_.N / 256) != 1) rot.tiles_in_place = false;
    }
    return rot;
}

// The rotations of a merged key switch (launch_ks_inner_multi) into its shape: sh.n_rot, sh.map_rot and sh.evk_rot - keys[r] where given
// (keys in the layout of EvalKey::d_perm: folded keys), else the rotation key's permuted copy.  shared_digits: the rotations act on ONE
// input, whose digit tiles are staged in LDS when every automorphism keeps them in place (sh.lds_digits).
void Evaluator::set_rotations(KsShape& sh, const Rotations& rot, bool shared_digits, const u64* const* keys) {
    for (int r = 0; r < rot.n; ++r) bind_key(*rot.key[r], sh.ell);   // a folded key is its rotation key's copy: the same cap
    sh.n_rot = rot.n;
    for (int r = 0; r < rot.n; ++r) {
        sh.map_rot[r] = rot.map[r];
        sh.evk_rot[r] = keys ? keys[r] : permuted(*rot.key[r], rot.map[r]);
    }
    if (shared_digits) sh.lds_digits = c_.lds_digits && rot.tiles_in_place ? 1 : 0;
}

// A merged rotation sum from its digits on: o.out = ModDown(sum_r sigma_r(<digits_r, key_r>)) + sum_r sigma_r(c0_r) (+ o.post).  sh: the
// prepared shape (strides, set_rotations, rot_ext_stride / rot_input_stride / ext_batch_stride as the caller's layout needs them); ext:
// the digits from modup; base: the ciphertexts, c0 of batch row b at base + b * c0_stride and c1 one polynomial further.  All rotated
// inner products are gathered and accumulated in the extended basis, and the inner product gathers the c0 parts too: into accQ times P
// where the one ModDown finishes in the row pass, else for moddown_finish to gather (sh.gsrc).
void Evaluator::rotation_sum(KsShape& sh, const u64* ext, const u64* base, size_t c0_stride, const KsOut& o) {
    const KsTail tail = moddown_tail(KsOutput::MergedSum);
    sh.gsrc = base;
    sh.gsrc_stride = c0_stride;
    if (tail == KsTail::RowPass) sh.gsrc_pmod = c_.d_pmod;
    KsAcc acc = inner_product(sh, ext, nullptr, base + (size_t)sh.ell * c_.N, tail);
    moddown(acc, o);
}

Scratch<u64> Evaluator::debug_ks_accp(const u64* ext, int ell, int batch, const int* indices, int n_rot) {
    const size_t pn = (size_t)ell * c_.N;
    if (ell < 1 || ell > c_.L + 1 || batch < 1 || n_rot < 0 || n_rot > (int)KsShape::MAX_ROT) throw Error(FHELIN_ERR_ARG, "debug_ks_accp: bad shape");
    if (!n_rot && !relin_key) throw Error(FHELIN_ERR_KEY, "debug_ks_accp: no relinearisation key");
    if (!n_rot) bind_key(*relin_key, ell);
    KsShape sh = ks_shape(ell, batch, {pn});
    Scratch<u64> own = c_.scratch<u64>((size_t)batch * pn);    // the Q limbs' own-digit operand: the Q half is computed and dropped
    hip_check(hipMemsetAsync(own, 0, (size_t)batch * pn * sizeof(u64), c_.stream), "hipMemsetAsync(debug_ks_accp)");
    if (n_rot) set_rotations(sh, rotations(indices, n_rot), true, nullptr);
    KsAcc acc = inner_product(sh, ext, n_rot ? nullptr : relin_key->d, own, KsTail::Finish);
    accp_inverse(acc);
    launch_ok("debug_ks_accp");
    return std::move(acc.accP);
}

void Evaluator::debug_ks_accq(const u64* ext, const u64* own, u64* conv, int ell, int batch, int index, u64* out) {
    const size_t pn = (size_t)ell * c_.N;
    if (ell < 1 || ell > c_.L + 1 || batch < 1) throw Error(FHELIN_ERR_ARG, "debug_ks_accq: bad shape");
    if (!index && !relin_key) throw Error(FHELIN_ERR_KEY, "debug_ks_accq: no relinearisation key");
    if (!index) bind_key(*relin_key, ell);
    KsShape sh = ks_shape(ell, batch, {pn, 2 * pn});
    const u64* evk = index ? nullptr : relin_key->d;
    if (index) {
        const RotKey k = rotation_key(index);
        const EvalKey* key = k.key.get();
        evk = set_gather(sh, &key, &k.map);
    }
    KsAcc acc = inner_product(sh, ext, evk, own, KsTail::RowPass);   // the special-limb half is computed and dropped
    moddown_rows(acc, conv, KsOut{out});
    launch_ok("debug_ks_accq");
}

int Evaluator::slot_count(int slots) const { return slots > 0 ? slots : (1 << c_.prm.log_slots); }

Evaluator::RotKey Evaluator::rotation_key(int index) {
    const u64 g = c_.rot_element(index);
    auto it = rot_keys.find(g);
    if (it == rot_keys.end()) throw Error(FHELIN_ERR_KEY, "no rotation key for index " + std::to_string(index) + " (EvalRotateKeyGen list)");
    return RotKey{it->second, c_.automorph_map(g), g};
}

bool Evaluator::have_rotation_keys(const std::vector<int>& indices, int slots) const {
    const int ns = slot_count(slots);
    for (int r : indices) {
        if (r % ns == 0) return false;
        if (!rot_keys.count(c_.rot_element(r))) return false;
    }
    return !indices.empty();
}

const u64* Evaluator::permuted(const EvalKey& key, const u32* map) {
    if (key.d_perm) return key.d_perm;
    const int nvec = key.digits * 2 * (c_.L + 1 + c_.K);
    key.d_perm = c_.dalloc<u64>(key.words());
    launch_automorph_pack30(c_.dt, key.d_perm, key.d, map, nvec, c_.stream);
    launch_ok("key permutation");
    // built once, read from every stream afterwards: finish it before anyone else can see the pointer
    hip_check(hipStreamSynchronize(c_.stream), "key permutation sync");
    return key.d_perm;
}

std::vector<CtPtr> Evaluator::rotate_sum_batch(const std::vector<CtPtr>& vin, const std::vector<int>& indices) {
    if (vin.empty()) return {};
    const int R = (int)indices.size();
    if (R < 1 || R > KsShape::MAX_ROT) throw Error(FHELIN_ERR_ARG, "rotate_sum_batch: 1..7 rotations");
    if (!have_rotation_keys(indices, vin[0]->slots)) throw Error(FHELIN_ERR_KEY, "rotate_sum_batch: missing rotation key");
    if (c_.K < 1) throw Error(FHELIN_ERR_STATE, "hybrid key switching needs at least one special prime");
    const Rotations rot = rotations(indices.data(), R);
    bind_rotations(rot, vin);
    const size_t N = c_.N;
    return for_groups(vin.size(), batch_limit, [&](size_t f, size_t i) { return same_shape(*vin[f], *vin[i]); },
                      [&](const std::vector<size_t>& idx) {
        if (vin[idx[0]]->npoly != 2) throw Error(FHELIN_ERR_STATE, "rotate: ciphertext must have 2 components");
        const std::vector<CtPtr> chunk = make_contiguous(pick(vin, idx), 0);
        const int B = (int)chunk.size(), ell = chunk[0]->ell;
        const size_t pn = (size_t)ell * N, ctw = 2 * pn;
        std::vector<CtPtr> o = new_ct_batch(B, 2, ell, chunk[0]->deg, chunk[0]->scale, chunk[0]->slots);
        const u64* base = chunk[0]->d;
        KsShape sh = ks_shape(ell, B, {ctw, ctw, pn, ctw});
        set_rotations(sh, rot, true);
        // accounting in units of the reference's rotations: R = 2^k - 1 merged terms stand for k tree steps
        int steps = 0;
        while ((1 << steps) < R + 1) ++steps;
        c_.stats.keyswitch += (u64)B * steps;
        c_.stats.keyswitch_limbs += (u64)B * steps * ell;
        {
            Scratch<u64> ext = modup(sh, base + pn, false);   // of c1, once for all rotations
            rotation_sum(sh, ext, base, ctw, KsOut{o[0]->d, nullptr, nullptr, base});   // one ModDown; its finish adds the unrotated input
            launch_ok("rotate_sum_batch");
        }
        for (int b = 0; b < B; ++b) o[b]->scale = vin[idx[b]]->scale;
        return o;
    });
}

Evaluator::FoldedKey Evaluator::folded_key(const PtPtr& p, int index, long double scale) {
    // the scale must match exactly: the scaling factors of neighbouring levels can lie within 1e-12 of each other (always for
    // ~60-bit scaling primes, whose spacing is 2N / 2^60), and a key folded at another level's scale is a different encoding
    const RotKey rk = rotation_key(index);
    for (size_t i = 0; i < folded_keys.size(); ++i) {
        const FoldedKey& f = folded_keys[i];
        if (f.pt.get() == p.get() && f.key.get() == rk.key.get() && f.index == index && f.scale == scale) {
            FoldedKey hit = f;
            if (i + 1 != folded_keys.size()) {   // least recently used goes first when the cache is full
                folded_keys.erase(folded_keys.begin() + i);
                folded_keys.push_back(hit);
            }
            return hit;
        }
    }
    FoldedKey f;
    f.pt = p;
    f.key = rk.key;
    f.index = index;
    f.scale = scale;
    const int nl = c_.L + 1 + c_.K;
    f.enc = p->at(nl, scale);
    f.d = std::make_shared<DevBlock>();
    f.d->ctx = &c_;
    f.d->d = c_.dalloc<u64>(f.key->words());
    launch_fold_key(c_.dt, f.d->d, f.key->d, rk.map, f.enc->d, f.key->digits * 2 * nl, c_.stream);
    launch_ok("fold_key");
    // built once, read from every stream afterwards: finish it before anyone else can see the pointer
    hip_check(hipStreamSynchronize(c_.stream), "fold_key sync");
    if (folded_keys.size() >= MAX_FOLDED) {
        // the evicted copy may still be read by work in flight on any stream
        hip_check(hipStreamSynchronize(c_.main_stream), "folded key eviction sync");
        for (int k = 1; k <= c_.n_lanes; ++k) hip_check(hipStreamSynchronize(c_.lane_stream[k]), "folded key eviction sync (lane)");
        folded_keys.erase(folded_keys.begin());
    }
    folded_keys.push_back(f);
    return f;
}

std::vector<CtPtr> Evaluator::hoisted_dot_rows(const std::vector<CtPtr>& xin, const std::vector<PtPtr>& pts, const std::vector<int>& indices,
                                              bool rescale_out) {
    if (xin.empty()) return {};
    const int R = (int)indices.size();
    if (R < 1 || R > KsShape::MAX_ROT || (int)pts.size() != R + 1)
        throw Error(FHELIN_ERR_ARG, "hoisted_dot_rows: 1..7 rotations, one plaintext per rotation + the unrotated term's");
    if (!have_rotation_keys(indices, xin[0]->slots)) throw Error(FHELIN_ERR_KEY, "hoisted_dot_rows: missing rotation key");
    if (c_.K < 1) throw Error(FHELIN_ERR_STATE, "hybrid key switching needs at least one special prime");
    const int ns = slot_count(xin[0]);
    for (int r : indices)
        if (r % ns == 0) throw Error(FHELIN_ERR_ARG, "hoisted_dot_rows: a rotation by 0 is the unrotated term (pts[0])");
    if (rescale_out && c_.K + 1 > 16)   // the merged ModDown + rescale takes at most 16 sources: ModDown, then a separate rescale
        return rescale_batch(hoisted_dot_rows(xin, pts, indices, false));
    bind_rotations(rotations(indices.data(), R), xin, true);   // before the operands' rescale and the folded keys
    std::vector<CtPtr> x = xin;
    {   // degree-2 operands are rescaled first (as before any product with a plaintext); a ciphertext that occurs twice is rescaled twice
        std::vector<CtPtr> need;
        std::vector<size_t> pos;
        for (size_t i = 0; i < x.size(); ++i)
            if (x[i]->deg >= 2) {
                need.push_back(x[i]);
                pos.push_back(i);
            }
        if (!need.empty()) {
            std::vector<CtPtr> r = rescale_batch(need);
            for (size_t k = 0; k < pos.size(); ++k) x[pos[k]] = r[k];
        }
    }
    const Rotations rot = rotations(indices.data(), R);
    const size_t N = c_.N;
    const int K = c_.K;
    hipStream_t s = c_.stream;
    return for_groups(x.size(), batch_limit, [&](size_t f, size_t i) { return same_shape(*x[f], *x[i]); },
                      [&](const std::vector<size_t>& idx) {
        if (x[idx[0]]->npoly != 2) throw Error(FHELIN_ERR_STATE, "hoisted_dot_rows: ciphertext must have 2 components");
        const std::vector<CtPtr> chunk = make_contiguous(pick(x, idx), 0);
        const int B = (int)chunk.size(), ell = chunk[0]->ell;
        const size_t pn = (size_t)ell * N, ctw = 2 * pn;
        const long double sf = c_.sf_real[chunk[0]->level()];
        const bool merged = rescale_out && ell >= 2 && K + 1 <= 16;
        if (rescale_out && !merged) throw Error(FHELIN_ERR_STATE, "hoisted_dot_rows: no limb left to drop");
        const int oell = merged ? ell - 1 : ell;
        std::vector<CtPtr> o = new_ct_batch(B, 2, oell, merged ? chunk[0]->deg : chunk[0]->deg + 1, chunk[0]->scale * sf, chunk[0]->slots);
        const u64* base = chunk[0]->d;
        KsShape sh = ks_shape(ell, B, {ctw, (size_t)2 * oell * N, pn, ctw});
        HoistAdd h;
        h.n_rot = R;
        std::vector<FoldedKey> hold;            // the folded keys and encodings of this launch set stay alive across a cache eviction
        const std::shared_ptr<Encoding> e0 = pts[0]->at(ell, sf);
        h.v[0] = e0->d;
        const u64* folded[KsShape::MAX_ROT];
        for (int r = 0; r < R; ++r) {
            hold.push_back(folded_key(pts[r + 1], indices[r], sf));
            folded[r] = hold.back().d->d;
            h.v[r + 1] = hold.back().enc->d;
        }
        set_rotations(sh, rot, true, folded);
        for (int r = 0; r < R; ++r) h.map[r] = sh.map_rot[r];
        c_.stats.keyswitch += (u64)B * R;
        c_.stats.keyswitch_limbs += (u64)B * R * ell;
        c_.stats.ct_pt_mult += (u64)B * (R + 1);
        c_.stats.ct_pt_limbs += (u64)B * (R + 1) * ell;
        if (merged) {
            c_.stats.rescale += (u64)B;
            c_.stats.rescale_limbs += (u64)B * ell;
        }
        {
            Scratch<u64> ext = modup(sh, base + pn, false);   // of c1, once for all rotations
            // sum_r V_r . sigma_r(d * evk_r) in the extended basis: the merged inner product with the folded keys
            KsAcc acc = inner_product(sh, ext, nullptr, base + pn, merged ? KsTail::Rescale : moddown_tail(KsOutput::MergedSum));
            if (!merged) {
                // what does not pass through the key switch: V_0 (c0, c1) + sum_r V_r sigma_r(c0)
                Scratch<u64> pre = c_.scratch<u64>((size_t)B * ctw);
                launch_hoist_addends(c_.dt, sh, h, pre, base, s);
                moddown(acc, KsOut{o[0]->d, nullptr, nullptr, pre});   // one ModDown
            } else {
                // the same addends times P into the accumulator's Q part, then P and the top limb are dropped together
                h.acc = acc.accQ;
                h.pmod = c_.d_pmod;
                launch_hoist_addends(c_.dt, sh, h, nullptr, base, s);
                moddown_rescale(acc, o[0]->d);
            }
            launch_ok("hoisted_dot_rows");
        }
        for (int b = 0; b < B; ++b) {
            o[b]->scale = x[idx[b]]->scale * sf;
            if (merged) o[b]->scale = o[b]->scale / (long double)c_.chain.q[ell - 1];
        }
        return o;
    });
}

int Evaluator::lt_split_cost(const std::vector<int>& idx, int n1) {
    std::set<int> groups, babies;
    for (int d : idx) {
        groups.insert(d - d % n1);
        if (d % n1) babies.insert(d % n1);
    }
    const int n2 = (int)groups.size(), R = n2 - (int)groups.count(0);
    return 4 * (n2 + (R + 6) / 7) + (int)babies.size();
}

std::vector<CtPtr> Evaluator::linear_transform_rows(const std::vector<CtPtr>& xin, const std::vector<std::vector<PtPtr>>& pts,
                                                    const std::vector<int>& baby, const std::vector<int>& giant, bool rescale_out,
                                                    long double pt_scale) {
    const int n1 = (int)baby.size(), n2 = (int)giant.size();
    if (n1 < 1 || n1 > LtDot::MAX_STEPS || n2 < 1 || (int)pts.size() != n2 || baby[0] != 0)
        throw Error(FHELIN_ERR_ARG, "linear_transform_rows: 1..32 baby steps (the first unrotated), >= 1 giant steps, pts [n2][n1]");
    for (const auto& row : pts)
        if ((int)row.size() != n1) throw Error(FHELIN_ERR_ARG, "linear_transform_rows: pts [n2][n1]");
    c_.require_device();
    if (c_.stride != 1) throw Error(FHELIN_ERR_STATE, "linear_transform_rows: interleaved samples (slot stride != 1) are not supported");
    if (c_.K < 1) throw Error(FHELIN_ERR_STATE, "hybrid key switching needs at least one special prime");
    if (xin.empty()) return {};
    const int ns = slot_count(xin[0]);
    // every key the call needs, before anything runs: the baby steps that carry a term, the rotated giant steps
    struct Step {
        int b;
        const EvalKey* key;
        const u32* map;
    };
    std::vector<Step> steps;
    for (int b = 0; b < n1; ++b) {
        bool any = false;
        for (int g = 0; g < n2; ++g) any = any || pts[g][b];
        if (!any) continue;
        if (b > 0 && baby[b] % ns == 0) throw Error(FHELIN_ERR_ARG, "linear_transform_rows: a baby step by 0 is the unrotated term (baby[0])");
        if (b == 0) {
            steps.push_back(Step{0, nullptr, nullptr});
        } else {
            const RotKey rk = rotation_key(baby[b]);
            steps.push_back(Step{b, rk.key.get(), rk.map});
        }
    }
    if (steps.empty()) throw Error(FHELIN_ERR_ARG, "linear_transform_rows: no term");
    // ... and every one of them at the limbs each row will be switched at (a degree-2 row is rescaled first), giant steps included
    for (const CtPtr& xi : xin) {
        const int ell = xi->deg >= 2 ? xi->ell - 1 : xi->ell;
        for (const Step& st : steps)
            if (st.key) bind_key(*st.key, ell);
        for (int g : giant)
            if (g % ns != 0) bind_key(*rotation_key(g).key, ell);
    }
    std::vector<CtPtr> x = xin;
    rescale_degree2(x, nullptr, "linear_transform_rows: ciphertext must have 2 components");   // as before any product with a plaintext
    const size_t N = c_.N;
    const int K = c_.K, nl = c_.L + 1 + K;
    // a plaintext made from residues holds its one encoding over the full key basis: a call that carries one reads every term that way
    bool dense = true;
    for (const auto& row : pts)
        for (const PtPtr& p : row) dense = dense && !(p && p->fixed);
    std::vector<CtPtr> out = for_groups(x.size(), std::max(1, batch_limit / n2), [&](size_t f, size_t i) { return same_shape(*x[f], *x[i]); },
                                        [&](const std::vector<size_t>& idx) {
        const std::vector<CtPtr> chunk = make_contiguous(pick(x, idx), 0);
        const int B = (int)chunk.size(), ell = chunk[0]->ell;
        const size_t pn = (size_t)ell * N, ctw = 2 * pn;
        const long double sf = pt_scale > 0 ? pt_scale : c_.sf_real[chunk[0]->level()];
        // the diagonals at this level's scale (or the caller's), over the rows the kernel reads - Q limbs 0..ell-1, then the special limbs
        // (Plaintext::at_sliced: the residues of the full-basis encoding on those rows): made on first use, kept by the plan's plaintexts
        std::vector<std::shared_ptr<Encoding>> enc((size_t)n2 * n1);
        size_t terms = 0;
        for (int g = 0; g < n2; ++g)
            for (int b = 0; b < n1; ++b)
                if (pts[g][b]) {
                    enc[(size_t)g * n1 + b] = dense ? pts[g][b]->at_sliced(ell, sf) : pts[g][b]->at(nl, sf);
                    ++terms;
                }
        std::vector<CtPtr> o = new_ct_batch(B * n2, 2, ell, chunk[0]->deg + 1, chunk[0]->scale * sf, chunk[0]->slots);
        const u64* base = chunk[0]->d;
        KsShape sh = ks_shape(ell, B, {ctw, ctw, pn, ctw});
        c_.stats.ct_pt_mult += (u64)B * terms;
        c_.stats.ct_pt_limbs += (u64)B * terms * ell;
        {
            Scratch<u64> ext = modup(sh, base + pn, false);   // of c1, once for all baby steps and groups
            // ONE accumulator and ONE ModDown over rows x groups, identity output map
            KsAcc acc = accumulators(ks_shape(ell, B * n2, {ctw, ctw, pn, ctw}), moddown_tail(KsOutput::Identity));
            std::vector<Scratch<u64>> tabs;
            for (int g0 = 0; g0 < n2; g0 += LtStep::MAX_G) {
                LtDot ld;
                ld.n_groups = std::min((int)LtStep::MAX_G, n2 - g0);
                ld.g0 = g0;
                ld.groups = n2;
                ld.pmod = c_.d_pmod;
                ld.dense_v = dense ? 1 : 0;
                std::vector<LtStep> tab;
                for (const Step& st : steps) {
                    LtStep e{};
                    if (st.b) {
                        bind_key(*st.key, ell);
                        e.key = permuted(*st.key, st.map);
                        e.map = st.map;
                    }
                    for (int g = 0; g < ld.n_groups; ++g)
                        if (const auto& v = enc[(size_t)(g0 + g) * n1 + st.b]) {
                            e.v[g] = v->d;
                            e.mask |= 1u << g;
                        }
                    if (e.mask) tab.push_back(e);
                }
                // accounting: a launch forms the key product of each of its rotated steps once per row - with n2 > MAX_G a baby step
                // is counted (and its key streamed) once per launch that carries one of its terms
                u64 rotated = 0;
                for (const LtStep& e : tab) rotated += e.key ? 1 : 0;
                c_.stats.keyswitch += (u64)B * rotated;
                c_.stats.keyswitch_limbs += (u64)B * rotated * ell;
                static_assert(sizeof(LtStep) % sizeof(u64) == 0, "the table is uploaded as 64-bit words");
                if (!tab.empty()) {     // a launch without steps writes the zero sums of its (empty) groups
                    const size_t words = tab.size() * sizeof(LtStep) / sizeof(u64);
                    tabs.push_back(c_.scratch<u64>(words));
                    c_.upload_async(tabs.back(), reinterpret_cast<const u64*>(tab.data()), words);
                    ld.steps = reinterpret_cast<const LtStep*>((const u64*)tabs.back());
                    ld.n_steps = (int)tab.size();
                }
                launch_ks_inner_dot(c_.dt, sh, ld, acc.accQ, acc.accP, ext, base, base + pn, c_.stream);
            }
            moddown(acc, KsOut{o[0]->d});
            launch_ok("linear_transform_rows");
        }
        // the giant steps: sum_g rot(inner_g, giant[g]) as rotate_each_sum forms it - unrotated groups first, then the rotated ones in
        // groups of <= 7 per shared ModDown (a single leftover through a plain rotation), the rows of the chunk in every launch
        std::vector<int> plain, rot;
        for (int g = 0; g < n2; ++g) (giant[g] % ns == 0 ? plain : rot).push_back(g);
        auto rows_of = [&](const std::vector<int>& gs) {
            std::vector<std::vector<CtPtr>> rows(B);
            for (int b = 0; b < B; ++b) {
                for (int g : gs) {
                    o[(size_t)b * n2 + g]->scale = x[idx[b]]->scale * sf;
                    rows[b].push_back(o[(size_t)b * n2 + g]);
                }
            }
            return rows;
        };
        std::vector<CtPtr> acc;
        for (size_t lo = 0; lo == 0 || lo < rot.size(); lo += KsShape::MAX_ROT) {
            std::vector<int> gs = lo == 0 ? plain : std::vector<int>();
            gs.insert(gs.end(), rot.begin() + std::min(lo, rot.size()), rot.begin() + std::min(lo + KsShape::MAX_ROT, rot.size()));
            std::vector<int> gi;
            for (int g : gs) gi.push_back(giant[g]);
            std::vector<CtPtr> t = rotate_each_sum_rows(rows_of(gs), gi);
            acc = acc.empty() ? t : add_batch(acc, t);
        }
        return acc;
    });
    return rescale_out ? rescale_batch(out) : out;
}

CtPtr Evaluator::rotate_each_sum(const std::vector<CtPtr>& vin, const std::vector<int>& indices) {
    if (vin.empty() || vin.size() != indices.size()) throw Error(FHELIN_ERR_ARG, "rotate_each_sum: one index per ciphertext");
    const int ns = slot_count(vin[0]);
    for (size_t i = 0; i < vin.size(); ++i)   // every key at its term's limbs before the first addition or ModUp runs
        if (indices[i] % ns != 0) bind_key(*rotation_key(indices[i]).key, vin[i]->ell);
    // unrotated terms are plain additions; the rest go through the merged key switch in groups of <= 7
    std::vector<CtPtr> rot;
    std::vector<int> ridx;
    CtPtr acc;
    for (size_t i = 0; i < vin.size(); ++i) {
        if (indices[i] % ns == 0) acc = acc ? add(acc, vin[i]) : vin[i];
        else {
            rot.push_back(vin[i]);
            ridx.push_back(indices[i]);
        }
    }
    for (size_t first = 0; first < rot.size(); first += KsShape::MAX_ROT) {
        const int R = (int)std::min(rot.size() - first, (size_t)KsShape::MAX_ROT);
        std::vector<CtPtr> chunk(rot.begin() + first, rot.begin() + first + R);
        bool uniform = have_rotation_keys(std::vector<int>(ridx.begin() + first, ridx.begin() + first + R), ns) && c_.K >= 1;
        for (const CtPtr& c : chunk) uniform = uniform && same_shape(*chunk[0], *c);
        if (!uniform || R < 2) {  // fall back to separate rotations
            for (int r = 0; r < R; ++r) {
                CtPtr t = rotate(chunk[r], ridx[first + r]);
                acc = acc ? add(acc, t) : t;
            }
            continue;
        }
        chunk = make_contiguous(chunk, 1);
        const size_t N = c_.N;
        const int K = c_.K, ell = chunk[0]->ell;
        const size_t pn = (size_t)ell * N, ctw = 2 * pn;
        const LevelTables& lt = c_.lvl[ell];
        const u64* base = chunk[0]->d;
        CtPtr o = new_ct(2, ell, chunk[0]->deg, chunk[0]->scale, chunk[0]->slots);
        {
            // ModUp of the R inputs as one batch
            Scratch<u64> ext = modup(ks_shape(ell, R, {ctw}), base + pn, false);
            // one accumulator for all R rotated inner products, one ModDown
            KsShape sh = ks_shape(ell, 1, {0, ctw, pn});
            sh.rot_ext_stride = (size_t)lt.beta * (ell + K) * N;
            sh.rot_input_stride = ctw;
            set_rotations(sh, rotations(ridx.data() + first, R), false);
            c_.stats.keyswitch += (u64)R;
            c_.stats.keyswitch_limbs += (u64)R * ell;
            rotation_sum(sh, ext, base, 0, KsOut{o->d});
            launch_ok("rotate_each_sum");
        }
        acc = acc ? add(acc, o) : o;
    }
    return acc;
}

std::vector<CtPtr> Evaluator::rotate_each_sum_rows(const std::vector<std::vector<CtPtr>>& rows, const std::vector<int>& indices) {
    if (rows.empty()) return {};
    const int ns = slot_count(rows[0][0]);
    for (const auto& row : rows)   // every key at its term's limbs before the first row runs
        for (size_t r = 0; r < std::min(row.size(), indices.size()); ++r)
            if (indices[r] % ns != 0) bind_key(*rotation_key(indices[r]).key, row[r]->ell);
    std::vector<int> rot_pos, plain_pos, ridx;
    for (size_t r = 0; r < indices.size(); ++r) {
        if (indices[r] % ns == 0) plain_pos.push_back((int)r);
        else {
            rot_pos.push_back((int)r);
            ridx.push_back(indices[r]);
        }
    }
    const int R = (int)rot_pos.size();
    bool uniform = R >= 2 && R <= KsShape::MAX_ROT && have_rotation_keys(ridx, ns) && c_.K >= 1;
    const CtPtr& f = rows[0][0];
    for (const auto& row : rows) {
        uniform = uniform && row.size() == indices.size();
        for (const CtPtr& c : row) uniform = uniform && same_shape(*f, *c);
    }
    std::vector<CtPtr> out(rows.size());
    if (!uniform) {
        for (size_t b = 0; b < rows.size(); ++b) out[b] = rotate_each_sum(rows[b], indices);
        return out;
    }
    const size_t N = c_.N;
    const int K = c_.K, ell = f->ell;
    const size_t pn = (size_t)ell * N, ctw = 2 * pn;
    const LevelTables& lt = c_.lvl[ell];
    const int nt = ell + K;
    const Rotations rot = rotations(ridx.data(), R);
    const size_t chunk_rows = (size_t)std::max(1, batch_limit / 2);   // rows x R polynomials go through one ModUp
    for (size_t lo = 0; lo < rows.size(); lo += chunk_rows) {
        const size_t hi = std::min(rows.size(), lo + chunk_rows);
        const int B = (int)(hi - lo);
        std::vector<CtPtr> flat;
        for (size_t b = lo; b < hi; ++b)
            for (int r : rot_pos) flat.push_back(rows[b][r]);
        // the rotated terms where they stand when every row holds them consecutively and the rows are equally spaced (the groups of
        // a shift sum: seven rotated terms, then the next group's unrotated one): the transforms read them with a row stride;
        // a gather copy otherwise
        size_t row_stride = (size_t)R * ctw;
        bool regular = B >= 1 && flat[0]->block != nullptr;
        for (int b = 0; b < B && regular; ++b) {
            for (int r = 0; r < R && regular; ++r) {
                const CtPtr& c = flat[(size_t)b * R + r];
                regular = c->block == flat[0]->block && c->words() == (size_t)ctw &&
                          c->d == flat[(size_t)b * R]->d + (size_t)r * ctw;
            }
            if (regular && b == 1) {
                regular = flat[R]->d > flat[0]->d;
                if (regular) row_stride = (size_t)(flat[R]->d - flat[0]->d);
            }
            if (regular && b >= 1) regular = flat[(size_t)b * R]->d == flat[0]->d + (size_t)b * row_stride;
        }
        if (!regular) {
            flat = make_contiguous(flat, 2);
            row_stride = (size_t)R * ctw;
        }
        const u64* base = flat[0]->d;
        std::vector<CtPtr> o = new_ct_batch(B, 2, ell, f->deg, f->scale, f->slots);
        {
            const bool spaced = row_stride != (size_t)R * ctw;   // the rows' runs of R terms lie further apart than the terms
            Scratch<u64> ext = modup(ks_shape(ell, B * R, {ctw}), base + pn, false, spaced ? R : 0,
                                     spaced ? row_stride : 0);
            KsShape sh = ks_shape(ell, B, {row_stride, ctw, pn});
            sh.rot_ext_stride = (size_t)lt.beta * nt * N;
            sh.rot_input_stride = ctw;
            sh.ext_batch_stride = (size_t)R * lt.beta * nt * N;
            set_rotations(sh, rot, false);
            c_.stats.keyswitch += (u64)B * R;
            c_.stats.keyswitch_limbs += (u64)B * R * ell;
            rotation_sum(sh, ext, base, row_stride, KsOut{o[0]->d});
            launch_ok("rotate_each_sum_rows");
        }
        for (int b = 0; b < B; ++b) out[lo + b] = o[b];
    }
    // unrotated terms are plain additions, in the order rotate_each_sum adds them: plain terms first, then the rotated sum
    if (!plain_pos.empty()) {
        std::vector<CtPtr> acc(rows.size());
        for (size_t b = 0; b < rows.size(); ++b) acc[b] = rows[b][plain_pos[0]];
        for (size_t k = 1; k < plain_pos.size(); ++k) {
            std::vector<CtPtr> t(rows.size());
            for (size_t b = 0; b < rows.size(); ++b) t[b] = rows[b][plain_pos[k]];
            acc = add_batch(acc, t);
        }
        out = add_batch(acc, out);
    }
    return out;
}

// hoisted rotations of one ciphertext.  A rotation here is KeySwitch_{s -> sigma^-1(s)}(c1) + c0 followed by the NTT-domain
// automorphism gather in the ModDown epilogue, so the ModUp of c1 does not depend on the rotation index: it is computed
// once and every index runs only its own inner product + ModDown.  Bit-identical to rotate(a, i).
std::vector<CtPtr> Evaluator::rotate_many(const CtPtr& a, const std::vector<int>& indices) {
    if (a->npoly != 2) throw Error(FHELIN_ERR_STATE, "rotate: ciphertext must have 2 components");
    const int ns = slot_count(a);
    std::vector<CtPtr> out(indices.size());
    std::vector<size_t> todo;
    for (size_t i = 0; i < indices.size(); ++i) {
        if (indices[i] % ns == 0) out[i] = a;
        else todo.push_back(i);
    }
    for (size_t i : todo) bind_key(*rotation_key(indices[i]).key, a->ell);   // all of them before the first chunk runs
    const size_t pn = (size_t)a->ell * c_.N, ctw = 2 * pn;
    for (size_t first = 0; first < todo.size(); first += KsShape::MAX_ROWS) {
        const int B = (int)std::min(todo.size() - first, (size_t)KsShape::MAX_ROWS);
        if (B == 1) {
            out[todo[first]] = rotate(a, indices[todo[first]]);
            continue;
        }
        KsRows rows;
        rows.shared_input = true;
        for (int b = 0; b < B; ++b) {
            const RotKey k = rotation_key(indices[todo[first + b]]);
            rows.keys.push_back(k.key.get());
            rows.maps.push_back(k.map);
        }
        std::vector<CtPtr> o = new_ct_batch(B, 2, a->ell, a->deg, a->scale, a->slots);
        keyswitch_rows(rows, a->d + pn, 0, a->ell, o[0]->d, ctw, a->d, 0);
        for (int b = 0; b < B; ++b) out[todo[first + b]] = o[b];
    }
    return out;
}

std::vector<CtPtr> Evaluator::rotate_each(const std::vector<CtPtr>& vin, const std::vector<int>& indices) {
    if (vin.size() != indices.size()) throw Error(FHELIN_ERR_ARG, "rotate_each: one index per ciphertext");
    // an operand that is not rotated is copied and joins no group
    auto rotated = [&](size_t f, size_t i) { return indices[i] % slot_count(vin[f]) != 0; };
    for (size_t i = 0; i < vin.size(); ++i)   // every key at its operand's limbs before the first group runs
        if (rotated(i, i)) bind_key(*rotation_key(indices[i]).key, vin[i]->ell);
    return for_groups(vin.size(), std::min(batch_limit, (int)KsShape::MAX_ROWS),
                      [&](size_t f, size_t i) { return rotated(f, f) && rotated(f, i) && same_shape(*vin[f], *vin[i]); },
                      [&](const std::vector<size_t>& idx) {
        const CtPtr& a = vin[idx[0]];
        if (a->npoly != 2) throw Error(FHELIN_ERR_STATE, "rotate: ciphertext must have 2 components");
        if (!rotated(idx[0], idx[0])) return std::vector<CtPtr>{clone(a)};
        if (idx.size() < 2) return std::vector<CtPtr>{rotate(a, indices[idx[0]])};
        KsRows rows;
        for (size_t i : idx) {
            const RotKey k = rotation_key(indices[i]);
            rows.keys.push_back(k.key.get());
            rows.maps.push_back(k.map);
        }
        const std::vector<CtPtr> chunk = make_contiguous(pick(vin, idx), 3);
        const int B = (int)chunk.size();
        const size_t pn = (size_t)a->ell * c_.N, ctw = 2 * pn;
        std::vector<CtPtr> o = new_ct_batch(B, 2, a->ell, a->deg, a->scale, a->slots);
        keyswitch_rows(rows, chunk[0]->d + pn, ctw, a->ell, o[0]->d, ctw, chunk[0]->d, ctw);
        for (int b = 0; b < B; ++b) o[b]->scale = vin[idx[b]]->scale;
        return o;
    });
}

// ------------------------------------------------------------------------------------------------ raw ops
// K5 steps 2+3: NTT of the centred lift of `last` ([P][N], coefficients modulo q_{ell-1}) into the ell-1 remaining limbs of
// each polynomial -> lifted [P][ell-1][N].  The lift rides in the load of the transform's first pass (LimbBatch::lift_qlm)
// when the dropped modulus is below twice every remaining one (x mod q_j is then one conditional subtraction); otherwise,
// or with FHELIN_FUSE_LIFT=0, the separate lift kernel runs first.  Same residues either way.
void Evaluator::lift_and_ntt(u64* lifted, const u64* last, int P, int ell, const NttEpilogue* ep, const u64* qlm_row) {
    auto ntt = [&](const LimbBatch& b) {
        if (ep)
            c_.ntt_epilogue(b, *ep);
        else
            c_.ntt(b, false);
    };
    const u64* qlm = qlm_row ? qlm_row : c_.d_qlmod + (size_t)(ell - 1) * (c_.L + 1);
    bool fuse = c_.fuse_lift;
    for (int j = 0; j + 1 < ell && fuse; ++j) fuse = c_.moduli[ell - 1] < 2 * c_.chain.q[j];
    if (fuse) {
        LimbBatch fb{lifted, P * (ell - 1), nullptr, 0, ell - 1, last};
        fb.lift_qlm = qlm;
        fb.lift_limb = ell - 1;
        ntt(fb);
        return;
    }
    launch_rescale_lift(c_.dt, lifted, last, P, ell, qlm, c_.stream);
    ntt(LimbBatch{lifted, P * (ell - 1), nullptr, 0, ell - 1});
}

// K5 step 4 rides in the row pass of the lift's NTT (FHELIN_FUSE_FINISH=0: rescale_finish_kernel reads the stored transform)
void Evaluator::rescale_finish(u64* out, const u64* c, const u64* last, int P, int ell, const u64* qlinv_row, const u64* qlm_row) {
    const size_t N = c_.N;
    const u64* qlinv = qlinv_row ? qlinv_row : c_.d_qlinv + (size_t)(ell - 1) * (c_.L + 1) * 2;
    Scratch<u64> lifted = c_.scratch<u64>((size_t)P * (ell - 1) * N);
    if (c_.fuse_finish) {
        NttEpilogue ep;
        ep.acc = c;
        ep.acc_poly_stride = (size_t)ell * N;
        ep.out = out;
        ep.out_stride = (size_t)2 * (ell - 1) * N;
        ep.w = qlinv;
        ep.ell = ell - 1;
        lift_and_ntt(lifted, last, P, ell, &ep, qlm_row);
    } else {
        lift_and_ntt(lifted, last, P, ell, nullptr, qlm_row);
        launch_rescale_finish(c_.dt, out, c, lifted, P, ell, qlinv, c_.stream);
    }
}

CtPtr Evaluator::raw_rescale(const CtPtr& a) {
    const int ell = a->ell, P = a->npoly;
    if (ell < 2) throw Error(FHELIN_ERR_STATE, "rescale: no limb left to drop");
    const size_t N = c_.N;
    Scratch<u64> last = c_.scratch<u64>((size_t)P * N);
    c_.stats.rescale += 1;
    c_.stats.rescale_limbs += (u64)ell;
    {
        // INTT of the last limb of every polynomial, read in place (stride = one polynomial), written densely
        LimbBatch lb{last, P, nullptr, ell - 1, 1, a->d + (size_t)(ell - 1) * N};
        lb.src_group = 1;
        lb.src_group_stride = (size_t)ell * N;
        c_.ntt(lb, true);
    }
    CtPtr o = new_ct(P, ell - 1, a->deg, a->scale, a->slots);
    rescale_finish(o->d, a->d, last, P, ell);
    launch_ok("rescale");
    return o;
}

CtPtr Evaluator::raw_rotate(const CtPtr& a, u64 g, const EvalKey& key, bool accumulate, const u32* map) {
    if (a->npoly != 2) throw Error(FHELIN_ERR_STATE, "rotate: ciphertext must have 2 components");
    const size_t pn = (size_t)a->ell * c_.N;
    CtPtr o = new_ct(2, a->ell, a->deg, a->scale, a->slots);
    // accumulate: out = a + rot(a) — the addition of the rotate-and-sum step rides in the ModDown epilogue
    keyswitch(a->d + pn, a->ell, key, o->d, a->d, nullptr, map ? map : c_.automorph_map(g), accumulate ? a->d : nullptr);
    return o;
}

std::vector<CtPtr> Evaluator::rotate_batch(const std::vector<CtPtr>& vin, int index) { return rotate_batch_impl(vin, index, false); }
std::vector<CtPtr> Evaluator::rotate_add_batch(const std::vector<CtPtr>& vin, int index) { return rotate_batch_impl(vin, index, true); }

std::vector<CtPtr> Evaluator::rotate_batch_impl(const std::vector<CtPtr>& vin, int index, bool accumulate) {
    if (vin.empty()) return {};
    const int ns = slot_count(vin[0]);
    std::vector<CtPtr> out(vin.size());
    if (vin.size() == 1 || index % ns == 0) {
        for (size_t i = 0; i < vin.size(); ++i) out[i] = accumulate ? rotate_add(vin[i], index) : rotate(vin[i], index);
        return out;
    }
    const RotKey k = rotation_key(index);
    return rotate_galois_batch(vin, k.g, *k.key, accumulate);
}

std::vector<CtPtr> Evaluator::conjugate_batch(const std::vector<CtPtr>& v) {
    if (!conj_key) throw Error(FHELIN_ERR_KEY, "no conjugation key");
    return rotate_galois_batch(v, 2ull * c_.N - 1, *conj_key, false);
}

std::vector<CtPtr> Evaluator::rotate_galois_batch(const std::vector<CtPtr>& vin, u64 g, const EvalKey& key, bool accumulate) {
    for (const CtPtr& x : vin) bind_key(key, x->ell);   // before the first group runs
    if (vin.size() == 1) return {raw_rotate(vin[0], g, key, accumulate)};
    // rows that share (level, degree, scale) go through one batched key switch; others form their own groups
    return keyswitch_groups(vin, key, c_.automorph_map(g), accumulate, false, "rotate: ciphertext must have 2 components");
}

CtPtr Evaluator::switch_key(const CtPtr& a, const EvalKey& key) {
    if (a->npoly != 2) throw Error(FHELIN_ERR_STATE, "switch_key: ciphertext must have 2 components");
    const size_t pn = (size_t)a->ell * c_.N;
    CtPtr o = new_ct(2, a->ell, a->deg, a->scale, a->slots);
    keyswitch(a->d + pn, a->ell, key, o->d, a->d, nullptr, nullptr);
    return o;
}

std::vector<CtPtr> Evaluator::switch_key_batch(const std::vector<CtPtr>& vin, const EvalKey& key) {
    for (const CtPtr& x : vin) bind_key(key, x->ell);   // before the first group runs
    if (vin.size() == 1) return {switch_key(vin[0], key)};
    // the switch reads neither degree nor scale: rows of one limb count share the launches (the items of a bootstrap batch in front of
    // their rescale to q0 carry a scale each), and every output keeps its input's bookkeeping
    return keyswitch_groups(vin, key, nullptr, false, true, "switch_key: ciphertext must have 2 components");
}

// (c0 + KS(c1)[0], KS(c1)[1]) of every row, written through `map` (null: the identity), one batched key switch per group of rows.  A group
// is the rows of one shape (same_shape), or with by_limbs those of one limb count, each output then keeping its own degree and slots too
std::vector<CtPtr> Evaluator::keyswitch_groups(const std::vector<CtPtr>& vin, const EvalKey& key, const u32* map, bool accumulate, bool by_limbs,
                                               const char* two_components) {
    return for_groups(vin.size(), batch_limit,
                      [&](size_t f, size_t i) { return by_limbs ? vin[f]->npoly == vin[i]->npoly && vin[f]->ell == vin[i]->ell : same_shape(*vin[f], *vin[i]); },
                      [&](const std::vector<size_t>& idx) {
        if (vin[idx[0]]->npoly != 2) throw Error(FHELIN_ERR_STATE, two_components);
        const std::vector<CtPtr> chunk = make_contiguous(pick(vin, idx), 4);
        const int B = (int)chunk.size();
        const int ell = chunk[0]->ell;
        const size_t pn = (size_t)ell * c_.N, ctw = 2 * pn;
        std::vector<CtPtr> o = new_ct_batch(B, 2, ell, chunk[0]->deg, chunk[0]->scale, chunk[0]->slots);
        const u64* base = chunk[0]->d;  // contiguous by construction (or a single ciphertext)
        keyswitch_batch(B, base + pn, ctw, ell, key, o[0]->d, ctw, base, nullptr, ctw, map, accumulate ? base : nullptr, ctw);
        for (int b = 0; b < B; ++b) {
            o[b]->scale = vin[idx[b]]->scale;
            if (by_limbs) {
                o[b]->deg = vin[idx[b]]->deg;
                o[b]->slots = vin[idx[b]]->slots;
            }
        }
        return o;
    });
}

std::vector<std::vector<CtPtr>> Evaluator::rotate_many_batch(const std::vector<CtPtr>& xs, const std::vector<int>& indices) {
    std::vector<std::vector<CtPtr>> out(xs.size());
    if (xs.empty()) return out;
    bool uniform = xs.size() >= 2 && !c_.fuse_moddown && c_.K >= 1;
    for (const CtPtr& x : xs)
        uniform = uniform && x->npoly == 2 && x->ell == xs[0]->ell && x->deg == xs[0]->deg && x->slots == xs[0]->slots;
    if (!uniform) {
        for (const CtPtr& x : xs)   // every key at every input's limbs before the first input runs
            for (int r : indices)
                if (r % slot_count(x) != 0) bind_key(*rotation_key(r).key, x->ell);
        for (size_t i = 0; i < xs.size(); ++i) out[i] = rotate_many(xs[i], indices);
        return out;
    }
    const int ns = slot_count(xs[0]);
    std::vector<size_t> todo;
    for (size_t i = 0; i < xs.size(); ++i) out[i].resize(indices.size());
    for (size_t k = 0; k < indices.size(); ++k) {
        if (indices[k] % ns == 0)
            for (size_t i = 0; i < xs.size(); ++i) out[i][k] = xs[i];
        else
            todo.push_back(k);
    }
    const int R = (int)todo.size();
    if (R == 0) return out;
    // the rotations gather at the inner product when ONE launch covers every index (KsShape::ginv_row); more than MAX_ROWS indices keep
    // the finishing kernel, which takes its rows in slices
    const bool gather = rot_in_gather() && R <= (int)KsShape::MAX_ROWS;
    std::vector<const EvalKey*> keys;
    std::vector<const u32*> maps;
    for (size_t k : todo) {
        const RotKey rk = rotation_key(indices[k]);
        bind_key(*rk.key, xs[0]->ell);   // the rows' keys go into the shapes below as pointers (row_keys): bound here, before any pass
        keys.push_back(rk.key.get());
        maps.push_back(rk.map);
    }
    const size_t N = c_.N;
    const int K = c_.K, ell = xs[0]->ell;
    const size_t pn = (size_t)ell * N, ctw = 2 * pn;
    const LevelTables& lt = c_.lvl[ell];
    const int nt = ell + K;
    hipStream_t s = c_.stream;
    // inputs per pass: the ModDown of a pass works on (inputs x R) rows
    const size_t per_pass = (size_t)std::max(1, 160 / R);
    for (size_t lo = 0; lo < xs.size(); lo += per_pass) {
        const size_t hi = std::min(xs.size(), lo + per_pass);
        const int B = (int)(hi - lo);
        std::vector<CtPtr> in = make_contiguous(std::vector<CtPtr>(xs.begin() + lo, xs.begin() + hi), 6);
        const u64* base = in[0]->d;
        const int rows = B * R;
        c_.stats.keyswitch += (u64)rows;
        c_.stats.keyswitch_limbs += (u64)rows * ell;
        std::vector<CtPtr> o = new_ct_batch(rows, 2, ell, xs[lo]->deg, xs[lo]->scale, xs[lo]->slots);
        {
            // ModUp of the B inputs' c1, once; digits times 2^64 for the keys as they are stored: launch_ks_inner ends in redc128
            Scratch<u64> ext = modup(ks_shape(ell, B, {ctw}), base + pn, !gather);
            // inner products: per input, rows of <= MAX_ROWS indices with their own keys, all reading that input's digits
            auto row_keys = [&](KsShape sh, int first, int cnt) {
                sh.per_row = 1;
                sh.shared_input = 1;
                for (int b = 0; b < cnt; ++b) {
                    sh.evk_row[b] = keys[first + b]->d;
                    sh.map_row[b] = maps[first + b];
                }
                return sh;
            };
            // ONE launch per chunk of <= MAX_ROWS indices over ALL inputs (KsShape::row_mod): row (i, r) = rotation r of input i; in the
            // XCD-aware block order a key tile is fetched once for all inputs and a digit tile once for all indices
            auto row_shape = [&](int first, int cnt) {
                KsShape sh = row_keys(ks_shape(ell, B * cnt, {ctw, ctw, ctw}), first, cnt);
                sh.row_mod = cnt;
                sh.ext_batch_stride = (size_t)lt.beta * nt * N;
                return sh;
            };
            // R > MAX_ROWS: per input and per chunk of <= MAX_ROWS indices, launch(shape, first row of the chunk, input)
            auto for_row_chunks = [&](auto&& launch) {
                for (int i = 0; i < B; ++i)
                    for (int first = 0; first < R; first += KsShape::MAX_ROWS) {
                        const int cnt = std::min(R - first, (int)KsShape::MAX_ROWS);
                        launch(row_keys(ks_shape(ell, cnt, {0, ctw}), first, cnt), (size_t)i * R + first, i);
                    }
            };
            const bool one_chunk = R <= (int)KsShape::MAX_ROWS;     // rows then lie [input][index] as the outputs do
            if (gather) {
                // every row gathers through its map at the inner product (its input's c0 included, times P); ONE identity ModDown over all rows
                KsShape sh = row_shape(0, R);
                set_gather(sh, keys.data(), maps.data(), base, ctw);
                KsAcc acc = inner_product(sh, ext, nullptr, base + pn, moddown_tail(KsOutput::Gathered));
                moddown(acc, KsOut{o[0]->d});
            } else {
                // ONE ModDown over all rows up to its finish, which takes them in slices and adds the input's c0 (gathered through each row's map)
                KsAcc acc = accumulators(ks_shape(ell, rows, {0, ctw}), KsTail::Finish);
                if (one_chunk) launch_ks_inner(c_.dt, row_shape(0, R), acc.accQ, acc.accP, ext, nullptr, base + pn, s);
                else
                    for_row_chunks([&](const KsShape& sh1, size_t row0, int i) {
                        launch_ks_inner(c_.dt, sh1, acc.accQ + row0 * 2 * ell * N, acc.accP + row0 * 2 * K * N,
                                        ext + (size_t)i * lt.beta * nt * N, nullptr, base + pn + (size_t)i * ctw, s);
                    });
                Scratch<u64> conv = moddown_conv(acc);
                if (one_chunk) launch_moddown_finish(c_.dt, row_shape(0, R), o[0]->d, acc.accQ, conv, c_.d_pinv, base, nullptr, nullptr, nullptr, s);
                else
                    for_row_chunks([&](const KsShape& sh1, size_t row0, int i) {
                        // add_stride 0 = the same c0 for every row
                        launch_moddown_finish(c_.dt, sh1, o[row0]->d, acc.accQ + row0 * 2 * ell * N, conv + row0 * 2 * ell * N, c_.d_pinv,
                                              base + (size_t)i * ctw, nullptr, nullptr, nullptr, s);
                    });
            }
            launch_ok("rotate_many_batch");
        }
        for (int i = 0; i < B; ++i)
            for (int r = 0; r < R; ++r) {
                o[(size_t)i * R + r]->scale = xs[lo + i]->scale;
                out[lo + i][todo[r]] = o[(size_t)i * R + r];
            }
    }
    return out;
}

// rescale of many ciphertexts of identical shape as ONE polynomial batch [2B][ell][N] (K5 kernels are per polynomial)
std::vector<CtPtr> Evaluator::rescale_batch(const std::vector<CtPtr>& vin) {
    return for_groups(vin.size(), batch_limit,
                      [&](size_t f, size_t i) { return vin[i]->npoly == 2 && vin[f]->npoly == 2 && vin[i]->ell == vin[f]->ell; },
                      [&](const std::vector<size_t>& idx) {
        if (idx.size() < 2) return std::vector<CtPtr>{rescale(vin[idx[0]])};
        const std::vector<CtPtr> chunk = make_contiguous(pick(vin, idx), 5);
        const int B = (int)chunk.size(), ell = chunk[0]->ell, P = 2 * B;
        if (ell < 2) throw Error(FHELIN_ERR_STATE, "rescale: no limb left to drop");
        const size_t N = c_.N;
        const u64* base = chunk[0]->d;
        Scratch<u64> last = c_.scratch<u64>((size_t)P * N);
        c_.stats.rescale += (u64)B;
        c_.stats.rescale_limbs += (u64)B * ell;
        LimbBatch lb{last, P, nullptr, ell - 1, 1, base + (size_t)(ell - 1) * N};
        lb.src_group = 1;
        lb.src_group_stride = (size_t)ell * N;
        c_.ntt(lb, true);
        std::vector<CtPtr> o = new_ct_batch(B, 2, ell - 1, 1, 0, chunk[0]->slots);
        rescale_finish(o[0]->d, base, last, P, ell);
        launch_ok("rescale_batch");
        last.reset();
        for (int b = 0; b < B; ++b) {
            const CtPtr& a = vin[idx[b]];
            o[b]->scale = a->scale / (long double)c_.chain.q[ell - 1];
            o[b]->deg = a->deg > 1 ? a->deg - 1 : 1;
        }
        return o;
    });
}

std::vector<CtPtr> Evaluator::mult_plain_batch(const std::vector<CtPtr>& vin, const PtPtr& p) {
    return mult_plain_each(vin, std::vector<PtPtr>(vin.size(), p));
}

std::vector<CtPtr> Evaluator::mult_plain_each(const std::vector<CtPtr>& vin, const std::vector<PtPtr>& p) {
    if (vin.size() != p.size()) throw Error(FHELIN_ERR_ARG, "mult_plain_each: one plaintext per ciphertext");
    if (vin.empty()) return {};
    // degree-2 operands are rescaled first (as in mult_plain); the same ciphertext may occur many times (one
    // container masked 128 ways): every distinct one once
    std::vector<CtPtr> x = vin;
    rescale_degree2(x);
    std::vector<CtPtr> out(x.size());
    // operands of one shape: ONE output block for all products, so that any sub-range a later batched key switch takes is
    // contiguous as it stands (no gather copies); the launches still go in runs of MAX_ITEMS
    bool one_shape = x.size() > 1;
    for (const CtPtr& c : x) one_shape = one_shape && c->npoly == x[0]->npoly && c->ell == x[0]->ell && c->deg == x[0]->deg;
    std::vector<CtPtr> all;
    if (one_shape) all = new_ct_batch((int)x.size(), x[0]->npoly, x[0]->ell, x[0]->deg + 1, x[0]->scale, x[0]->slots);
    for_runs(x.size(), [&](size_t a, size_t b) { return x[a]->npoly == x[b]->npoly && x[a]->ell == x[b]->ell && x[a]->deg == x[b]->deg; },
             [&](size_t lo, size_t hi) {
                 const CtPtr& f = x[lo];
                 std::vector<CtPtr> o = one_shape ? std::vector<CtPtr>(all.begin() + lo, all.begin() + hi)
                                                  : new_ct_batch((int)(hi - lo), f->npoly, f->ell, f->deg + 1, f->scale, f->slots);
                 EwItems it;
                 it.n = (int)(hi - lo);
                 it.vecs = f->npoly * f->ell;
                 it.b_vecs = f->ell;
                 for (size_t i = lo; i < hi; ++i) {
                     auto enc = p[i]->at(x[i]->ell, c_.sf_real[x[i]->level()]);
                     o[i - lo]->scale = x[i]->scale * enc->scale;
                     it.out[i - lo] = o[i - lo]->d;
                     it.a[i - lo] = x[i]->d;
                     it.b[i - lo] = enc->d;
                     out[i] = o[i - lo];
                 }
                 launch_ew_items(c_.dt, it, 0, f->ell, c_.stream);
                 c_.stats.ct_pt_mult += (u64)(hi - lo);
                 c_.stats.ct_pt_limbs += (u64)(hi - lo) * f->ell;
             });
    launch_ok("mult_plain_each");
    return out;
}

CtPtr Evaluator::dot_plain(const std::vector<CtPtr>& vin, const std::vector<PtPtr>& p, long double pt_scale, const CtPtr& dest) {
    if (vin.size() != p.size() || vin.empty()) throw Error(FHELIN_ERR_ARG, "dot_plain: one plaintext per ciphertext, at least one term");
    // degree-2 operands are rescaled first, every distinct ciphertext once (as mult_plain does)
    std::vector<CtPtr> x = vin;
    rescale_degree2(x);
    bool uniform = x.size() >= 2;
    for (const CtPtr& c : x)   // any component count, as long as it is the first operand's
        uniform = uniform && c->npoly == x[0]->npoly && c->ell == x[0]->ell && c->deg == x[0]->deg && same_scale(*x[0], *c);
    if (!uniform) {
        if (pt_scale > 0) throw Error(FHELIN_ERR_ARG, "dot_plain: an explicit plaintext scale needs uniform operands");
        std::vector<CtPtr> prod = mult_plain_each(x, p);
        CtPtr acc = prod[0];
        for (size_t i = 1; i < prod.size(); ++i) acc = add(acc, prod[i]);
        return acc;
    }
    const CtPtr& f = x[0];
    const long double sf = pt_scale > 0 ? pt_scale : c_.sf_real[f->level()];
    CtPtr acc;
    for (size_t lo = 0; lo < x.size(); lo += EwItems::MAX_ITEMS) {
        const size_t hi = std::min(x.size(), lo + (size_t)EwItems::MAX_ITEMS);
        EwItems it;
        it.n = (int)(hi - lo);
        it.vecs = f->npoly * f->ell;
        it.b_vecs = f->ell;
        for (size_t i = lo; i < hi; ++i) {
            it.a[i - lo] = x[i]->d;
            it.b[i - lo] = p[i]->at(f->ell, sf)->d;
        }
        // a caller that will hand several such sums to one batched key switch provides their common block (dest)
        const bool into_dest = dest && x.size() <= (size_t)EwItems::MAX_ITEMS && dest->npoly == f->npoly && dest->ell == f->ell;
        CtPtr o = into_dest ? dest : new_ct(f->npoly, f->ell, f->deg + 1, f->scale * sf, f->slots);
        if (into_dest) {
            o->deg = f->deg + 1;
            o->scale = f->scale * sf;
            o->slots = f->slots;
        }
        launch_ew_dot(c_.dt, o->d, it, f->ell, c_.stream);
        c_.stats.ct_pt_mult += (u64)(hi - lo);
        c_.stats.ct_pt_limbs += (u64)(hi - lo) * f->ell;
        acc = acc ? add(acc, o) : o;
    }
    launch_ok("dot_plain");
    return acc;
}

bool Evaluator::dot_plain_groups(const std::vector<CtPtr>& cts, const std::vector<std::vector<PtPtr>>& pts, long double pt_scale,
                                 const std::vector<CtPtr>& dest) {
    if (!dot_groups || cts.empty() || cts.size() > (size_t)EwDotGroups::MAX_A || pts.empty() || pts.size() > (size_t)EwDotGroups::MAX_G ||
        dest.size() != pts.size())
        return false;
    const CtPtr& f = cts[0];
    for (const CtPtr& c : cts)
        if (c->deg != 1 || !same_shape(*f, *c)) return false;
    for (const CtPtr& o : dest)
        if (!o || o->npoly != 2 || o->ell != f->ell) return false;
    const long double sf = pt_scale > 0 ? pt_scale : c_.sf_real[f->level()];
    EwDotGroups d;
    d.na = (int)cts.size();
    d.ng = (int)pts.size();
    d.ell = f->ell;
    for (int b = 0; b < d.na; ++b) d.a[b] = cts[b]->d;
    u64 terms = 0;
    for (int g = 0; g < d.ng; ++g) {
        if (pts[g].size() != cts.size()) return false;
        for (int b = 0; b < d.na; ++b) {
            d.p[g][b] = pts[g][b] ? pts[g][b]->at(f->ell, sf)->d : nullptr;
            terms += pts[g][b] ? 1 : 0;
        }
        d.out[g] = dest[g]->d;
        dest[g]->deg = f->deg + 1;
        dest[g]->scale = f->scale * sf;
        dest[g]->slots = f->slots;
    }
    launch_ew_dot_groups(c_.dt, d, c_.stream);
    launch_ok("dot_plain_groups");
    c_.stats.ct_pt_mult += terms;
    c_.stats.ct_pt_limbs += terms * (u64)f->ell;
    return true;
}

bool Evaluator::dot_plain_groups_batch(const std::vector<std::vector<CtPtr>>& cts, const std::vector<std::vector<PtPtr>>& pts, long double pt_scale,
                                       const std::vector<std::vector<CtPtr>>& dest) {
    const size_t nb = cts.size();
    if (!dot_groups || nb < 2 || dest.size() != nb || cts[0].empty() || cts[0].size() > (size_t)EwDotGroups::MAX_A || pts.empty() ||
        pts.size() > (size_t)EwDotGroups::MAX_G)
        return false;
    const size_t na = cts[0].size(), ng = pts.size();
    const CtPtr& f = cts[0][0];
    for (size_t x = 0; x < nb; ++x) {
        if (cts[x].size() != na || dest[x].size() != ng) return false;
        for (const CtPtr& c : cts[x])
            if (c->deg != 1 || !same_shape(*f, *c)) return false;
        for (const CtPtr& o : dest[x])
            if (!o || o->npoly != 2 || o->ell != f->ell) return false;
    }
    EwDotGroups d;
    d.na = (int)na;
    d.ng = (int)ng;
    d.ell = f->ell;
    d.nbatch = (int)nb;
    // equally spaced over the batch, ascending addresses
    for (size_t b = 0; b < na; ++b) {
        if (cts[1][b]->d <= cts[0][b]->d) return false;
        const size_t st = (size_t)(cts[1][b]->d - cts[0][b]->d);
        for (size_t x = 0; x < nb; ++x)
            if (cts[x][b]->d != cts[0][b]->d + x * st) return false;
        d.a[b] = cts[0][b]->d;
        d.a_stride[b] = st;
    }
    for (size_t g = 0; g < ng; ++g) {
        if (dest[1][g]->d <= dest[0][g]->d) return false;
        const size_t st = (size_t)(dest[1][g]->d - dest[0][g]->d);
        for (size_t x = 0; x < nb; ++x)
            if (dest[x][g]->d != dest[0][g]->d + x * st) return false;
        d.out[g] = dest[0][g]->d;
        d.out_stride[g] = st;
    }
    const long double sf = pt_scale > 0 ? pt_scale : c_.sf_real[f->level()];
    u64 terms = 0;
    std::vector<std::shared_ptr<Encoding>> hold;
    for (size_t g = 0; g < ng; ++g) {
        if (pts[g].size() != na) return false;
        for (size_t b = 0; b < na; ++b) {
            if (pts[g][b]) {
                hold.push_back(pts[g][b]->at(f->ell, sf));
                d.p[g][b] = hold.back()->d;
                ++terms;
            } else {
                d.p[g][b] = nullptr;
            }
        }
        for (size_t x = 0; x < nb; ++x) {
            dest[x][g]->deg = f->deg + 1;
            dest[x][g]->scale = cts[x][0]->scale * sf;
            dest[x][g]->slots = f->slots;
        }
    }
    launch_ew_dot_groups(c_.dt, d, c_.stream);
    launch_ok("dot_plain_groups_batch");
    c_.stats.ct_pt_mult += terms * nb;
    c_.stats.ct_pt_limbs += terms * nb * (u64)f->ell;
    return true;
}

bool Evaluator::dot_plain_cyclic(const std::vector<CtPtr>& cts, const std::vector<PtPtr>& pts, const std::vector<CtPtr>& dest) {
    constexpr int P = EwCyclic::PERIOD;
    if (cts.empty() || (int)cts.size() > P || (int)pts.size() != P || (int)dest.size() != P) return false;
    const CtPtr& f = cts[0];
    for (const CtPtr& c : cts)
        if (c->deg != 1 || !same_shape(*f, *c)) return false;
    for (const CtPtr& o : dest)
        if (!o || o->npoly != 2 || o->ell != f->ell) return false;
    const long double sf = c_.sf_real[f->level()];
    EwCyclic d;
    d.n = (int)cts.size();
    d.ell = f->ell;
    std::vector<std::shared_ptr<Encoding>> hold;
    for (int j = 0; j < P; ++j) {
        hold.push_back(pts[j]->at(f->ell, sf));
        d.m[j] = hold.back()->d;
        d.a[j] = j < d.n ? cts[j]->d : nullptr;
        d.out[j] = dest[j]->d;
        dest[j]->deg = f->deg + 1;
        dest[j]->scale = f->scale * sf;
        dest[j]->slots = f->slots;
    }
    launch_ew_cyclic_dot(c_.dt, d, c_.stream);
    launch_ok("dot_plain_cyclic");
    c_.stats.ct_pt_mult += (u64)P * d.n;
    c_.stats.ct_pt_limbs += (u64)P * d.n * (u64)f->ell;
    return true;
}

bool Evaluator::dot_plain_window(const std::vector<CtPtr>& cur, const std::vector<CtPtr>& prev, const std::vector<PtPtr>& pts,
                                 const std::vector<CtPtr>& dest, bool accumulate) {
    constexpr int W = EwWindow::W;
    if ((int)cur.size() != W || (int)prev.size() != W || (int)pts.size() != W || (int)dest.size() != W) return false;
    CtPtr f;
    for (const auto* v : {&cur, &prev})
        for (const CtPtr& c : *v)
            if (c && !f) f = c;
    if (!f) return false;
    u64 terms = 0;
    for (const auto* v : {&cur, &prev})
        for (const CtPtr& c : *v)
            if (c) {
                if (c->deg != 1 || !same_shape(*f, *c)) return false;
                ++terms;
            }
    for (const CtPtr& o : dest)
        if (!o || o->npoly != 2 || o->ell != f->ell) return false;
    const long double sf = c_.sf_real[f->level()];
    EwWindow d;
    d.ell = f->ell;
    d.accumulate = accumulate ? 1 : 0;
    std::vector<std::shared_ptr<Encoding>> hold;
    for (int j = 0; j < W; ++j) {
        hold.push_back(pts[j]->at(f->ell, sf));
        d.m[j] = hold.back()->d;
        d.cur[j] = cur[j] ? cur[j]->d : dest[0]->d;      // absent: any readable block of the operands' shape, dropped by the mask
        d.prev[j] = prev[j] ? prev[j]->d : dest[0]->d;
        if (cur[j]) d.cur_mask |= 1u << j;
        if (prev[j]) d.prev_mask |= 1u << j;
        d.out[j] = dest[j]->d;
        dest[j]->deg = f->deg + 1;
        dest[j]->scale = f->scale * sf;
        dest[j]->slots = f->slots;
    }
    launch_ew_window_dot(c_.dt, d, c_.stream);
    launch_ok("dot_plain_window");
    c_.stats.ct_pt_mult += terms * (u64)W / 2;          // every operand meets half of the block's plaintexts on average
    c_.stats.ct_pt_limbs += terms * (u64)W / 2 * (u64)f->ell;
    return true;
}

std::vector<CtPtr> Evaluator::add_batch(const std::vector<CtPtr>& a, const std::vector<CtPtr>& b) { return add_sub_batch(a, b, 1); }
std::vector<CtPtr> Evaluator::sub_batch(const std::vector<CtPtr>& a, const std::vector<CtPtr>& b) { return add_sub_batch(a, b, 2); }

// FLEXIBLEAUTO alignment of many operand pairs at once: x[i], y[i] = what match(a[i], b[i]) gives.  The common case of a row loop or
// of a round of a polynomial evaluation - a degree-1 operand with more limbs meets a degree-1 operand with fewer - goes through ONE
// batched integer multiply + rescale per (target limbs, target scale) instead of one per pair (adjust_deg1_batch: the residues of
// adjust(); the same ciphertext brought to the same target for several pairs is adjusted once); everything else through match().
void Evaluator::match_batch(const std::vector<CtPtr>& a, const std::vector<CtPtr>& b, std::vector<CtPtr>& x, std::vector<CtPtr>& y) {
    const size_t n = a.size();
    x.assign(n, CtPtr());
    y.assign(n, CtPtr());
    std::vector<char> aligned(n, 0);
    for (int side = 0; side < 2; ++side) {
        // side 0: b is brought down to a; side 1: a is brought down to b
        std::map<std::pair<int, long long>, std::vector<size_t>> groups;   // (target ell, bits of the target scale) -> pairs
        for (size_t i = 0; i < n; ++i) {
            if (aligned[i]) continue;
            const CtPtr& lo = side == 0 ? a[i] : b[i];
            const CtPtr& hi = side == 0 ? b[i] : a[i];
            if (lo->deg == 1 && hi->deg == 1 && lo->ell < hi->ell) {
                long long bits;
                const double sd = (double)lo->scale;
                std::memcpy(&bits, &sd, sizeof bits);
                groups[{lo->ell, bits}].push_back(i);
            }
        }
        for (auto& g : groups) {
            if (g.second.size() < 2) continue;
            // the 80-bit scales of a group must agree exactly (they do for rows of one call); else leave the pairs to match()
            const long double sc = (side == 0 ? a[g.second[0]] : b[g.second[0]])->scale;
            bool same = true;
            for (size_t i : g.second) same = same && (side == 0 ? a[i] : b[i])->scale == sc;
            if (!same) continue;
            std::vector<CtPtr> hi;
            std::map<const Ciphertext*, size_t> slot;                       // distinct ciphertexts to adjust
            std::vector<size_t> which(g.second.size());
            for (size_t k = 0; k < g.second.size(); ++k) {
                const CtPtr& h = side == 0 ? b[g.second[k]] : a[g.second[k]];
                auto it = slot.find(h.get());
                if (it == slot.end()) {
                    it = slot.emplace(h.get(), hi.size()).first;
                    hi.push_back(h);
                }
                which[k] = it->second;
            }
            std::vector<CtPtr> adj = adjust_deg1_batch(hi, g.first.first, sc);
            for (size_t k = 0; k < g.second.size(); ++k) {
                const size_t i = g.second[k];
                x[i] = side == 0 ? a[i] : adj[which[k]];
                y[i] = side == 0 ? adj[which[k]] : b[i];
                aligned[i] = 1;
            }
        }
    }
    for (size_t i = 0; i < n; ++i)
        if (!aligned[i]) match(a[i], b[i], x[i], y[i]);
}

std::vector<CtPtr> Evaluator::add_sub_batch(const std::vector<CtPtr>& a, const std::vector<CtPtr>& b, int op) {
    if (a.size() != b.size()) throw Error(FHELIN_ERR_ARG, "add_batch: operand count mismatch");
    std::vector<CtPtr> x, y, out(a.size());
    for (size_t i = 0; i < a.size(); ++i)
        if (a[i]->npoly != b[i]->npoly) throw Error(FHELIN_ERR_STATE, "add: component count mismatch");
    match_batch(a, b, x, y);   // the driver's residual additions output[i] + inputs[i] (src/main.cpp:237-239): one batched adjustment
    for_runs(x.size(), [&](size_t p, size_t q) { return x[p]->npoly == x[q]->npoly && x[p]->ell == x[q]->ell; },
             [&](size_t lo, size_t hi) {
                 const CtPtr& f = x[lo];
                 std::vector<CtPtr> o = new_ct_batch((int)(hi - lo), f->npoly, f->ell, f->deg, f->scale, f->slots);
                 EwItems it;
                 it.n = (int)(hi - lo);
                 it.vecs = it.b_vecs = f->npoly * f->ell;
                 for (size_t i = lo; i < hi; ++i) {
                     o[i - lo]->deg = x[i]->deg;
                     o[i - lo]->scale = x[i]->scale;
                     it.out[i - lo] = o[i - lo]->d;
                     it.a[i - lo] = x[i]->d;
                     it.b[i - lo] = y[i]->d;
                     out[i] = o[i - lo];
                 }
                 launch_ew_items(c_.dt, it, op, f->ell, c_.stream);
             });
    launch_ok("add_batch");
    return out;
}

void Evaluator::rescale_degree2(std::vector<CtPtr>& a, std::vector<CtPtr>* b, const char* two_components) {
    std::vector<CtPtr> need;
    std::map<const Ciphertext*, size_t> slot;
    for (const auto* side : {&a, b})
        for (size_t i = 0; side && i < side->size(); ++i) {
            const CtPtr& c = (*side)[i];
            if (two_components && c->npoly != 2) throw Error(FHELIN_ERR_STATE, two_components);
            if (c->deg >= 2 && !slot.count(c.get())) {
                slot[c.get()] = need.size();
                need.push_back(c);
            }
        }
    if (need.empty()) return;
    const std::vector<CtPtr> r = rescale_batch(need);
    for (auto* side : {&a, b})
        for (size_t i = 0; side && i < side->size(); ++i) {
            CtPtr& c = (*side)[i];
            if (c->deg >= 2) c = r[slot[c.get()]];
        }
}

std::vector<CtPtr> Evaluator::tensor_products(const std::vector<CtPtr>& x, const std::vector<CtPtr>& y, const std::vector<size_t>& idx) {
    const int B = (int)idx.size(), ell = x[idx[0]]->ell;
    std::vector<CtPtr> d = new_ct_batch(B, 3, ell, 2, 0, x[idx[0]]->slots);   // contiguous [B][3][ell][N]
    for (int k0 = 0; k0 < B; k0 += EwItems::MAX_ITEMS) {
        EwItems it;
        it.n = std::min(B - k0, (int)EwItems::MAX_ITEMS);
        for (int k = 0; k < it.n; ++k) {
            it.out[k] = d[k0 + k]->d;
            it.a[k] = x[idx[k0 + k]]->d;
            it.b[k] = y[idx[k0 + k]]->d;
        }
        launch_tensor_items(c_.dt, it, ell, c_.stream);
    }
    return d;
}

void Evaluator::product_operands(const std::vector<CtPtr>& a, const std::vector<CtPtr>& b, std::vector<CtPtr>& x, std::vector<CtPtr>& y) {
    // operands of degree 2 are rescaled first (every distinct ciphertext once), then brought to a common level per pair
    std::vector<CtPtr> ra = a, rb = b;
    rescale_degree2(ra, &rb, "mult: operands must have 2 components");
    match_batch(ra, rb, x, y);   // the level adjustments of all pairs of a round together (one batched rescale per target level)
}

std::vector<CtPtr> Evaluator::mult_batch(const std::vector<CtPtr>& a, const std::vector<CtPtr>& b) {
    if (a.size() != b.size()) throw Error(FHELIN_ERR_ARG, "mult_batch: operand count mismatch");
    if (!relin_key) throw Error(FHELIN_ERR_KEY, "no relinearisation key (EvalMultKeyGen not called)");
    std::vector<CtPtr> x, y;
    product_operands(a, b, x, y);
    for (const CtPtr& xi : x) bind_key(*relin_key, xi->ell);   // the products' limbs are known only now; before the first tensor product
    std::vector<CtPtr> out = for_groups(a.size(), batch_limit, [&](size_t f, size_t i) { return x[i]->ell == x[f]->ell; },
                                        [&](const std::vector<size_t>& idx) {
        const int B = (int)idx.size(), ell = x[idx[0]]->ell;
        const size_t pn = (size_t)ell * c_.N;
        const std::vector<CtPtr> d = tensor_products(x, y, idx);
        std::vector<CtPtr> o = new_ct_batch(B, 2, ell, 2, 0, x[idx[0]]->slots);
        keyswitch_batch(B, d[0]->d + 2 * pn, 3 * pn, ell, *relin_key, o[0]->d, 2 * pn, d[0]->d, d[0]->d + pn, 3 * pn, nullptr, nullptr, 0);
        for (int k = 0; k < B; ++k) {
            const size_t i = idx[k];
            o[k]->deg = x[i]->deg + y[i]->deg;
            o[k]->scale = x[i]->scale * y[i]->scale;
        }
        return o;
    });
    launch_ok("mult_batch");
    return out;
}

std::vector<CtPtr> Evaluator::mult_affine_rescale_batch(const std::vector<CtPtr>& a, const std::vector<CtPtr>& b, int f, double cadd,
                                                        const std::vector<CtPtr>& sub) {
    if (a.size() != b.size() || (!sub.empty() && sub.size() != a.size())) throw Error(FHELIN_ERR_ARG, "mult_affine_rescale_batch: operand count mismatch");
    if (f != 1 && f != 2) throw Error(FHELIN_ERR_ARG, "mult_affine_rescale_batch: factor 1 or 2");
    if (!relin_key) throw Error(FHELIN_ERR_KEY, "no relinearisation key (EvalMultKeyGen not called)");
    if (c_.K < 1 || c_.K + 1 > 16) throw Error(FHELIN_ERR_STATE, "mult_affine_rescale_batch: 1..15 special primes");
    // operands as mult_batch takes them (degree 2 rescaled first, every distinct ciphertext once), the pairs brought to one level one by one
    std::vector<CtPtr> ra = a, rb = b, x(a.size()), y(a.size());
    rescale_degree2(ra, &rb, "mult: operands must have 2 components");
    for (size_t i = 0; i < a.size(); ++i) match(ra[i], rb[i], x[i], y[i]);
    for (const CtPtr& xi : x) bind_key(*relin_key, xi->ell);   // relin_key->d goes to inner_product below as a pointer
    const size_t N = c_.N;
    const int K = c_.K, L1 = c_.L + 1;
    hipStream_t s = c_.stream;
    auto product_scale = [&](size_t i) { return x[i]->scale * y[i]->scale; };
    return for_groups(a.size(), batch_limit,
                      [&](size_t f0, size_t i) { return x[i]->ell == x[f0]->ell && fabsl(product_scale(i) / product_scale(f0) - 1.0L) < 1e-12L; },
                      [&](const std::vector<size_t>& idx) {
        const size_t first = idx[0];
        const int B = (int)idx.size(), ell = x[first]->ell;
        if (ell < 2) throw Error(FHELIN_ERR_STATE, "mult_affine_rescale_batch: no limb left to drop");
        const size_t pn = (size_t)ell * N;
        const long double sc = product_scale(first);
        const std::vector<CtPtr> d = tensor_products(x, y, idx);
        // the subtrahends at the products' (limbs, degree 2, scale), in one block
        std::vector<CtPtr> sadj;
        if (!sub.empty()) {
            for (int k = 0; k < B; ++k) sadj.push_back(adjust(sub[idx[k]], ell, 2, sc));
            sadj = make_contiguous(sadj, 7);
        }
        ScalarSet cst;
        if (cadd != 0.0) real_to_scalars(c_, (long double)cadd * sc, ell, cst);
        // key switch of d2 up to the accumulator
        KsShape sh = ks_shape(ell, B, {3 * pn, (size_t)2 * (ell - 1) * N, pn});
        c_.stats.keyswitch += (u64)B;
        c_.stats.keyswitch_limbs += (u64)B * ell;
        c_.stats.rescale += (u64)B;
        c_.stats.rescale_limbs += (u64)B * ell;
        const u64* c_ntt = d[0]->d + 2 * pn;
        std::vector<CtPtr> o = new_ct_batch(B, 2, ell - 1, 1, 0, x[first]->slots);
        {
            Scratch<u64> ext = modup(sh, c_ntt, true);   // digits times 2^64: launch_ks_inner ends in redc128
            KsAcc acc = inner_product(sh, ext, relin_key->d, c_ntt, f == 2 ? KsTail::EditsAccP : KsTail::Rescale);   // f = 2: accP itself is doubled below
            // X_Q = f acc_Q + P (f (d0, d1) + constant - subtrahend),  X_P = f acc_P
            launch_affine_acc(c_.dt, sh, acc.accQ, d[0]->d, sadj.empty() ? nullptr : sadj[0]->d, cst, cadd != 0.0 ? 1 : 0, f, c_.d_pmod, s);
            if (f == 2) launch_ew_add(c_.dt, acc.accP, acc.accP, acc.accP, B * 2 * K, B * 2 * K, L1, K, s);
            moddown_rescale(acc, o[0]->d);   // P and the top limb dropped together
            launch_ok("mult_affine_rescale_batch");
        }
        for (int k = 0; k < B; ++k) o[k]->scale = product_scale(idx[k]) / (long double)c_.chain.q[ell - 1];
        return o;
    });
}

std::vector<CtPtr> Evaluator::mult_affine_unmerged(const std::vector<CtPtr>& a, const std::vector<CtPtr>& b, const std::vector<AffineSpec>& spec) {
    std::vector<CtPtr> t = mult_batch(a, b);
    const size_t n = t.size();
    {   // factor 2: t + t, all such items in one batched addition
        std::vector<size_t> pos;
        std::vector<CtPtr> sel;
        for (size_t i = 0; i < n; ++i)
            if (spec[i].f == 2) {
                pos.push_back(i);
                sel.push_back(t[i]);
            }
        if (!sel.empty()) {
            const std::vector<CtPtr> r = add_batch(sel, sel);
            for (size_t j = 0; j < pos.size(); ++j) t[pos[j]] = r[j];
        }
    }
    for (size_t i = 0; i < n; ++i)
        if (spec[i].cadd != 0.0) t[i] = add_real(t[i], spec[i].cadd);
    for (const bool neg : {true, false}) {   // the subtrahends in one sub_batch, the addends in one add_batch
        std::vector<size_t> pos;
        std::vector<CtPtr> sel, ad;
        for (size_t i = 0; i < n; ++i)
            if (spec[i].addend && spec[i].negate == neg) {
                pos.push_back(i);
                sel.push_back(t[i]);
                ad.push_back(spec[i].addend);
            }
        if (sel.empty()) continue;
        const std::vector<CtPtr> r = neg ? sub_batch(sel, ad) : add_batch(sel, ad);
        for (size_t j = 0; j < pos.size(); ++j) t[pos[j]] = r[j];
    }
    return rescale_batch(t);
}

std::vector<CtPtr> Evaluator::mult_affine_batch(const std::vector<CtPtr>& a, const std::vector<CtPtr>& b, const std::vector<AffineSpec>& spec) {
    if (a.size() != b.size() || spec.size() != a.size()) throw Error(FHELIN_ERR_ARG, "mult_affine_batch: operand count mismatch");
    if (!relin_key) throw Error(FHELIN_ERR_KEY, "no relinearisation key (EvalMultKeyGen not called)");
    for (const AffineSpec& sp : spec) {
        if (sp.f != 1 && sp.f != 2) throw Error(FHELIN_ERR_ARG, "mult_affine_batch: factor 1 or 2");
        if (sp.addend && sp.addend->npoly != 2) throw Error(FHELIN_ERR_STATE, "add: component count mismatch");
    }
    if (!exact_products_on()) return mult_affine_unmerged(a, b, spec);
    const size_t n = a.size();
    std::vector<CtPtr> x, y;
    product_operands(a, b, x, y);
    for (const CtPtr& xi : x) bind_key(*relin_key, xi->ell);   // relin_key->d goes to launch_ks_inner below as a pointer
    // where the sequence would adjust the PRODUCT to its addend, or has no limb to drop, it runs itself (on the prepared operands: its own
    // preparation finds nothing left to do)
    for (size_t i = 0; i < n; ++i)
        if (x[i]->ell < 2 || (spec[i].addend && spec[i].addend->ell < x[i]->ell)) return mult_affine_unmerged(x, y, spec);
    const size_t N = c_.N;
    const int K = c_.K;
    hipStream_t s = c_.stream;
    static_assert(AffineItems::MAX_ITEMS <= EwItems::MAX_ITEMS, "the tensor products of a group are one launch");
    return for_groups(n, std::min(batch_limit, (int)AffineItems::MAX_ITEMS), [&](size_t f, size_t i) { return x[i]->ell == x[f]->ell; },
                      [&](const std::vector<size_t>& idx) {
        const size_t first = idx[0];
        const int B = (int)idx.size(), ell = x[first]->ell;
        const size_t pn = (size_t)ell * N;
        const std::vector<CtPtr> d = tensor_products(x, y, idx);
        // the affine parts at their products' (limbs, degree 2, scale): the addend as match() brings it to the product, the constant as add_real forms it
        AffineItems items;
        std::vector<CtPtr> adj(B);
        std::map<std::pair<const Ciphertext*, long double>, CtPtr> adjusted;
        std::vector<u64> cst((size_t)B * ell, 0);
        for (int k = 0; k < B; ++k) {
            const size_t i = idx[k];
            const AffineSpec& sp = spec[i];
            const long double sc = x[i]->scale * y[i]->scale;
            if (sp.f == 2) items.f2 |= 1u << k;
            if (sp.addend) {
                const CtPtr& ad = sp.addend;
                // a degree-1 addend that several items bring to the same (limbs, scale) - T_1 of a row, for every odd power of a round - is
                // adjusted once (one integer multiply, no rescale: the counters do not see it)
                const std::pair<const Ciphertext*, long double> key{ad.get(), sc};
                auto hit = ad->deg == 1 ? adjusted.find(key) : adjusted.end();
                if (hit != adjusted.end()) {
                    adj[k] = hit->second;
                } else {
                    adj[k] = ad->ell == ell && ad->deg == 2 ? ad : adjust(ad, ell, 2, sc);
                    if (ad->deg == 1) adjusted[key] = adj[k];
                }
                items.add[k] = adj[k]->d;
                if (sp.negate) items.neg |= 1u << k;
            }
            if (sp.cadd != 0.0) {
                ScalarSet one;
                real_to_scalars(c_, (long double)sp.cadd * sc, ell, one);
                for (int l = 0; l < ell; ++l) cst[(size_t)k * ell + l] = one.v[2 * l];
                items.cst |= 1u << k;
            }
        }
        Scratch<u64> dcst = c_.scratch<u64>(cst.size());
        if (items.cst) c_.upload_async(dcst, cst.data(), cst.size());
        KsShape sh = ks_shape(ell, B, {3 * pn, (size_t)2 * (ell - 1) * N, pn});
        sh.accp_limbs = K + 1;
        // counted as the unmerged sequence counts: one key switch and one rescale per product
        c_.stats.keyswitch += (u64)B;
        c_.stats.keyswitch_limbs += (u64)B * ell;
        c_.stats.rescale += (u64)B;
        c_.stats.rescale_limbs += (u64)B * ell;
        const u64* c_ntt = d[0]->d + 2 * pn;
        std::vector<CtPtr> o = new_ct_batch(B, 2, ell - 1, 1, 0, x[first]->slots);
        {
            Scratch<u64> ext = modup(sh, c_ntt, true);   // digits times 2^64: launch_ks_inner ends in redc128
            KsAcc acc = accumulators(sh, KsTail::Exact);   // accP with its K+1-th slot (sh.accp_limbs)
            launch_ks_inner(c_.dt, sh, acc.accQ, acc.accP, ext, relin_key->d, c_ntt, s);
            launch_affine_acc_items(c_.dt, sh, items, acc.accQ, acc.accP, d[0]->d, dcst, c_.d_pmod, s);
            moddown_rescale_exact(acc, o[0]->d, items.f2);
            launch_ok("mult_affine_batch");
        }
        for (int k = 0; k < B; ++k) o[k]->scale = x[idx[k]]->scale * y[idx[k]]->scale / (long double)c_.chain.q[ell - 1];
        return o;
    });
}

std::vector<CtPtr> Evaluator::add_plain_batch(const std::vector<CtPtr>& v, const PtPtr& p) {
    std::vector<CtPtr> out(v.size());
    for_runs(v.size(), [&](size_t a, size_t b) { return v[a]->npoly == v[b]->npoly && v[a]->ell == v[b]->ell; },
             [&](size_t lo, size_t hi) {
                 const CtPtr& f = v[lo];
                 std::vector<CtPtr> o = new_ct_batch((int)(hi - lo), f->npoly, f->ell, f->deg, f->scale, f->slots);
                 EwItems it;
                 it.n = (int)(hi - lo);
                 it.vecs = f->npoly * f->ell;
                 it.b_vecs = f->ell;
                 for (size_t i = lo; i < hi; ++i) {
                     auto enc = p->at(v[i]->ell, v[i]->scale);
                     o[i - lo]->deg = v[i]->deg;
                     o[i - lo]->scale = v[i]->scale;
                     it.out[i - lo] = o[i - lo]->d;
                     it.a[i - lo] = v[i]->d;
                     it.b[i - lo] = enc->d;
                     out[i] = o[i - lo];
                 }
                 launch_ew_items(c_.dt, it, 3, f->ell, c_.stream);
             });
    launch_ok("add_plain_batch");
    return out;
}

CtPtr Evaluator::rotate_add(const CtPtr& a, int index) {
    if (index % slot_count(a) == 0) return add(a, a);
    const RotKey k = rotation_key(index);
    return raw_rotate(a, k.g, *k.key, true, k.map);
}

CtPtr Evaluator::raw_mult_relin(const CtPtr& a, const CtPtr& b, const EvalKey& key) {
    if (a->npoly != 2 || b->npoly != 2 || a->ell != b->ell) throw Error(FHELIN_ERR_STATE, "mult: operands must be 2-component, same level");
    const int ell = a->ell;
    const size_t pn = (size_t)ell * c_.N;
    Scratch<u64> d = c_.scratch<u64>(3 * pn);
    launch_tensor(c_.dt, d, a->d, b->d, ell, c_.stream);
    CtPtr o = new_ct(2, ell, a->deg + b->deg, a->scale * b->scale, a->slots);
    keyswitch(d + 2 * pn, ell, key, o->d, d, d + pn, nullptr);
    return o;
}

CtPtr Evaluator::raw_modraise(const CtPtr& a, int new_ell) {
    if (a->ell != 1) throw Error(FHELIN_ERR_STATE, "modraise: the input must have exactly one limb (q0)");
    if (new_ell < 1 || new_ell > c_.L + 1) throw Error(FHELIN_ERR_ARG, "modraise: bad target limb count");
    const size_t N = c_.N;
    const int P = a->npoly;
    hipStream_t s = c_.stream;
    Scratch<u64> coef = c_.scratch<u64>((size_t)P * N);
    // INTT of the q0 limb of every polynomial, out of place (the input is immutable)
    LimbBatch ib{coef, P, nullptr, 0, 1, a->d};
    c_.ntt(ib, true);
    CtPtr up = new_ct(P, new_ell, a->deg, a->scale, a->slots);
    launch_modraise(c_.dt, up->d, coef, P, 0, new_ell, s);
    c_.ntt(LimbBatch{up->d, P * new_ell, nullptr, 0, new_ell}, false);
    launch_ok("modraise");
    return up;
}

std::vector<CtPtr> Evaluator::raw_modraise_batch(const std::vector<CtPtr>& vin, int new_ell) {
    if (vin.size() <= 1) {
        std::vector<CtPtr> out;
        for (const CtPtr& a : vin) out.push_back(raw_modraise(a, new_ell));
        return out;
    }
    for (const CtPtr& a : vin)
        if (a->ell != 1 || a->npoly != vin[0]->npoly) throw Error(FHELIN_ERR_STATE, "modraise: the inputs must have exactly one limb (q0) and one shape");
    if (new_ell < 1 || new_ell > c_.L + 1) throw Error(FHELIN_ERR_ARG, "modraise: bad target limb count");
    std::vector<CtPtr> in = make_contiguous(vin, 7);
    const size_t N = c_.N;
    const int B = (int)in.size(), P = in[0]->npoly * B;
    hipStream_t s = c_.stream;
    Scratch<u64> coef = c_.scratch<u64>((size_t)P * N);
    c_.ntt(LimbBatch{coef, P, nullptr, 0, 1, in[0]->d}, true);
    std::vector<CtPtr> up = new_ct_batch(B, in[0]->npoly, new_ell, 1, 0, in[0]->slots);
    launch_modraise(c_.dt, up[0]->d, coef, P, 0, new_ell, s);
    c_.ntt(LimbBatch{up[0]->d, P * new_ell, nullptr, 0, new_ell}, false);
    launch_ok("modraise_batch");
    coef.reset();
    for (int b = 0; b < B; ++b) {
        up[b]->deg = vin[b]->deg;
        up[b]->scale = vin[b]->scale;
        up[b]->slots = vin[b]->slots;
    }
    return up;
}

// ------------------------------------------------------------------------------------------------ leveled ops
CtPtr Evaluator::rescale(const CtPtr& a) {
    CtPtr o = raw_rescale(a);
    o->scale = a->scale / (long double)c_.chain.q[a->ell - 1];
    o->deg = a->deg > 1 ? a->deg - 1 : 1;
    return o;
}

CtPtr Evaluator::level_reduce(const CtPtr& a, int new_ell) {
    if (new_ell == a->ell) return a;
    if (new_ell < 1 || new_ell > a->ell) throw Error(FHELIN_ERR_ARG, "level_reduce: bad target");
    CtPtr o = new_ct(a->npoly, new_ell, a->deg, a->scale, a->slots);
    const size_t N = c_.N;
    hip_check(hipMemcpy2DAsync(o->d, (size_t)new_ell * N * 8, a->d, (size_t)a->ell * N * 8, (size_t)new_ell * N * 8, a->npoly,
                               hipMemcpyDeviceToDevice, c_.stream), "level_reduce");
    return o;
}

CtPtr Evaluator::mult_int(const CtPtr& a, u64 k, bool raise_deg, long double new_scale, int keep_ell) {
    // keep_ell > 0: the product on the first keep_ell limbs only (== level_reduce(mult_int(a), keep_ell), without touching the
    // limbs that would be dropped)
    const int ell = keep_ell > 0 ? std::min(keep_ell, a->ell) : a->ell;
    ScalarSet sc;
    for (int i = 0; i < ell; ++i) {
        u64 q = c_.chain.q[i];
        u64 v = k % q;
        sc.v[2 * i] = v;
        sc.v[2 * i + 1] = h_shoup(v, q);
    }
    CtPtr o = new_ct(a->npoly, ell, raise_deg ? a->deg + 1 : a->deg, new_scale, a->slots);
    if (c_.trace_scalar) c_.note_scalar(a->npoly * ell);
    launch_ew_scalar(c_.dt, o->d, a->d, sc, a->npoly * ell, 0, ell, c_.stream, ell < a->ell ? a->ell : 0);
    launch_ok("mult_int");
    return o;
}

// FLEXIBLEAUTO level adjustment of several degree-1 ciphertexts to ONE (limb count, scale): integer scalar x, the limbs above
// ell + 1 left out, and ONE batched rescale for all of them.  Same residues as adjust() one by one.
std::vector<CtPtr> Evaluator::adjust_deg1_batch(const std::vector<CtPtr>& v, int ell, long double scale) {
    return adjust_deg1_batch(v, ell, std::vector<long double>(v.size(), scale));
}

std::vector<CtPtr> Evaluator::adjust_deg1_batch(const std::vector<CtPtr>& v, int ell, const std::vector<long double>& scales) {
    if (scales.size() != v.size()) throw Error(FHELIN_ERR_ARG, "adjust_deg1_batch: one target scale per ciphertext");
    std::vector<CtPtr> out(v.size()), pending, src;
    std::vector<size_t> pos;
    for (size_t i = 0; i < v.size(); ++i) {
        CtPtr cur = v[i];
        if (cur->ell < ell) throw Error(FHELIN_ERR_STATE, "adjust: cannot raise a ciphertext to a lower level");
        if (cur->deg == 2) cur = rescale(cur);
        if (cur->ell == ell) {
            out[i] = cur;
            continue;
        }
        src.push_back(cur);
        pos.push_back(i);
    }
    if (!src.empty()) {
        // the integer products land in ONE block per component count (ell + 1 limbs each: only what the rescale reads), so that the
        // batched rescale takes them as they stand
        const long double qdrop = (long double)c_.chain.q[ell];
        const int lim = ell + 1;
        pending.assign(src.size(), CtPtr());
        std::map<int, std::vector<size_t>> by_npoly;
        for (size_t j = 0; j < src.size(); ++j) by_npoly[src[j]->npoly].push_back(j);
        for (const auto& g : by_npoly) {
            const std::vector<size_t>& idx = g.second;
            const size_t B = idx.size();
            const int npoly = g.first;
            if (B == 1 && by_npoly.size() > 1) {   // a single ciphertext of its shape: no block to share
                const CtPtr& cur = src[idx[0]];
                const u64 k = (u64)llroundl(scales[pos[idx[0]]] * qdrop / cur->scale);
                pending[idx[0]] = mult_int(cur, k, true, cur->scale * (long double)k, lim);
                continue;
            }
            std::vector<CtPtr> blk = new_ct_batch((int)B, npoly, lim, 2, 0, src[idx[0]]->slots);
            const bool items = adjust_items && B > 1;
            std::vector<u64> consts(items ? B * lim * 2 : 0);
            for (size_t b = 0; b < B; ++b) {
                const CtPtr& cur = src[idx[b]];
                const u64 k = (u64)llroundl(scales[pos[idx[b]]] * qdrop / cur->scale);
                const CtPtr& o = blk[b];
                o->deg = cur->deg + 1;
                o->scale = cur->scale * (long double)k;
                o->slots = cur->slots;
                pending[idx[b]] = o;
                if (items) {
                    for (int l = 0; l < lim; ++l) {
                        const u64 q = c_.chain.q[l], r = k % q;
                        consts[(b * lim + l) * 2] = r;
                        consts[(b * lim + l) * 2 + 1] = h_shoup(r, q);
                    }
                    continue;
                }
                ScalarSet sc;
                for (int l = 0; l < lim; ++l) {
                    const u64 q = c_.chain.q[l], r = k % q;
                    sc.v[2 * l] = r;
                    sc.v[2 * l + 1] = h_shoup(r, q);
                }
                if (c_.trace_scalar) c_.note_scalar(npoly * lim);
                launch_ew_scalar(c_.dt, o->d, cur->d, sc, npoly * lim, 0, lim, c_.stream, lim < cur->ell ? cur->ell : 0);
            }
            if (!items) continue;
            // every product of the group in one launch per EwScalarItems::MAX_ITEMS ciphertexts: the constants of (ciphertext, limb)
            // travel as a device table, uploaded once
            Scratch<u64> dk = c_.scratch<u64>(consts.size());
            for (size_t off = 0; off < consts.size(); off += 2 * c_.N)   // upload_async takes <= 2N words per call
                c_.upload_async(dk + off, consts.data() + off, std::min(consts.size() - off, (size_t)2 * c_.N));
            for (size_t lo = 0; lo < B; lo += EwScalarItems::MAX_ITEMS) {
                EwScalarItems d;
                d.n = (int)std::min(B - lo, (size_t)EwScalarItems::MAX_ITEMS);
                d.npoly = npoly;
                d.ell = lim;
                for (int k = 0; k < d.n; ++k) {
                    d.a[k] = src[idx[lo + k]]->d;
                    d.in_limbs[k] = src[idx[lo + k]]->ell;
                }
                launch_ew_scalar_items(c_.dt, d, blk[lo]->d, dk + lo * lim * 2, c_.stream);
            }
            launch_ok("adjust_deg1_batch");
            dk.reset();
        }
        launch_ok("adjust_deg1_batch");
    }
    if (!pending.empty()) {
        std::vector<CtPtr> r = rescale_batch(pending);
        for (size_t k = 0; k < pos.size(); ++k) {
            r[k]->scale = scales[pos[k]];
            out[pos[k]] = r[k];
        }
    }
    return out;
}

std::vector<CtPtr> Evaluator::scaled_diff_batch(const std::vector<CtPtr>& u, const std::vector<CtPtr>& w, const std::vector<u128>& a,
                                                const std::vector<u128>& c, bool raise_deg, const std::vector<long double>& scales) {
    const size_t B = u.size();
    if (w.size() != B || a.size() != B || c.size() != B || scales.size() != B)
        throw Error(FHELIN_ERR_ARG, "scaled_diff_batch: one operand pair, two constants and one scale per result");
    if (B == 0) return {};
    const int npoly = u[0]->npoly, ell = u[0]->ell;
    for (size_t i = 0; i < B; ++i)
        if (u[i]->npoly != npoly || w[i]->npoly != npoly || u[i]->ell != ell || w[i]->ell != ell)
            throw Error(FHELIN_ERR_STATE, "scaled_diff_batch: operands of different shapes");
    std::vector<u64> consts(B * ell * 4);
    for (size_t i = 0; i < B; ++i)
        for (int l = 0; l < ell; ++l) {
            const u64 q = c_.chain.q[l], ra = (u64)(a[i] % q), rc = (u64)(c[i] % q);
            u64* k = &consts[(i * ell + l) * 4];
            k[0] = ra;
            k[1] = h_shoup(ra, q);
            k[2] = rc;
            k[3] = h_shoup(rc, q);
        }
    Scratch<u64> dk = c_.scratch<u64>(consts.size());
    for (size_t off = 0; off < consts.size(); off += 2 * c_.N)   // upload_async takes <= 2N words per call
        c_.upload_async(dk + off, consts.data() + off, std::min(consts.size() - off, (size_t)2 * c_.N));
    std::vector<CtPtr> out = new_ct_batch((int)B, npoly, ell, 1, 0, u[0]->slots);
    for (size_t lo = 0; lo < B; lo += EwScaledDiff::MAX_ITEMS) {
        EwScaledDiff d;
        d.n = (int)std::min(B - lo, (size_t)EwScaledDiff::MAX_ITEMS);
        d.vecs = npoly * ell;
        d.ell = ell;
        for (int k = 0; k < d.n; ++k) {
            d.out[k] = out[lo + k]->d;
            d.u[k] = u[lo + k]->d;
            d.w[k] = w[lo + k]->d;
        }
        launch_ew_scaled_diff(c_.dt, d, dk + lo * ell * 4, c_.stream);
    }
    launch_ok("scaled_diff_batch");
    dk.reset();
    for (size_t i = 0; i < B; ++i) {
        out[i]->deg = raise_deg ? u[i]->deg + 1 : u[i]->deg;
        out[i]->scale = scales[i];
        out[i]->slots = u[i]->slots;
    }
    return out;
}

CtPtr Evaluator::adjust(const CtPtr& a, int ell, int deg, long double scale) {
    CtPtr cur = a;
    if (cur->ell < ell) throw Error(FHELIN_ERR_STATE, "adjust: cannot raise a ciphertext to a lower level");
    if (cur->ell == ell) {
        if (cur->deg == deg) return cur;
        if (cur->deg == 1 && deg == 2) {
            u64 k = (u64)llroundl(scale / cur->scale);
            return mult_int(cur, k, true, scale);
        }
        throw Error(FHELIN_ERR_STATE, "adjust: cannot lower the scale degree without dropping a limb");
    }
    if (deg == 1) {
        if (cur->deg == 2) cur = rescale(cur);
        if (cur->ell == ell) return cur;
        const long double qdrop = (long double)c_.chain.q[ell];
        u64 k = (u64)llroundl(scale * qdrop / cur->scale);
        cur = mult_int(cur, k, true, cur->scale * (long double)k, ell + 1);   // only the limbs the rescale reads
        cur = rescale(cur);
        cur->scale = scale;
        return cur;
    }
    if (cur->deg == 2) cur = rescale(cur);
    u64 k = (u64)llroundl(scale / cur->scale);
    return mult_int(cur, k, true, scale, ell);   // the product on the limbs that are kept only
}

void Evaluator::match(const CtPtr& a, const CtPtr& b, CtPtr& ao, CtPtr& bo) {
    if (a->ell == b->ell && a->deg == b->deg) {
        ao = a;
        bo = b;
        return;
    }
    // the operand with fewer limbs fixes the level; at equal level the degree-2 operand fixes the degree
    const bool a_rules = a->ell < b->ell || (a->ell == b->ell && a->deg >= b->deg);
    if (a_rules) {
        ao = a;
        bo = adjust(b, a->ell, a->deg, a->scale);
    } else {
        bo = b;
        ao = adjust(a, b->ell, b->deg, b->scale);
    }
}

CtPtr Evaluator::add(const CtPtr& a, const CtPtr& b) {
    if (a->npoly != b->npoly) throw Error(FHELIN_ERR_STATE, "add: component count mismatch");
    CtPtr x, y;
    match(a, b, x, y);
    CtPtr o = new_ct(x->npoly, x->ell, x->deg, x->scale, x->slots);
    launch_ew_add(c_.dt, o->d, x->d, y->d, x->npoly * x->ell, x->npoly * x->ell, 0, x->ell, c_.stream);
    launch_ok("add");
    return o;
}

CtPtr Evaluator::sub(const CtPtr& a, const CtPtr& b) {
    if (a->npoly != b->npoly) throw Error(FHELIN_ERR_STATE, "sub: component count mismatch");
    CtPtr x, y;
    match(a, b, x, y);
    CtPtr o = new_ct(x->npoly, x->ell, x->deg, x->scale, x->slots);
    launch_ew_sub(c_.dt, o->d, x->d, y->d, x->npoly * x->ell, x->npoly * x->ell, 0, x->ell, c_.stream);
    launch_ok("sub");
    return o;
}

CtPtr Evaluator::negate(const CtPtr& a) {
    CtPtr o = new_ct(a->npoly, a->ell, a->deg, a->scale, a->slots);
    launch_ew_neg(c_.dt, o->d, a->d, a->npoly * a->ell, 0, a->ell, c_.stream);
    launch_ok("negate");
    return o;
}

CtPtr Evaluator::add_plain(const CtPtr& a, const PtPtr& p) {
    auto enc = p->at(a->ell, a->scale);
    // one pass (op 3 of ew_items: add on component 0, copy the others) instead of a copy of the ciphertext + an add
    CtPtr o = new_ct(a->npoly, a->ell, a->deg, a->scale, a->slots);
    EwItems it;
    it.n = 1;
    it.vecs = a->npoly * a->ell;
    it.b_vecs = a->ell;
    it.out[0] = o->d;
    it.a[0] = a->d;
    it.b[0] = enc->d;
    launch_ew_items(c_.dt, it, 3, a->ell, c_.stream);
    launch_ok("add_plain");
    return o;
}

CtPtr Evaluator::mult_plain(const CtPtr& a, const PtPtr& p) {
    CtPtr x = a->deg >= 2 ? rescale(a) : a;
    auto enc = p->at(x->ell, c_.sf_real[x->level()]);
    CtPtr o = new_ct(x->npoly, x->ell, x->deg + 1, x->scale * enc->scale, x->slots);
    launch_ew_mul(c_.dt, o->d, x->d, enc->d, x->npoly * x->ell, x->ell, 0, x->ell, c_.stream);
    c_.stats.ct_pt_mult += 1;
    c_.stats.ct_pt_limbs += (u64)x->ell;
    launch_ok("mult_plain");
    return o;
}

CtPtr Evaluator::mult_no_relin(const CtPtr& a, const CtPtr& b) {
    if (a->npoly != 2 || b->npoly != 2) throw Error(FHELIN_ERR_STATE, "mult: operands must have 2 components");
    CtPtr x = a->deg >= 2 ? rescale(a) : a;
    CtPtr y = b->deg >= 2 ? rescale(b) : b;
    CtPtr xa, ya;
    match(x, y, xa, ya);
    CtPtr o = new_ct(3, xa->ell, xa->deg + ya->deg, xa->scale * ya->scale, xa->slots);
    launch_tensor(c_.dt, o->d, xa->d, ya->d, xa->ell, c_.stream);
    launch_ok("tensor");
    return o;
}

CtPtr Evaluator::relinearize(const CtPtr& a) {
    if (a->npoly == 2) return a;
    if (!relin_key) throw Error(FHELIN_ERR_KEY, "no relinearisation key (EvalMultKeyGen not called)");
    const size_t pn = (size_t)a->ell * c_.N;
    CtPtr o = new_ct(2, a->ell, a->deg, a->scale, a->slots);
    keyswitch(a->d + 2 * pn, a->ell, *relin_key, o->d, a->d, a->d + pn, nullptr);
    return o;
}

CtPtr Evaluator::mult(const CtPtr& a, const CtPtr& b) { return relinearize(mult_no_relin(a, b)); }

CtPtr Evaluator::rotate(const CtPtr& a, int index) {
    if (index % slot_count(a) == 0) return clone(a);
    const RotKey k = rotation_key(index);
    return raw_rotate(a, k.g, *k.key, false, k.map);
}

}  // namespace fhelin
