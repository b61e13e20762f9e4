// RNS-CKKS evaluator on top of the gfx950 kernels: ciphertext / plaintext / key objects and the leveled
// operations the reference reaches through OpenFHE's CryptoContext (reference src/FHEController.cpp
// :409-436 add/mult/rotate, FLEXIBLEAUTO level + scale bookkeeping implied by :18-24).
#pragma once
#include <cmath>
#include <map>
#include <memory>
#include <vector>
#include "context.h"
#include "kernels_elem.h"

namespace fhelin {

// One device allocation shared by the ciphertexts of a batch (rows of a matmul processed together).
struct DevBlock {
    Context* ctx = nullptr;
    u64* d = nullptr;
    ~DevBlock();
};

// Device-resident ciphertext: d[npoly][ell][N], NTT (evaluation) form.
struct Ciphertext {
    Context* ctx = nullptr;
    u64* d = nullptr;
    std::shared_ptr<DevBlock> block;  // set when d is a view into a batch allocation (then d is not owned)
    int npoly = 2;
    int ell = 0;          // live Q limbs; level (OpenFHE GetLevel) = L+1-ell
    int deg = 1;          // noiseScaleDeg: 1 after rescale / fresh, 2 after a multiplication
    long double scale = 0;
    int slots = 0;
    // set when the ciphertext was produced by a heavy op running asynchronously on a worker lane (capi_internal.h):
    // its data is valid on other streams only after async_ev
    bool async_pending = false;
    int async_lane = 0;
    u64 async_seq = 0;
    hipEvent_t async_ev = nullptr;
    // set only by the client's seeded (secret-key) encryptor: c1 is the expansion of (seed, nonce) (include/fhelin.h "Compact
    // ciphertexts") and the ciphertext can be exported compact.  Every operation makes a new Ciphertext and nothing writes into an
    // existing one, so no operation's result carries it.
    bool seeded = false;
    u64 nonce = 0;
    uint8_t seed[32] = {};
    // set only for a WRAPPED input (include/fhelin.h "Wrapped inputs"): ell = the inputs' limbs + 1 (limb ids 0..ell-1 of Q then P, so
    // the extra limb of an input at n_q limbs is p_0); slot column t < wrap_pos.size() holds input wrap_pos[t] of a sample of
    // wrap_total inputs (read order).  Only the unwrap, decryption, compact export and fhelin_ct_info accept one.
    std::vector<int> wrap_pos;
    int wrap_total = 0;
    bool wrapped() const { return !wrap_pos.empty(); }
    ~Ciphertext();
    int level() const { return ctx->L + 1 - ell; }
    size_t words() const { return (size_t)npoly * ell * ctx->N; }
};
typedef std::shared_ptr<Ciphertext> CtPtr;

// One device encoding of a plaintext vector at a given (limb count, scale).
struct Encoding {
    Context* ctx = nullptr;
    u64* d = nullptr;  // [ell][N] NTT form
    int ell = 0;
    // 0: row l is limb l (ell <= L+1 chain limbs, or the full key basis at ell = L+1+k).  > 0: limb-sliced (Plaintext::at_sliced): ell =
    // ell_q + k rows, Q limbs 0..ell_q-1 and then the k special limbs - the rows of the full-basis encoding a key switch at ell_q limbs reads
    int ell_q = 0;
    long double scale = 0;
    // made under lane `made_lane` (stream order covers its later uses there); another lane's stream waits for `ready` before its first
    // use (Plaintext::at) - a device-side wait, the host never blocks
    hipEvent_t ready = nullptr;
    int made_lane = 0;
    unsigned lanes_ordered = 0;   // bit k: lane k's stream is already ordered behind `ready`
    ~Encoding();
};

// Plaintext handle: keeps the slot values and lazily (re-)encodes them at whatever (level, scale) an
// operation needs — the effect OpenFHE gets by adjusting plaintext levels inside EvalMult/EvalAdd.
struct Plaintext {
    Context* ctx = nullptr;
    std::vector<double> values;  // real slot values, size == slots
    std::vector<double> imag;    // optional imaginary parts (bootstrapping's DFT diagonals); empty = real vector
    int slots = 0;
    // interleaved samples (context.h Context::stride) as the plaintext was made: `values` stay logical and at() encodes each into all
    // `stride` lanes of the slots * stride physical slots.  1 on bootstrapping's diagonals, which are written over the physical packing.
    int stride = 1;
    int level = 0;               // level requested at encode time (reference encode(vec, level, slots))
    // max |values[i]|, kept by Client::encode (finite there): at() refuses an encoding whose max_abs * scale may reach 2^125
    // (encode_domain_check) without a second pass over the values (every coefficient is an average of slot values, so max_abs bounds
    // it).  0 on plaintexts the library fills in itself (bootstrapping's diagonals, the unwrap mask): bounded by construction, and
    // the device encoder's staging walk sees their values anyway
    double max_abs = 0.0;
    static constexpr size_t MAX_ENCODINGS = 16;
    std::vector<std::shared_ptr<Encoding>> cache;   // most recently used first (Plaintext::at)
    std::shared_ptr<Encoding> at(int ell, long double scale, int ell_q = 0);
    // the limb-sliced encoding over the key basis at ell_q live limbs, [ell_q + k][N], at exactly `scale`: what
    // Evaluator::linear_transform_rows multiplies in QP.  Cached apart from the plain encodings (Encoding::ell_q is part of the key)
    std::shared_ptr<Encoding> at_sliced(int ell_q, long double scale);
    // device bytes of the limb-sliced encodings this handle holds
    size_t sliced_bytes() const {
        size_t b = 0;
        for (const auto& e : cache)
            if (e->ell_q > 0) b += (size_t)e->ell * ctx->N * 8;
        return b;
    }
    // set on a handle of the content-keyed plaintext cache (capi_internal.h PtCache): the cache's own plaintext of the same values.  An
    // encoding this handle has not used yet is taken from there when one exists at EXACTLY this (limb count, scale) - the bytes this
    // handle would have made itself - and every encoding made here is left there for the handles of later passes.  The handle's own
    // list, and with it which of two nearly equal scales an operation gets, is what it would be without the cache.
    std::shared_ptr<Plaintext> shared;
    static constexpr size_t MAX_SHARED_ENCODINGS = 64;
    // set on a handle made from residues (fhelin_debug_pt_from_residues): it has no slot values, its one encoding is all it holds, and a
    // request at any other (limb count, scale) is an error (FHELIN_ERR_STATE) instead of an encoding of nothing
    bool fixed = false;
};
typedef std::shared_ptr<Plaintext> PtPtr;

struct EvalKey {
    Context* ctx = nullptr;
    u64* d = nullptr;  // [dnum][2][L+1+k][N] NTT form; component 0 = b, 1 = a
    // the same key with every limb vector gathered through the key's own automorphism map (d_perm[v][n] = d[v][map_g[n]]):
    // the merged rotation sums apply sigma_g to the inner product d * evk BEFORE the shared ModDown, so with this copy the
    // key streams of ks_inner_multi are contiguous and only the digits are gathered.  A plain rotation gathers at its inner product
    // too and reads the same copy (KsShape::gather).  Built on first use (Evaluator::permuted).
    mutable u64* d_perm = nullptr;
    int digits = 0;        // digits held: Context::digits_at(max_ell); d, d_perm and the folded copies all have this many
    bool seeded = false;   // every a half is the expansion of the key-set seed (include/fhelin.h "Seeded evaluation keys")
    // level-capped keys (include/fhelin.h "Level-capped keys"): the most live limbs a key switch may bind this key at.  Of the digits
    // held, the Q rows max_ell .. L are zero (never read at ell <= max_ell); max_ell == L+1: uncapped, today's key
    int max_ell = 0;
    // what the key is, for the refusal's message and the usage recorder: kind 1 relinearisation / 2 rotation / 3 conjugation as in
    // the key-set file (0: not known), its Galois element (0 for kind 1), the rotation index it was generated for where known
    int kind = 0;
    u64 galois = 0;
    bool has_index = false;
    int index = 0;
    bool capped() const { return max_ell < ctx->L + 1; }
    ~EvalKey();
    size_t words() const { return (size_t)digits * 2 * (ctx->L + 1 + ctx->K) * ctx->N; }
};
typedef std::shared_ptr<EvalKey> KeyPtr;

// two scales that one launch set may treat as one: within 1e-9 of each other (every output still carries its own)
inline bool same_scale(const Ciphertext& a, const Ciphertext& b) { return fabsl(b.scale / a.scale - 1.0L) < 1e-9L; }
// "the same shape" of the batched operations: two components, the same limbs and noise degree, the same scale in the sense above.
// A site that needs more says so (same_shape(..) && ..); one that deliberately tests less keeps its own predicate.
inline bool same_shape(const Ciphertext& a, const Ciphertext& b) {
    return a.npoly == 2 && b.npoly == 2 && a.ell == b.ell && a.deg == b.deg && same_scale(a, b);
}

// round(v) (half away from zero, 80-bit v) modulo the first ell limbs, with Shoup companions (polyeval.cpp)
void real_to_scalars(const Context& c, long double v, int ell, ScalarSet& sc);

class Evaluator {
public:
    explicit Evaluator(Context& c) : c_(c) {}
    Context& ctx() { return c_; }

    // ---- allocation / import / export
    CtPtr new_ct(int npoly, int ell, int deg, long double scale, int slots);
    std::vector<CtPtr> new_ct_batch(int count, int npoly, int ell, int deg, long double scale, int slots);
    // base pointer of `v` if its members are consecutive views of one block (else nullptr)
    static u64* contiguous_base(const std::vector<CtPtr>& v);
    std::vector<CtPtr> make_contiguous(const std::vector<CtPtr>& v, int site = -1);
    u64 gather_copies[8] = {};   // ciphertext copies made by make_contiguous, per call site (diagnostics)
    bool dot_groups = true;    // inner sums of all giant steps of a linear stage in one pass (dot_plain_groups); FHELIN_DOT_GROUPS=0: one pass each
    bool cheb_leaf_at_product = true;   // r-leaves of the Paterson-Stockmeyer tree born at their product's (limbs, scale); FHELIN_CHEB_LEAF_AT=0: level-adjusted afterwards
    bool cheb_leaf_classes = true;   // a Chebyshev leaf's babies aligned to the deepest power IT uses (one level saved: OpenFHE's depth); FHELIN_CHEB_LEAF_CLASSES=0: all babies at one level
    bool cheb_rounds = true;   // Paterson-Stockmeyer products in rounds (polyeval.cpp cheb_recurse); FHELIN_CHEB_ROUNDS=0: one at a time
    bool adjust_items = true;  // the integer products of a batched level adjustment in one launch per 32 ciphertexts (adjust_deg1_batch); FHELIN_ADJUST_ITEMS=0: one launch each
    int batch_limit = 32;   // rows processed per batched key switch (FHELIN_BATCH overrides; 16 / 24 / 32 / 48 / 64 re-measured at the end of round 2: DESIGN.md)
    CtPtr clone(const CtPtr& a);
    KeyPtr new_key(int max_ell = 0);   // max_ell in 1 .. L: a level-capped key (zero-filled: its absent rows stay zero); 0 or L+1: uncapped

    // ---- level-capped keys (include/fhelin.h "Level-capped keys")
    // THE check: every site that hands `key` to a KsShape or an accumulator at `ell` live limbs calls this before it launches or counts
    // anything.  ell > key.max_ell is FHELIN_ERR_KEY (the rows such a switch would read are not held).  While the usage recorder runs it
    // also notes max(ell) for the key.  One integer comparison on the default path.
    void bind_key(const EvalKey& key, int ell);
    bool usage_on = false;
    std::map<std::pair<int, u64>, int> usage;   // (kind, galois) -> max ell bound while usage_on

    // ---- keys
    std::map<u64, KeyPtr> rot_keys;  // by galois element
    KeyPtr relin_key;
    KeyPtr conj_key;
    // sparse-secret bootstrapping (include/fhelin.h "Sparse-secret bootstrapping"): s -> s~ (kind 4, always capped at two limbs) and
    // s~ -> s (kind 5); null with the knob off
    KeyPtr to_sparse_key, from_sparse_key;

    // ---- K6-K8 composite: out[2][ell][N] = KeySwitch(c) (+ add0/add1, gathered through map if given)
    void keyswitch(const u64* c_ntt, int ell, const EvalKey& key, u64* out, const u64* add0, const u64* add1, const u32* map,
                   const u64* post = nullptr);
    // the same for `batch` independent polynomials laid out with the given element strides
    void keyswitch_batch(int batch, const u64* c_ntt, size_t c_stride, int ell, const EvalKey& key, u64* out, size_t out_stride,
                         const u64* add0, const u64* add1, size_t add_stride, const u32* map, const u64* post, size_t post_stride);
    // rows with their own evaluation key / automorphism map; shared_input: all rows key-switch the SAME polynomial
    // (c_stride ignored, ModUp done once).  At most KsShape::MAX_ROWS rows.
    struct KsRows {
        std::vector<const EvalKey*> keys;
        std::vector<const u32*> maps;
        bool shared_input = false;
    };
    void keyswitch_rows(const KsRows& rows, const u64* c_ntt, size_t c_stride, int ell, u64* out, size_t out_stride, const u64* add0,
                        size_t add_stride);
    // v[i] + sum_r rot(v[i], indices[r]) with ONE ModUp and ONE ModDown per row: the rotated terms are accumulated in the
    // extended basis (kernels_elem.h launch_ks_inner_multi).  Two steps of a rotate-and-sum tree, x += rot(x, s);
    // x += rot(x, 2s), are the call {s, 2s, 3s}.  All keys must exist (have_rotation_keys).
    std::vector<CtPtr> rotate_sum_batch(const std::vector<CtPtr>& v, const std::vector<int>& indices);
    bool have_rotation_keys(const std::vector<int>& indices, int slots) const;
    const u64* permuted(const EvalKey& key, const u32* map);   // key.d_perm, built once
    // sum_i rot(v[i], indices[i]) for up to 7 ciphertexts of identical shape (index 0 = unrotated term allowed): every
    // term has its own ModUp and key, the inner products are accumulated in QP and share ONE ModDown (giant steps)
    CtPtr rotate_each_sum(const std::vector<CtPtr>& v, const std::vector<int>& indices);
    // the same for many independent rows that share one index list: out[b] = sum_r rot(rows[b][r], indices[r]), with the key
    // switches of a chunk of rows batched (one ModUp over rows x terms, one inner-product launch, one ModDown over rows).
    // Same residues as rotate_each_sum row by row (<= 7 rotated terms per row).
    std::vector<CtPtr> rotate_each_sum_rows(const std::vector<std::vector<CtPtr>>& rows, const std::vector<int>& indices);
    // double hoisting: out[b] = xs[b] * pts[0] + sum_r rot(xs[b], indices[r]) * pts[r + 1]  (== sum_r rot(xs[b] * rot(pts[r + 1], -indices[r]),
    // indices[r]) in slot values) with ONE ModUp and ONE ModDown per row: the rotations share the row's digits and the plaintext
    // products are taken in the extended basis, through rotation keys with the plaintext folded in (folded_key; kernels_elem.h
    // launch_fold_key).  Meant for FEW plaintexts shared by MANY rows (the re-arranged weights of matmulRElarge): a folded key is a
    // full key copy.  Output: noise degree + 1, scale x the level's plaintext scale; 1 <= R <= 7 rotations.
    // rescale_out: the result is wanted rescaled - ModDown and rescale run as ONE basis conversion (drop P and the top limb together:
    // kernels_elem.h launch_moddown_rescale_conv); output one limb and one noise degree lower, scale / q_top.  A different integer
    // function from hoisted_dot_rows + rescale (one rounding instead of two), same value up to rounding noise.
    std::vector<CtPtr> hoisted_dot_rows(const std::vector<CtPtr>& xs, const std::vector<PtPtr>& pts, const std::vector<int>& indices,
                                        bool rescale_out = false);
    // baby-step/giant-step matrix x ciphertext, the baby steps shared in QP (include/fhelin.h "Linear transforms"):
    //     out[r] = sum_g rot( xs[r] * pts[g][0] + sum_{b>0} rot(xs[r], baby[b]) * pts[g][b],  giant[g] )
    // pts [n2][n1], null = term absent; baby[0] == 0; n1 <= 32.  ONE ModUp per row, the inner sums of all groups from the rotation keys
    // as they are (launch_ks_inner_dot: no folded keys, no rotated ciphertext in memory), ONE ModDown over rows x groups, then the
    // giant steps through rotate_each_sum_rows.  The residues of rotate_each_sum([hoisted_dot(x, pts[g], baby[1:]) for g], giant).
    // The planner's cost of splitting the diagonal indices idx (>= 0) into n1 baby steps, in quarters of a pair-ModDown:
    // 4 * (n2 + ceil(R / 7)) + (baby keys read); n2 = the giant-step groups that carry a diagonal, R = those of them that are rotated (g != 0),
    // baby keys = the distinct nonzero residues d mod n1.  Every group costs one pair-ModDown for its inner sum and the rotated groups share one
    // more per 7 in the giant steps; a baby step costs one pass over its rotation key in the inner product, taken as a quarter of a
    // pair-ModDown (2 beta (ell + k) limb vectors streamed once against the ModDown's 2 k inverse and 2 ell forward transforms and its
    // conversion) - an estimate, not a measurement.  Used by fhelin_lt_create and by the bootstrap's stages (Bootstrapper::set_lt)
    static int lt_split_cost(const std::vector<int>& idx, int n1);
    // pt_scale > 0: the plaintexts are taken at that scale instead of the level's own (the bootstrap's first stage after a ModRaise to fewer
    // limbs: Bootstrapper::apply); the result's scale follows
    std::vector<CtPtr> linear_transform_rows(const std::vector<CtPtr>& xs, const std::vector<std::vector<PtPtr>>& pts,
                                             const std::vector<int>& baby, const std::vector<int>& giant, bool rescale_out = false,
                                             long double pt_scale = 0);
    // the power steps of a Chebyshev evaluation and EvalMod's double angle through mult_affine_rescale_batch.  OFF by default
    // (FHELIN_MERGED_PRODUCTS=1 turns it on): measured at no gain (282.0 vs 281.2 ms per pass: the launches it saves are replaced by its
    // own) and at 3 x the logit error (0.017 vs 0.006: the merged conversion's rounding has three times the standard deviation of a
    // centred rescale, and these chains are where rounding noise is amplified) - DESIGN.md 6c
    bool merged_products = false;
    bool merged_rescale = true; // results that are rescaled right after their key switch drop P and the top limb in one conversion; FHELIN_MERGED_RESCALE=0: ModDown, then rescale
    bool double_hoist = true;   // Composite::matmulRElarge takes its first step through hoisted_dot_rows; FHELIN_DOUBLE_HOIST=0: rotate_each_sum_rows
    struct FoldedKey {
        PtPtr pt;
        KeyPtr key;
        int index = 0;
        long double scale = 0;
        std::shared_ptr<Encoding> enc;   // the plaintext over the full key basis [L+1+k][N]
        std::shared_ptr<DevBlock> d;     // [digits][2][L+1+k][N], layout of EvalKey::d_perm
    };
    std::vector<FoldedKey> folded_keys;  // bounded (MAX_FOLDED), oldest first
    static constexpr size_t MAX_FOLDED = 12;
    FoldedKey folded_key(const PtPtr& p, int index, long double scale);   // by value: the cache may evict the entry on a later call
    // hoisted rotations: rot(a, i) for every i in `indices` with ONE ModUp of a (results identical to rotate(a, i))
    std::vector<CtPtr> rotate_many(const CtPtr& a, const std::vector<int>& indices);
    // the same for several ciphertexts of one shape and ONE index list (the baby steps of a batch of bootstraps): one ModUp over
    // all inputs, per input the inner products of all indices, one ModDown over all inputs x indices.  out[i][k] holds exactly
    // the residues of rotate(xs[i], indices[k]).
    std::vector<std::vector<CtPtr>> rotate_many_batch(const std::vector<CtPtr>& xs, const std::vector<int>& indices);
    // test hook (fhelin_debug_ks_accp): the special-limb half of a key switch's inner product over digits the caller chooses residue by
    // residue, through inner_product and accp_inverse as they stand.  ext [batch][beta][ell+K][N] (device); returns the accumulator's own
    // [batch][2][K][N]: INTT(accP).  n_rot = 0: the identity form over the relinearisation key as stored (the sum comes times 2^-64);
    // else the merged form over the permuted keys of the n_rot <= 7 rotations.
    Scratch<u64> debug_ks_accp(const u64* ext, int ell, int batch, const int* indices, int n_rot);
    // test hook (fhelin_debug_ks_accq): the Q-limb half of a single-key inner product and the row-pass finish of its ModDown over operands the
    // caller chooses residue by residue, through inner_product and moddown_rows as they stand.  ext [batch][beta][ell+K][N], own [batch][ell][N]
    // (the switched polynomial, NTT form), conv [batch][2][ell][N] (coefficient form, canonical; overwritten), out [batch][2][ell][N], all
    // device: out = (accQ - NTT(conv)) * P^-1.  index = 0: the identity form over the relinearisation key as stored (digit terms times 2^-64,
    // the own-limb term plain); else the gathered form of that rotation (operands read through its map, no c0 addend).
    void debug_ks_accq(const u64* ext, const u64* own, u64* conv, int ell, int batch, int index, u64* out);
    // rows of identical shape through one batched key switch with an explicit Galois element and key (conjugation, the SubSum
    // rotations by multiples of the slot count); accumulate: v_i + sigma_g(v_i)
    std::vector<CtPtr> rotate_galois_batch(const std::vector<CtPtr>& v, u64 galois, const EvalKey& key, bool accumulate);
    std::vector<CtPtr> conjugate_batch(const std::vector<CtPtr>& v);
    // the identity-automorphism switch to the secret `key` targets: (c0 + KS(c1)[0], KS(c1)[1]) - the relinearisation's key switch with
    // c1 where that has c2 and no second addend.  Limbs, degree, scale and slots pass through.  The batch: rows of one shape through
    // one batched key switch, out[i] the residues of switch_key(v[i], key)
    CtPtr switch_key(const CtPtr& a, const EvalKey& key);
    std::vector<CtPtr> switch_key_batch(const std::vector<CtPtr>& v, const EvalKey& key);
    std::vector<CtPtr> raw_modraise_batch(const std::vector<CtPtr>& v, int new_ell);   // raw_modraise over many one-limb ciphertexts
    // rot(v[i], indices[i]) for ciphertexts of identical shape, one batched key switch per chunk of rows
    std::vector<CtPtr> rotate_each(const std::vector<CtPtr>& v, const std::vector<int>& indices);
    // batched leveled ops over independent ciphertexts of identical (level, degree, scale): one launch set per op
    std::vector<CtPtr> rotate_add_batch(const std::vector<CtPtr>& v, int index);   // v_i + rot(v_i, index)
    std::vector<CtPtr> rotate_batch(const std::vector<CtPtr>& v, int index);
    std::vector<CtPtr> rotate_batch_impl(const std::vector<CtPtr>& v, int index, bool accumulate);
    std::vector<CtPtr> mult_plain_batch(const std::vector<CtPtr>& v, const PtPtr& p);
    // element-wise ops over many independent ciphertexts, one launch per 32 operands of identical shape; the
    // bookkeeping (rescale before a product, level/scale matching before a sum) is exactly that of the single ops
    std::vector<CtPtr> mult_plain_each(const std::vector<CtPtr>& v, const std::vector<PtPtr>& p);  // v[i] * p[i]
    // sum_i v[i] * p[i]: the residues of add(...add(mult_plain(v0,p0), mult_plain(v1,p1))...) in one pass per 32 terms when the
    // operands share one shape after the usual pre-rescale (else that chain itself)
    // out_g = sum_b cts[b] * pts[g][b] (null = term absent) for all g in ONE pass over the ciphertexts, written to dest[g]
    // (deg+1, scale x plaintext scale); false if the operands do not fit the kernel (caller falls back to dot_plain per g)
    bool dot_plain_groups(const std::vector<CtPtr>& cts, const std::vector<std::vector<PtPtr>>& pts, long double pt_scale,
                          const std::vector<CtPtr>& dest);
    // the 32 cyclic sums out_k = sum_i cts[i] * pts[(i + k) mod 32] over <= 32 ciphertexts of one shape (degree 1) in one pass
    // (kernels_elem.h launch_ew_cyclic_dot), written to dest[k]; the residues of dot_plain per k.  false: operands do not fit
    bool dot_plain_cyclic(const std::vector<CtPtr>& cts, const std::vector<PtPtr>& pts, const std::vector<CtPtr>& dest);
    // one 32 x 32 block of a sliding-window sum (kernels_elem.h launch_ew_window_dot):
    //     dest[t] (+)= sum_{j<32} (j <= t ? cur[j] : prev[j]) * pts[(t - j) mod 32]
    // cur / prev: 32 entries each, null = zero; all present ciphertexts of one shape, degree 1; accumulate: dest holds earlier blocks' sums
    bool dot_plain_window(const std::vector<CtPtr>& cur, const std::vector<CtPtr>& prev, const std::vector<PtPtr>& pts,
                          const std::vector<CtPtr>& dest, bool accumulate);
    // dot_plain_groups for SEVERAL sets of ciphertexts and ONE set of plaintexts in one launch (a batch of bootstraps: the stage's
    // diagonals are fetched once for the batch): out[x][g] = sum_b cts[x][b] * pts[g][b].  Needs every cts[.][b] and every dest[.][g]
    // equally spaced over x (views of one block); false otherwise (caller: dot_plain_groups per set).  Same residues.
    bool dot_plain_groups_batch(const std::vector<std::vector<CtPtr>>& cts, const std::vector<std::vector<PtPtr>>& pts, long double pt_scale,
                                const std::vector<std::vector<CtPtr>>& dest);
    CtPtr dot_plain(const std::vector<CtPtr>& v, const std::vector<PtPtr>& p, long double pt_scale = 0,
                    const CtPtr& dest = CtPtr());   // pt_scale > 0: encode the plaintexts at this scale instead of the level's own;
                                                    // dest: write the sum there (a slice of a caller's batch block)
    std::vector<CtPtr> add_batch(const std::vector<CtPtr>& a, const std::vector<CtPtr>& b);        // a[i] + b[i]
    std::vector<CtPtr> add_plain_batch(const std::vector<CtPtr>& v, const PtPtr& p);
    std::vector<CtPtr> sub_batch(const std::vector<CtPtr>& a, const std::vector<CtPtr>& b);        // a[i] - b[i]
    // a[i] * b[i] with relinearisation: one batched key switch (shared relin key) per chunk of rows
    std::vector<CtPtr> mult_batch(const std::vector<CtPtr>& a, const std::vector<CtPtr>& b);
    // rescale(f * a[i] * b[i] + cadd - sub[i]) (f = 1 or 2; sub empty = none): relinearised products that are rescaled right away - the
    // power steps T_2k = 2 T_k^2 - 1, T_(j+k) = 2 T_j T_k - T_(j-k) of a Chebyshev evaluation, EvalMod's double angle.  Operands as in
    // mult_batch; the constant and the subtrahend (adjusted to the product's limbs / degree 2 / scale) enter the key switch's
    // accumulator times P, and ModDown and rescale run as ONE basis conversion: 2 ell fewer transforms and five fewer launches per
    // product than mult_batch, add_batch, add_real / sub_batch, rescale_batch.  One rounding where those have two (oracle:
    // orc_mult_affine_rescale).  Output: degree 1, one limb fewer, scale a.scale * b.scale / q_top.
    std::vector<CtPtr> mult_affine_rescale_batch(const std::vector<CtPtr>& a, const std::vector<CtPtr>& b, int f, double cadd,
                                                 const std::vector<CtPtr>& sub);
    // The same power steps with the residues of the UNMERGED sequence, bit for bit (on by default; FHELIN_EXACT_PRODUCTS=0: the sequence
    // itself - mult_batch, add_batch, add_real / sub_batch, rescale_batch).  out[i] = rescale(f_i a[i] b[i] + cadd_i +- addend_i): every
    // item has its own factor, constant and addend, so the even and the odd powers of a round share ONE batched key switch.  The affine
    // part enters the accumulator times P as in mult_affine_rescale_batch, but ModDown and rescale keep their two roundings: the tail
    // (moddown_rescale_exact) forms the rescale's centred lift from the top limb of the ModDown's result, which it obtains in coefficient
    // form from the SAME inverse transform that serves the special limbs, and one forward transform carries conversion and lift together
    // (DESIGN.md 6g).  Operand preparation is mult_batch's own (product_operands); an addend is brought to its product's (limbs, degree
    // 2, scale) as sub_batch / add_batch bring it there; a call with an addend of fewer limbs than its product (where those would adjust
    // the product instead) runs the sequence.
    struct AffineSpec {
        int f = 1;          // 1 or 2
        double cadd = 0;    // real constant added to every slot
        CtPtr addend;       // optional
        bool negate = false;   // the addend is subtracted
    };
    bool exact_products = true;
    // the knob, and a shape the tail takes (1..15 special primes); a product with a single limb fails as its rescale would
    bool exact_products_on() const { return exact_products && c_.K >= 1 && c_.K + 1 <= 16; }
    std::vector<CtPtr> mult_affine_batch(const std::vector<CtPtr>& a, const std::vector<CtPtr>& b, const std::vector<AffineSpec>& spec);
    // the same Chebyshev series on several ciphertexts at once: every product of the evaluation runs as mult_batch over
    // all ciphertexts AND all independent nodes of the same depth (baby powers of one doubling round)
    std::vector<CtPtr> eval_chebyshev_many(const std::vector<CtPtr>& xs, const std::vector<double>& coeffs, double a, double b);
    // levels eval_chebyshev_many spends on a series of this degree (>= 1) with every knob at its default, the result's pending rescale
    // counted: the depth of the tree it builds (polyeval.cpp), worked out on the host.  4 for 14, 5 for 28, 6 for 29..59, 7 for 119
    static int cheb_depth(int degree);
    std::vector<CtPtr> rescale_batch(const std::vector<CtPtr>& v);

    // ---- leveled ops (functional: inputs are never modified)
    CtPtr add(const CtPtr& a, const CtPtr& b);
    CtPtr sub(const CtPtr& a, const CtPtr& b);
    CtPtr negate(const CtPtr& a);
    CtPtr add_plain(const CtPtr& a, const PtPtr& p);
    CtPtr mult_plain(const CtPtr& a, const PtPtr& p);
    CtPtr mult(const CtPtr& a, const CtPtr& b);             // tensor + relinearise (auto-rescale inputs of deg 2)
    CtPtr mult_no_relin(const CtPtr& a, const CtPtr& b);    // 3-component result
    CtPtr relinearize(const CtPtr& a);
    CtPtr mult_int(const CtPtr& a, u64 k, bool raise_deg, long double new_scale, int keep_ell = 0);
    std::vector<CtPtr> adjust_deg1_batch(const std::vector<CtPtr>& v, int ell, long double scale);  // by an integer constant
    std::vector<CtPtr> adjust_deg1_batch(const std::vector<CtPtr>& v, int ell, const std::vector<long double>& scales);  // one target scale each
    // out[i] = a[i] * u[i] - c[i] * w[i] (integers a, c reduced per limb; kernels_elem.h launch_ew_scaled_diff) for pairs of identical
    // shape, one launch per 32 pairs, the results in ONE block (a batched rescale takes them as they stand).  Degree u's (+1 if
    // raise_deg), scale scales[i].  The residues of sub(mult_int(u, a), mult_int(w, c)) at equal (limbs, degree).
    std::vector<CtPtr> scaled_diff_batch(const std::vector<CtPtr>& u, const std::vector<CtPtr>& w, const std::vector<u128>& a,
                                         const std::vector<u128>& c, bool raise_deg, const std::vector<long double>& scales);
    CtPtr mult_real(const CtPtr& a, double c);              // by a real constant: per-limb scalar round(c * Delta_level)
    CtPtr add_real(const CtPtr& a, double c);               // add a real constant to every slot
    // sum_k coef[k] * terms[k] + c0 for ciphertexts of identical (level, degree 1, scale): the residues of the chain
    // add(mult_real(t_1, c_1), mult_real(t_2, c_2), ...) + add_real(c0), in one kernel pass (falls back to that chain when
    // the shapes differ).  Terms with coef 0 are skipped.
    CtPtr lincomb(const std::vector<CtPtr>& terms, const std::vector<double>& coef, double c0);
    CtPtr lincomb_at(const std::vector<CtPtr>& terms, const std::vector<double>& coef, double c0, long double want_scale, int keep_ell);
    CtPtr rotate(const CtPtr& a, int index);
    CtPtr conjugate(const CtPtr& a);
    // polynomial evaluation (EvalPoly :1291, EvalMultMany :1297, EvalChebyshevFunction :1319-1335)
    CtPtr eval_poly(const CtPtr& x, const std::vector<double>& coeffs);                 // power basis
    CtPtr eval_chebyshev(const CtPtr& x, const std::vector<double>& coeffs, double a, double b);  // sum' c_k T_k(u), u = affine map of [a,b] to [-1,1]
    CtPtr mult_many(const std::vector<CtPtr>& v);
    // the same on several inputs / operand lists at once: every multiplication round is ONE batched relinearisation over all of them
    std::vector<CtPtr> eval_poly_many(const std::vector<CtPtr>& xs, const std::vector<double>& coeffs);
    std::vector<CtPtr> mult_many_rows(const std::vector<std::vector<CtPtr>>& vs);
    CtPtr rescale(const CtPtr& a);                           // drop one limb, divide the scale by it
    CtPtr level_reduce(const CtPtr& a, int new_ell);         // drop limbs without scaling
    // bring `a` to (ell, deg) with scale `scale` following the FLEXIBLEAUTO rules
    CtPtr adjust(const CtPtr& a, int ell, int deg, long double scale);

    // raw, no bookkeeping (parity tests): exactly the residue functions of the oracle
    CtPtr raw_rescale(const CtPtr& a);
    // qlm_row / qlinv_row (optional): the tables of a dropped modulus that is not q_{ell-1} of the chain (the unwrap drops p_0 from a
    // wrapped input over q_0..q_{n_q-1}, p_0: limb id ell-1 is then p_0's) - q_drop mod q_t and (q_drop^-1 mod q_t, Shoup)
    void lift_and_ntt(u64* lifted, const u64* last, int P, int ell, const NttEpilogue* ep = nullptr, const u64* qlm_row = nullptr);
    // K5 steps 2-4: out [P][ell-1][N] = (c - NTT(centred lift of last)) * q_{ell-1}^-1, c [P][ell][N]
    void rescale_finish(u64* out, const u64* c, const u64* last, int P, int ell, const u64* qlinv_row = nullptr, const u64* qlm_row = nullptr);
    CtPtr raw_rotate(const CtPtr& a, u64 galois, const EvalKey& key, bool accumulate = false, const u32* map = nullptr);   // map: galois' own, if at hand
    CtPtr rotate_add(const CtPtr& a, int index);            // a + rot(a, index), one fused key switch (rotsum step :833)
    CtPtr raw_mult_relin(const CtPtr& a, const CtPtr& b, const EvalKey& key);
    // K9 ModRaise (EvalBootstrap's first step): a ciphertext with ONE limb (modulus q0) -> new_ell limbs, every coefficient's
    // centred representative read modulo each q_t.  Scale / degree / slots are copied; the caller sets what they mean.
    CtPtr raw_modraise(const CtPtr& a, int new_ell);

private:
    Context& c_;
    // the one body of rotate_galois_batch and switch_key_batch (evaluator.cpp)
    std::vector<CtPtr> keyswitch_groups(const std::vector<CtPtr>& vin, const EvalKey& key, const u32* map, bool accumulate, bool by_limbs,
                                        const char* two_components);
    void keyswitch_impl(int batch, const KsRows* rows, const u64* c_ntt, size_t c_stride, int ell, const EvalKey* key, u64* out,
                        size_t out_stride, const u64* add0, const u64* add1, size_t add_stride, const u32* map, const u64* post,
                        size_t post_stride);
    // ---- the stages every key switch is built from (evaluator.cpp "key-switch stages"): the place to change the pipeline
    struct KsStrides { size_t c = 0, out = 0, add = 0, post = 0; };   // the element strides of a KsShape, in the struct's own order
    KsShape ks_shape(int ell, int batch, const KsStrides& st) const;    // ell, k, alpha, beta, L1 from the context
    // the tail an accumulator is meant for, named when it is made: what may be left to the tail's transforms follows from it alone
    enum class KsTail {
        RowPass,     // moddown, finished in the row pass of NTT(conv)
        Finish,      // moddown, finished by launch_moddown_finish (or by the caller's own launches after moddown_conv)
        Rescale,     // moddown_rescale
        Exact,       // moddown_rescale_exact
        EditsAccP,   // moddown_rescale after the caller has worked on accP, which must then hold the residues themselves
    };
    // what lives between a key switch's inner product and its tail: made by inner_product or accumulators, consumed by ONE tail
    struct KsAcc {
        KsShape sh;          // the shape as decided: accp_rows / accq_rows are set here and nowhere else
        KsTail tail;
        Scratch<u64> accQ;   // [sh.batch][2][ell][N]; empty with sh.accq_rows
        Scratch<u64> accP;   // [sh.batch][2][K, or sh.accp_limbs][N]
        NttProduct qprod;    // with sh.accq_rows: the Q-limb sums, for the tail's row pass to form
    };
    // where a ModDown's result goes: out = .. + add0 / add1 (+ post), written through `map`; as constructed: the identity, no addends
    struct KsOut {
        u64* out = nullptr;
        const u64 *add0 = nullptr, *add1 = nullptr, *post = nullptr;
        const u32* map = nullptr;
    };
    enum class KsOutput { Identity, Gathered, Scattered, MergedSum };
    KsTail moddown_tail(KsOutput o) const;   // RowPass or Finish: the one reading of FHELIN_FUSE_MODDOWN / _FUSE_FINISH / _ROT_GATHER
    // a plain rotation that gathers at the inner product (KsShape::gather) into its shape: the keys' permuted copies, the inverse Galois
    // elements, optionally c0 (into accQ times P).  sh.per_row: one key and map per row; else one of each, and that key is returned
    const u64* set_gather(KsShape& sh, const EvalKey* const* keys, const u32* const* maps, const u64* c0 = nullptr, size_t c0_stride = 0);
    Scratch<u64> modup(const KsShape& up, const u64* src, bool times_r2, int group2 = 0, size_t group2_stride = 0);
    // evk: the one key of every row, or null: the shape's own - per row (sh.evk_row) or, a merged sum (sh.n_rot > 0), per rotation (sh.evk_rot)
    KsAcc inner_product(const KsShape& sh, const u64* ext, const u64* evk, const u64* c_ntt, KsTail tail);
    KsAcc accumulators(const KsShape& sh, KsTail tail);   // for a caller that launches its own inner product: both buffers, nothing decided
    bool accp_in_rows(const KsShape& sh, KsTail tail) const;   // FHELIN_FUSE_ACCP_ROWS: the class rule of DESIGN.md 6j
    bool accq_in_rows(const KsShape& sh, KsTail tail) const;   // FHELIN_FUSE_ACCQ_ROWS: the class rule of 6k
    void accp_inverse(KsAcc& acc);   // INTT(accP) of a tail: the column pass alone with sh.accp_rows
    // the first half of moddown: conv [sh.batch][2][ell][N] from accP, in NTT form unless the tail is RowPass (whose row pass transforms it)
    Scratch<u64> moddown_conv(KsAcc& acc);
    void moddown(KsAcc& acc, const KsOut& o);
    // the last kernel of a row-pass ModDown: o.out = (accQ - NTT(conv)) * P^-1 + add (+ post) in the row pass of NTT(conv); with sh.accq_rows
    // accQ is formed there from acc.qprod
    void moddown_rows(const KsAcc& acc, u64* conv, const KsOut& o);
    void moddown_rescale(KsAcc& acc, u64* out);
    void moddown_rescale_exact(KsAcc& acc, u64* out, u32 f2);
    // logical slot count of a ciphertext (slots = 0: the context's)
    int slot_count(int slots) const;
    int slot_count(const CtPtr& a) const { return slot_count(a->slots); }
    // key, automorphism map and Galois element of a rotation index; FHELIN_ERR_KEY when the key was not generated
    struct RotKey {
        const KeyPtr& key;   // the entry of rot_keys
        const u32* map;
        u64 g;
    };
    RotKey rotation_key(int index);
    // the rotations of a merged key switch, looked up once per call: keys, maps, and whether every map keeps the 512-coefficient tiles
    struct Rotations {
        int n = 0;
        const EvalKey* key[KsShape::MAX_ROT] = {};
        const u32* map[KsShape::MAX_ROT] = {};
        bool tiles_in_place = true;
    };
    Rotations rotations(const int* indices, int n);
    // bind_key for every rotation of `rot` at the limbs each operand will be switched at (a degree-2 operand is rescaled first when
    // rescales_first): the refusal of a batched call comes before its first group runs
    void bind_rotations(const Rotations& rot, const std::vector<CtPtr>& v, bool rescales_first = false);
    void set_rotations(KsShape& sh, const Rotations& rot, bool shared_digits, const u64* const* keys = nullptr);
    void rotation_sum(KsShape& sh, const u64* ext, const u64* base, size_t c0_stride, const KsOut& o);
    // every degree-2 ciphertext of the list(s) replaced by its rescaled one: one rescale_batch over the distinct ones; FHELIN_ERR_STATE
    // (`what`) for an operand that does not have two components, before anything runs
    void rescale_degree2(std::vector<CtPtr>& a, std::vector<CtPtr>* b = nullptr, const char* two_components = nullptr);
    // the tensor products x[idx[k]] (x) y[idx[k]] of one group: a block [B][3][ell][N], one launch per 32 pairs
    std::vector<CtPtr> tensor_products(const std::vector<CtPtr>& x, const std::vector<CtPtr>& y, const std::vector<size_t>& idx);
    // operands of a batched product as mult_batch takes them: degree 2 rescaled first (every distinct ciphertext once), pairs matched
    void product_operands(const std::vector<CtPtr>& a, const std::vector<CtPtr>& b, std::vector<CtPtr>& x, std::vector<CtPtr>& y);
    // the unmerged sequence of mult_affine_batch: mult_batch, add_batch (factor 2), add_real per item, sub_batch / add_batch, rescale_batch
    std::vector<CtPtr> mult_affine_unmerged(const std::vector<CtPtr>& a, const std::vector<CtPtr>& b, const std::vector<AffineSpec>& spec);
    // a plain rotation gathers at the inner product and ends in the same identity ModDown (KsShape::gather); FHELIN_FUSE_MODDOWN=1 keeps
    // its scattered epilogue
    bool rot_in_gather() const { return c_.fuse_finish && c_.rot_gather && !c_.fuse_moddown; }
    // NTT(conv) [batch][2][ell-1][N] and the merged ModDown + rescale finish into out (launch_moddown_rescale_finish)
    void moddown_rescale_finish(const KsAcc& acc, u64* out, u64* conv, const u64* minv);
    typedef std::vector<CtPtr> CtRow;  // one value per input ciphertext
    CtRow cheb_recurse(const std::vector<double>& c, const std::vector<CtRow>& T, const std::map<int, CtRow>& G, int baby);
    std::vector<CtPtr> add_sub_batch(const std::vector<CtPtr>& a, const std::vector<CtPtr>& b, int op);
    void match(const CtPtr& a, const CtPtr& b, CtPtr& ao, CtPtr& bo);
    void match_batch(const std::vector<CtPtr>& a, const std::vector<CtPtr>& b, std::vector<CtPtr>& x, std::vector<CtPtr>& y);
};

}  // namespace fhelin
