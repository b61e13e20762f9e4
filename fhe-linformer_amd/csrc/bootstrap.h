// CKKS bootstrapping on the GPU evaluator: ModRaise -> (SubSum) -> CoeffsToSlots -> approximate modular
// reduction (Chebyshev cosine + double-angle) -> SlotsToCoeffs.  Mirrors what the reference obtains from
// OpenFHE's EvalBootstrapSetup / EvalBootstrapKeyGen / EvalBootstrap (reference src/FHEController.cpp
// :237-240, :280, :438-469; level budget {3,3}, 16384 slots, sparse ternary secret).
#pragma once
#include <complex>
#include <map>
#include <vector>
#include "client.h"
#include "evaluator.h"

namespace fhelin {

typedef std::complex<double> cplx;
typedef std::map<int, std::vector<cplx>> DiagMap;  // rotation (mod slots) -> diagonal: out = sum_r d_r * rot(in, r)

// one level of the homomorphic DFT, prepared for baby-step / giant-step evaluation
struct LinStage {
    int g0 = 1;    // all rotation indices are multiples of g0
    int bsz = 1;   // baby-step count
    struct Term {
        int giant;   // giant shift (slots), applied after the inner sum
        int baby;    // baby shift (slots)
        PtPtr diag;  // diagonal, pre-rotated by -giant
    };
    std::vector<Term> terms;
    // the engine form of the same terms (Bootstrapper::set_lt on; empty otherwise): the argument lists of
    // Evaluator::linear_transform_rows - baby[b] = b * g0 for b < bsz, the giant steps that carry a term in ascending order, pts [n2][bsz]
    // with null where no diagonal falls
    std::vector<int> lt_baby, lt_giant;
    std::vector<std::vector<PtPtr>> lt_pts;
};

class Bootstrapper {
public:
    Bootstrapper(Evaluator& ev, Client& cl) : ev_(ev), cl_(cl) {}
    ~Bootstrapper();
    void setup(int budget_enc, int budget_dec, int slots);
    bool ready() const { return slots_ > 0; }
    // Linear stages on the linear-transform engine (include/fhelin.h "Bootstrap linear stages"): every stage is split into
    // at most 32 baby steps (n1 == 0: the planner's cost 4 (n2 + ceil(R / 7)) + baby keys picks per stage; n1 > 0: forced, capped by the
    // stage's span) and applied as ONE Evaluator::linear_transform_rows call over the batch - one ModUp, the baby steps' key products
    // formed once in QP, n2 + ceil(R / 7) pair-ModDowns.  The split decides the diagonals' pre-rotation and the key list, so the knob binds
    // at setup(): FHELIN_ERR_STATE afterwards.  Off (the default): nothing below changes
    void set_lt(bool on, int n1);
    bool lt() const { return lt_; }
    int lt_n1() const { return lt_n1_; }
    // device bytes of the limb-sliced encodings the stages' diagonals hold (one per (limbs, scale) a term was applied at)
    size_t lt_encoding_bytes() const;
    // Sparse-secret encapsulation (include/fhelin.h "Sparse-secret bootstrapping"): hamming = h~ > 0 switches to an
    // ephemeral secret of that weight around the ModRaise - the two-limb ciphertext in front of the rescale to q0 goes to s~, the raised
    // one comes back to s - so that |I| is bounded by the smaller K this call writes together with R and cheb_degree (a later
    // fhelin_bootstrap_config overrides them).  0: off, nothing below changes.  8 <= h~ <= N (FHELIN_ERR_ARG otherwise); the secret and
    // the two keys are made by setup(): FHELIN_ERR_STATE afterwards
    void set_sparse(int hamming);
    int sparse_h() const { return sparse_h_; }
    // the degree the knob writes for a K: the largest one Evaluator::cheb_depth evaluates in five levels where the range allows it
    static constexpr int SPARSE_MAX_K = 12, SPARSE_CHEB_DEGREE = 28;
    // drop: raise to L+1-drop limbs only, so that the result has `drop` limbs fewer (level plan: the caller knows that the
    // circuit up to the next bootstrap leaves that many unused)
    CtPtr bootstrap(const CtPtr& ct, int drop = 0);
    // several independent ciphertexts at once (the GELU containers of one sample, src/main.cpp:354-358; the two halves of
    // affine-1, :319-320): every launch of the pipeline carries all of them, the switching keys and plaintext diagonals are
    // read once per batch.  out[i] holds exactly the residues of bootstrap(cts[i], drop).
    std::vector<CtPtr> bootstrap_batch(const std::vector<CtPtr>& cts, int drop = 0);
    // Iterative (two-pass) bootstrapping, OpenFHE's EvalBootstrap(ct, 2, p) as this engine defines it: y = BTS(x),
    // z = BTS(2^p (y - x)) at x's two limbs and scale, out = rescale(k (2^p y - z)) with k = round(Delta_next q_top / (2^p s_y)).
    // The result keeps about twice the bits of one bootstrap and has one limb fewer than it.  1 <= p <= 30 (FHELIN_ERR_ARG
    // otherwise); 2^p |y - x| must stay inside the bootstrap's input range, so p at or below one bootstrap's precision is useful.
    // drop as for bootstrap(); one bootstrap's output must keep >= 3 limbs (FHELIN_ERR_STATE otherwise).
    CtPtr bootstrap_iter(const CtPtr& ct, int p, int drop = 0);
    // both bootstraps as bootstrap_batch over all inputs; out[i] holds exactly the residues of bootstrap_iter(cts[i], p, drop)
    std::vector<CtPtr> bootstrap_iter_batch(const std::vector<CtPtr>& cts, int p, int drop = 0);
    static constexpr int MAX_ITER_PRECISION = 30;
    // Paired bootstrapping: two ciphertexts with REAL slot values go through one pipeline as a + i b and are taken apart by
    // one conjugation at the output level.  Consecutive inputs are paired, (0,1), (2,3), ...; an odd last input, and both inputs of a pair
    // whose slot counts differ, travel in the same batched pipeline as singles (exactly the residues of bootstrap(ct, drop)).  Every
    // output has the limbs, degree and nominal scale of bootstrap(cts[i], drop); correction == 0 leaves no bit for the 1/2 of the split
    // (FHELIN_ERR_STATE).  The bootstrap counter advances once per pipeline.
    std::vector<CtPtr> bootstrap_pairs(const std::vector<CtPtr>& cts, int drop = 0);
    // a and b as one pair whatever else holds: unequal slot counts are FHELIN_ERR_ARG
    std::pair<CtPtr, CtPtr> bootstrap_pair(const CtPtr& a, const CtPtr& b, int drop = 0);
    // debug / test hook: stop after stage 1 (ModRaise+SubSum), 2 (CoeffsToSlots, real part), 3 (EvalMod, real part)
    CtPtr partial(const CtPtr& ct, int stage);
    CtPtr pair_partial(const CtPtr& a, const CtPtr& b, int stage);   // the same stages of the pair's one pipeline
    // the two kernels of a paired bootstrap on their own (kernels_elem.h launch_ew_pair_pack / launch_ew_pair_split; the debug entries
    // of include/fhelin.h reach them): out[i] = ka[i] a[i] + i kb[i] b[i] on the two bottom limbs, one block, degree a's + 1, scale
    // a's x ka; and (w + wc, i (wc - w)) per pair of one shape, at w's degree, scale and slots
    std::vector<CtPtr> pack_pairs(const std::vector<CtPtr>& a, const std::vector<CtPtr>& b, const std::vector<u64>& ka, const std::vector<u64>& kb);
    void split_pairs(const std::vector<CtPtr>& w, const std::vector<CtPtr>& wc, std::vector<CtPtr>& out_a, std::vector<CtPtr>& out_b);
    int depth() const { return depth_; }
    int out_ell() const { return ev_.ctx().L + 1 - depth_; }   // limbs of the result when nothing is dropped
    // read-only views for the residue-level parity tests (include/fhelin.h fhelin_bootstrap_describe / _diag / _cheb): the
    // oracle composes the same stages from the diagonals' exported encodings
    const std::vector<LinStage>& stages(bool s2c) const { return s2c ? s2c_ : c2s_; }
    const std::vector<double>& cheb() const { return cheb_; }
    bool packed() const { return packed_; }
    int slots() const { return slots_; }                   // of the physical packing the stages are built for
    int logical_slots() const { return logical_slots_; }   // as setup() was asked: slots() / the interleave stride
    int budget_enc() const { return budget_enc_; }   // as setup() was called (evaluation-key sets record them)
    int budget_dec() const { return budget_dec_; }

    // parameters (DESIGN.md "Bootstrapping")
    int K = 28;            // bound on |I|: t = Delta m + q0 I
    int R = 3;             // double-angle iterations
    int cheb_degree = 47;  // degree of the cosine fit (depth 6: Evaluator::cheb_depth)
    int correction = 10;   // message is scaled to q0 / 2^correction before ModRaise

private:
    Evaluator& ev_;
    Client& cl_;
    int slots_ = 0, logical_slots_ = 0;
    int budget_enc_ = 0, budget_dec_ = 0;
    bool stage_order_legacy_ = false;   // FHELIN_BOOT_STAGES_LEGACY=1: larger stages first (round-1 split 5+5+4)
    bool lt_ = false;       // set_lt
    int lt_n1_ = 0;
    int sparse_h_ = 0;      // set_sparse
    bool packed_ = false;   // sparse packing: real and imaginary halves share one ciphertext through EvalMod (bootstrap.cpp)
    int depth_ = 0;
    std::vector<LinStage> c2s_, s2c_;
    std::vector<double> cheb_;
    u64* mono_i_ = nullptr;  // NTT of X^{N/2} over the Q limbs: multiplication by i

    LinStage prepare(const DiagMap& m, int n);   // n: slots the stage's diagonals are written over
    CtPtr apply(const LinStage& st, const CtPtr& x);
    CtPtr mult_i(const CtPtr& x);
    CtPtr mod_raise(const CtPtr& ct, long double& rho, int top_ell);
    std::vector<CtPtr> eval_mod(const std::vector<CtPtr>& xs);
    CtPtr run(const CtPtr& ct, int stop_after, int drop = 0);
    std::vector<CtPtr> apply_batch(const LinStage& st, const std::vector<CtPtr>& xs);
    std::vector<CtPtr> run_batch(const std::vector<CtPtr>& cts, int drop);
    // one item of a batched pipeline: the single a, or (b set) the pair a + i b
    struct Item {
        CtPtr a, b;
    };
    // per-item prologue (message to q0 / 2^correction: integer multiply, or the pack of a pair), the shared core over all items, per-item
    // epilogue (the exact 2^correction, or half of it and the split of a pair).  Results in item order, two per pair; stop_after > 0: one
    // per item, the pipeline's state after that stage (partial())
    std::vector<CtPtr> run_items(const std::vector<Item>& items, int drop, int stop_after = 0);
    void ensure_mono_i();
};

}  // namespace fhelin
