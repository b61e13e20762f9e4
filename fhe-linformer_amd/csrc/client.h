// Client-side CKKS: key generation, encode/decode (special FFT, fp64), public-key encryption, decryption.
// Mirrors reference FHEController::generate_context / generate_*_keys / encode / encrypt / decrypt
// (src/FHEController.cpp:47-49, :237-273, :348-404).  Sampling and the fp64 FFT run on the host (as in the
// reference); every residue-polynomial operation (NTT, dyadic products) runs on the GPU kernels.
#pragma once
#include <functional>
#include <vector>
#include "evaluator.h"
#include "kernels_client.h"

namespace fhelin {

// Cryptographic pseudo-random generator: the ChaCha20 stream (RFC 8439 block function, 20 rounds) keyed with a 256-bit
// secret seed; 64-bit block counter (state words 12-13), 64-bit stream id (words 14-15).  Every secret the client samples
// (secret key, encryption randomness, key-switching-key noise and masks) comes from this stream.
struct Prng {
    static constexpr int LANES = 8;                // blocks produced per refill
    explicit Prng(const uint8_t seed[32], u64 stream = 0);
    u64 next();
    u64 uniform(u64 q);        // unbiased in [0, q)
    double normal();           // standard normal (Box-Muller)
    // one 64-byte block for the given (counter, stream): known-answer tests against RFC 8439
    static void block(const uint8_t seed[32], u64 counter, u64 stream, uint8_t out[64]);
private:
    u32 key_[8];
    u64 counter_ = 0, stream_ = 0;
    u32 buf_[16 * LANES];
    int pos_ = 16 * LANES;     // u32 words consumed of buf_
    void refill();
    bool have_spare = false;
    double spare = 0;
};

class Client {
public:
    Client(Evaluator& ev, const uint8_t seed[32]);
    ~Client();
    void keygen();                       // secret (sparse ternary) + public key
    bool has_keys() const { return s_all != nullptr; }
    // Evaluation context (include/fhelin.h fhelin_evalkeys_load): public key and switching keys imported from a set, no secret.
    // Key generation then only confirms keys that are present; decryption and everything else that needs s fails (FHELIN_ERR_KEY).
    bool eval_only() const { return eval_only_; }
    bool keygen_run() const { return keygen_run_; }   // keygen() or import_secret() ever ran on this context
    bool has_public_key() const { return pk != nullptr; }
    const u64* public_key() const { return pk; }      // device [2][L+1][N]
    // takes ownership (a pool block); makes this an evaluation context.  seeded: its a half is the key-set seed's expansion
    void install_public_key(u64* d_pk, bool seeded = false);
    void gen_relin_key();                // EvalMultKeyGen
    void gen_rotation_key(int index);    // EvalRotateKeyGen for one index
    void gen_conj_key();
    // Sparse-secret bootstrapping (include/fhelin.h "Sparse-secret bootstrapping"), once per context: the ephemeral secret s~ (ternary,
    // exactly `hamming` non-zero coefficients, keygen's placement loop on the context's generator), then the to-sparse key s -> s~
    // (kind 4, always capped at two limbs) and the from-sparse key s~ -> s (kind 5, capped by a table entry of its kind), in this
    // order.  Without the secret: confirms that both keys are present (FHELIN_ERR_KEY names the missing one)
    void gen_sparse_keys(int hamming);
    bool has_sparse_secret() const { return s_sparse != nullptr; }
    const std::vector<int8_t>& sparse_secret() const { return sparse_coeffs_; }   // the coefficients of s~ (test hook)
    // device [L+1+k][N] NTT form.  kind / galois: the key's nonce fields in seeded-key mode (include/fhelin.h "Seeded evaluation keys")
    // force_cap > 0: the key is capped at that many limbs whatever the cap table says
    KeyPtr make_switch_key(const u64* s_from_all, const u64* s_to_all, u64 kind, u64 galois, int force_cap = 0);
    // Level-capped keys (include/fhelin.h "Level-capped keys"): every switching key made from now on whose (kind, Galois element) has an
    // entry is made capped at the entry's limbs (make_switch_key); an entry of n_q limbs, or none, is an uncapped key.  Replaces the table.
    // kind 1 relinearisation (galois 0), 2 rotation, 3 conjugation (galois 2N-1), 4 to-sparse and 5 from-sparse (galois 0; the to-sparse
    // key is held at two limbs whatever its entry says).  The caller validates (fhelin_ctx_set_key_caps).
    struct KeyCap {
        int kind;
        u64 galois;
        int max_ell;
    };
    void set_key_caps(const std::vector<KeyCap>& table);
    int key_cap(int kind, u64 galois) const;   // n_q where the table has no entry

    // Seeded-key mode (include/fhelin.h "Seeded evaluation keys"): keygen draws a public key-set seed and every key's a half is
    // its expansion, made on the device by seeded_keygen_combine_kernel.  Off: key generation consumes the generator as before.
    void set_seeded_keys(bool on) { seeded_keys_ = on; }
    bool seeded_keys() const { return seeded_keys_; }
    bool has_key_seed() const { return has_key_seed_; }
    const uint8_t* key_seed() const { return key_seed_; }
    bool public_key_seeded() const { return pk && pk_seeded_; }
    void install_key_seed(const uint8_t seed[32]);    // an evaluation context loaded from a compact set

    PtPtr encode(const double* vals, int n, int level, int slots);
    CtPtr encrypt(const PtPtr& p, int drop = 0);   // drop: limbs left out below the plaintext's level (level plan)
    // n_vec real vectors of n_per values each (row-major) -> n_vec fresh ciphertexts at `level`: encoding (special FFT, scaling,
    // rounding), sampling of (u, e0, e1) and the dyadic combination all on the GPU, in batched launches
    // nonce_of (seeded mode): null = a call of its own (a fresh seed, nonce = vector index); else the output index of every vector
    // within a call whose seed the caller drew with begin_call()
    // per_lane (interleaved samples): vals [n_vec][stride][n_per], sample i of a vector in the physical slots = i mod stride; otherwise every
    // vector is replicated into all lanes.  The interleaving happens in front of the encoder and draws nothing.
    std::vector<CtPtr> encrypt_batch(const double* vals, int n_vec, int n_per, int level, int slots, const int* nonce_of = nullptr,
                                     bool per_lane = false);
    std::vector<CtPtr> ingest_sample(const double* emb, const int* tokens, const double* table, int vocab, int S, const double* cls,
                                     const double* pos, const double* E_w, const double* E_b, const double* F_w, const double* F_b,
                                     int w_cols, int level, const std::vector<int>& drop, std::vector<double>* proj_out = nullptr,
                                     const std::vector<int>* wrap_ell = nullptr);
    // `stride` samples of one length S in one group of 64 + S + 1 ciphertexts (interleaved samples): emb / tokens [stride] pointers (emb
    // null: token ids), everything else shared; proj_out [stride] as ingest_sample's; wrap_ell as ingest_sample's (the group's wrapped
    // ciphertexts: the same inputs of every sample in one ciphertext)
    std::vector<CtPtr> ingest_interleaved(const double* const* emb, const int* const* tokens, const double* table, int vocab, int S,
                                          const double* cls, const double* pos, const double* E_w, const double* E_b, const double* F_w,
                                          const double* F_b, int w_cols, int level, const std::vector<int>& drop,
                                          std::vector<std::vector<double>>* proj_out = nullptr,
                                          const std::vector<int>* wrap_ell = nullptr);
    // wrap_ell (include/fhelin.h "Wrapped inputs"): the limbs every input is wanted at; the result is then the WRAPPED ciphertexts (runs
    // of inputs of one target in read order, <= 128 each, over ell + 1 limbs), always seeded secret-key encryptions; drop is ignored
    // test hook: the sampler's raw output, n_poly polynomials of N centred coefficients (kind 0 Gaussian, 1 ternary)
    std::vector<long> debug_sample(int kind, int n_poly);
    // flood_bits > 0 (include/fhelin.h "Sanitised replies"): one uniform polynomial on [-2^flood_bits, 2^flood_bits) is added to the phase
    // on the device, after the inverse NTT and before the download; 0: the plain decryption, unchanged
    std::vector<double> decrypt(const CtPtr& c, int slots, int flood_bits = 0);   // interleaved samples: lane 0
    std::vector<double> decrypt_interleaved(const CtPtr& c, int slots, int flood_bits = 0);   // [stride][slots]: every lane
    // Batched decryption (include/fhelin.h "Batched decryption"): the decoder on the device, bit for bit the doubles decrypt gives.
    // out [n][L][W] on the host: L = stride with all_lanes (decrypt_interleaved's order) else 1 (lane 0, decrypt's), W = n_idx when idx
    // (logical slot numbers in [0, slots)) is given, else slots; slots <= 0: the ciphertexts' own count, which must agree.  The batch may
    // mix limb counts, scales, degrees and wrapped inputs.  One phase launch, ONE inverse NTT over every limb read, the lift, the forward
    // special FFT and the gather for the whole batch, ONE download and ONE stream synchronisation.  flood_bits > 0: one key draw per
    // call, the flood of ciphertext b on stream (C << 32) + b, C += 2 - a batch of one is decrypt(c, slots, flood_bits), a batch of n
    // is not n single calls.  Every refusal comes before the first draw.
    void decrypt_batch(const std::vector<CtPtr>& cts, int slots, int flood_bits, bool all_lanes, const int* idx, int n_idx, double* out);
    // Reply sanitisation (include/fhelin.h "Sanitised replies"): degree-2 inputs rescaled, the optional 0/1 mask applied (product +
    // rescale), then out_b = first out_ell limbs of x_b + Enc_pk(0) + flood in ONE fused launch for the whole batch; the randomness
    // scratch is wiped.  Needs the public key only (works on an evaluation context).
    std::vector<CtPtr> sanitize(const std::vector<CtPtr>& v, const PtPtr& mask, int flood_bits, int out_ell);
    // test hook: the flood sampler alone for an explicit ChaCha20 key and stream, residues [ell][N] (coefficient form)
    std::vector<u64> debug_flood(const uint8_t key[32], u64 stream, int flood_bits, int ell);
    // test hook (include/fhelin.h "Sampler streams"): the keys the next n_keys sampler-key draws (sample_small_device,
    // draw_sampler_key) will return, key_words [n_keys][8], computed on a COPY of the generator - nothing is consumed - and the
    // current sampler call counter.  No device work.
    void debug_sampler_peek(int n_keys, u32* key_words, u64* sample_calls) const;
    CtPtr phase(const CtPtr& c, int nlimbs);   // c0 + c1 s (+ c2 s^2) on the first nlimbs limbs, NTT form, 1 component

    // raw import/export of key material (parity tests feed identical arrays to the oracle)
    // Seeded mode (include/fhelin.h fhelin_ctx_set_seeded_encryption): encrypt / encrypt_batch / ingest_sample encrypt with the
    // secret key, c0 = m - a s + e, c1 = a with a expanded from a fresh 32-byte seed per call and nonce = output index in the call
    void set_seeded(bool on);
    bool seeded() const { return seeded_; }
    void begin_call();                   // seeded mode: draw the next call's seed from the generator (no-op otherwise)

    void export_secret(u64* out);        // [L+1+k][N]
    void import_secret(const u64* in);   // replaces the secret (NTT form) — tests only

private:
    Evaluator& ev_;
    Context& c_;
    Prng rng_;
    u64* s_all = nullptr;   // secret, NTT form over Q and P limbs [L+1+k][N]
    u64* pk = nullptr;      // [2][L+1][N]: b = -a s + e, a
    u64* s_sparse = nullptr;             // the ephemeral secret s~ of sparse-secret bootstrapping, as s_all; never on an evaluation context
    std::vector<int8_t> sparse_coeffs_;  // its N coefficients
    // the placement loop of a sparse ternary secret: h distinct positions, a sign each; co [2N] sign-extended 128-bit pairs, zero on entry
    void place_sparse_ternary(std::vector<u64>& co, int h);
    void sample_small_to_ntt(u64* dst, int nlimbs_q, bool with_p, int kind);  // kind 0 gaussian, 1 ternary (host sampler: key generation)
    void draw_small_host(std::vector<u64>& co, int kind);   // its draws alone: N coefficients as sign-extended 128-bit pairs
    std::map<std::pair<int, u64>, int> key_caps_;
    // device sampler (encryption randomness): dst [n_poly][ell][N] coefficient form; a fresh ChaCha20 key per call
    void sample_small_device(u64* dst, int n_poly, int ell, int kind);
    // the wide sampler (launch_sample_flood), keyed as sample_small_device; gauss: e0 + f as one polynomial
    void sample_flood_device(u64* dst, int n_poly, int ell, int flood_bits, bool gauss);
    SamplerKey draw_sampler_key();
    void check_flood(int flood_bits, int nl, const char* who) const;   // 0..62 and 2^(flood_bits + 2) below q_0 .. q_{nl-1}
    // c0 = b u + e0 + m, c1 = a u + e1 for n_vec encodings enc [n_vec][ell][N] (enc_stride words apart; 0 = one shared encoding)
    // seeded mode: c0 = m - a s + e, c1 = a instead; nonces [n_vec] are the vectors' output indices within the current call
    void encrypt_encoded(const u64* enc, size_t enc_stride, int n_vec, int ell, long double scale, int slots, std::vector<CtPtr>& out,
                         const u64* nonces);
    // wrapped inputs, shared by ingest_sample and ingest_interleaved: the grouping by target and the seeded encryption of the packed vectors
    void wrap_groups(const std::vector<int>& wrap_ell, int n_vec, std::vector<int>& group_ell, std::vector<int>& pos) const;
    std::vector<CtPtr> encrypt_wrapped(double* dv, int phys, int slots, int n_vec, const std::vector<int>& group_ell,
                                       const std::vector<int>& pos, const std::function<void*(size_t)>& get);
    std::vector<double> decrypt_physical(const CtPtr& c, int slots, int flood_bits, int mult);
    u64 sample_calls_ = 0;
    bool eval_only_ = false, keygen_run_ = false;
    bool seeded_ = false;
    uint8_t call_seed_[32] = {};
    bool seeded_keys_ = false, has_key_seed_ = false, pk_seeded_ = false;
    uint8_t key_seed_[32] = {};
    SamplerKey key_seed_words() const;
};

// special FFT helpers (shared by encode/decode); slots must be a power of two
void ckks_fft_special(std::vector<std::pair<double, double>>& v, bool inverse);
// tables of the special FFT for `slots` slots: rot[j] = 5^j mod 4*slots, ksi[k] = exp(2 pi i k / (4*slots))
void ckks_fft_tables(int slots, std::vector<u32>& rot, std::vector<std::pair<double, double>>& ksi);
// stride > 1 (interleaved samples): slots logical values, each replicated into the stride lanes of the slots * stride physical slots
std::shared_ptr<Encoding> encode_to_device(Context& c, const std::vector<double>& values, const std::vector<double>& imag, int slots,
                                           int ell, long double scale, int stride = 1, int ell_q = 0);
// the encoder's domain: throws FHELIN_ERR_ARG for a non-finite max_abs, or when the two exponents allow max_abs * scale >= 2^125
void encode_domain_check(double max_abs, long double scale);
// device encoder for n_vec vectors: re / im [n_vec][n_per] (im may be null) -> dst [n_vec][ell][N] NTT form
// stride > 1: re / im [n_vec][lanes][n_per] with lanes = stride (lane i = sample i) or 1 (the vector replicated); the staged uploads stay at
// logical size and launch_interleave_slots makes the physical vectors in front of the inverse FFT
void encode_batch_device(Context& c, u64* dst, const double* re, const double* im, int n_vec, int n_per, int slots, int ell, long double scale,
                         int stride = 1, int lanes = 1, int ell_q = 0);
// ell_q > 0: the limb-sliced form, ell == ell_q + k rows: Q limbs 0..ell_q-1, then the k special limbs (Plaintext::at_sliced)
void encode_complex_on_device(Context& c, u64* dst, double* dv, int n_vec, int slots, int ell, long double scale, int ell_q = 0);

}  // namespace fhelin
