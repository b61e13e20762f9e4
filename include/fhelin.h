/*
 * fhelin.h — C ABI of the MI355X-native RNS-CKKS evaluation engine (libfhelin_amd.so).
 *
 * This is the drop-in boundary underneath the reference's `class FHEController`
 * (reference src/FHEController.h:22-161).  The reference binds OpenFHE's C++ objects directly
 * (`CryptoContext<DCRTPoly> context`, `Ciphertext<DCRTPoly>`, `Plaintext`; src/FHEController.h:19-23);
 * a maintainer replaces those with the opaque handles below (see INTEGRATION.md and the
 * source-compatible shim include/FHEController.h).  Every entry point cites the reference call site
 * it stands in for.  All functions return 0 on success or an FHELIN_ERR_* code; the message of the
 * last failure on the calling thread is available from fhelin_last_error().
 *
 * Conventions
 *  - plain C types only: pointers, sizes, integers, doubles.  No torch / HIP types in signatures
 *    (a hipStream_t travels as void*).
 *  - residue data is uint64_t, limb-major: poly[limb][N]; ciphertext = poly 0 then poly 1 (then 2).
 *  - limb ids: Q limbs 0..L, special (P) limbs L+1..L+k.
 *  - device work is asynchronous on the context's stream; fhelin_sync() waits for it (and first issues the deferred
 *    bootstraps / polynomial evaluations whose results nobody has read yet, see fhelin_bootstrap_batch).
 *  - there is NO CPU fallback: on a host-only context (device < 0) every evaluation entry point
 *    fails with FHELIN_ERR_NO_DEVICE.
 */
#ifndef FHELIN_H
#define FHELIN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FHELIN_OK 0
#define FHELIN_ERR_ARG 1
#define FHELIN_ERR_NO_DEVICE 2
#define FHELIN_ERR_HIP 3
#define FHELIN_ERR_STATE 4
#define FHELIN_ERR_KEY 5
#define FHELIN_ERR_INTERNAL 6

typedef struct fhelin_ctx fhelin_ctx;   /* CryptoContext<DCRTPoly>            (FHEController.h:23)  */
typedef struct fhelin_ct fhelin_ct;     /* Ctxt = Ciphertext<DCRTPoly>        (FHEController.h:20)  */
typedef struct fhelin_pt fhelin_pt;     /* Ptxt = Plaintext                   (FHEController.h:19)  */

/* CCParams<CryptoContextCKKSRNS> as set in generate_context (FHEController.cpp:4-35). */
typedef struct fhelin_params {
    int32_t log_n;         /* SetRingDim(1 << log_n)                 :12-13 */
    int32_t n_q;           /* multiplicative depth + 1               :31-35 */
    int32_t first_bits;    /* SetFirstModSize(55)                    :25    */
    int32_t scale_bits;    /* SetScalingModSize(52), FLEXIBLEAUTO    :18-24 */
    int32_t n_p;           /* special primes of HYBRID key switching (OpenFHE-internal); < 0: OpenFHE's rule
                              ceil(bits of the widest digit / special_bits), read it back with fhelin_ctx_info */
    int32_t special_bits;  /* 60                                                       */
    int32_t dnum;          /* SetNumLargeDigits(4)                   :11    */
    int32_t log_slots;     /* SetBatchSize(1 << 14)                  :6,14  */
    int32_t hamming;       /* SPARSE_TERNARY secret weight           :8     */
    int32_t device;        /* HIP device ordinal; < 0 = host-only parameter context */
    uint64_t seed;         /* 0: the client-side generator (ChaCha20) is keyed with 256 bits of OS entropy — the default and the
                              only secure choice; != 0: deterministic 64-bit TEST seed (reproducible tests / benchmarks) */
} fhelin_params;
/* Accepted parameters (fhelin_ctx_create returns FHELIN_ERR_ARG otherwise): 12 <= log_n <= 17; 1 <= n_q <= 64; 0 <= n_p <= 16
 * after resolution; first_bits, scale_bits and special_bits (the last only when n_p > 0) in [20, 60]; digit size
 * ceil(n_q / dnum) <= 16 limbs and at most 16 digits.  Every prime of the resulting chain must lie below 2^60, and a chain that holds
 * one at or above 2^60 is refused.  The scaling primes alternate around 2^scale_bits, so scale_bits = 60 is refused as soon as the
 * chain needs a scaling prime above 2^scale_bits (n_q >= 3); first_bits = 60 and scale_bits = 59 are accepted.  n_p = 0 is a chain without key switching: rotations and relinearisation return FHELIN_ERR_STATE. */

const char* fhelin_last_error(void);
const char* fhelin_version(void);

/* ---- context (GenCryptoContext + Enable(...), FHEController.cpp:37-45) ------------------------ */
int fhelin_ctx_create(const fhelin_params* p, fhelin_ctx** out);
/* the same with an explicit 256-bit secret seed (p->seed ignored): a client re-creating its own keys from its secret-key
 * file, as FHEController::load_context does from ../keys/secret-key.txt (FHEController.cpp:208-214) */
int fhelin_ctx_create_seeded(const fhelin_params* p, const uint8_t* seed32, fhelin_ctx** out);
/* the 256-bit secret seed all key material of this context derives from — SECRET: belongs in the client's secret-key
 * file (FHEController.cpp:80-86 writes secret-key.txt), never next to the public context */
int fhelin_ctx_secret_seed(const fhelin_ctx* c, uint8_t* out32);
/* one 64-byte ChaCha20 block of the client-side generator (known-answer test hook, RFC 8439 section 2.3.2) */
int fhelin_prng_block(const uint8_t* seed32, uint64_t counter, uint64_t stream, uint8_t* out64);
void fhelin_ctx_destroy(fhelin_ctx* c);
int fhelin_ctx_info(const fhelin_ctx* c, fhelin_params* out, int32_t* alpha, int32_t* has_device);
int fhelin_ctx_moduli(const fhelin_ctx* c, uint64_t* out, int32_t cap);          /* Q then P */
int fhelin_ctx_roots(const fhelin_ctx* c, uint64_t* out, int32_t cap);           /* psi per limb */
int fhelin_ctx_scaling_factors(const fhelin_ctx* c, double* out, int32_t cap);   /* real Delta per level */
int fhelin_ctx_set_stream(fhelin_ctx* c, void* hip_stream);                      /* adopt a caller stream */
/* Deferred rows (default on; FHELIN_LAZY_ROWS=0 or on = 0 here: eager).  fhelin_fc_matmul_pt and fhelin_fc_unwrapExpanded
 * return handles whose rows are evaluated when first read (together with the other rows of the same call the reading
 * operation takes) and never if nobody reads them: the reference's drivers compute whole row sets and then use one row
 * (src/main.cpp:183,:196; :416-424).  A forced row holds exactly the residues eager evaluation gives. */
int fhelin_ctx_set_lazy_rows(fhelin_ctx* c, int32_t on);
/* evaluate EXACTLY the deferred rows among v[0..n) now, in one batched call per producing call (a rank of a row-sharded run
 * evaluates the rows it owns and nothing else); handles that are not deferred are left alone */
int fhelin_ct_force(fhelin_ctx* c, const fhelin_ct* const* v, int32_t n);
/* Level plan (profile-guided; off unless asked for).  The reference's drivers are straight-line programs (src/main.cpp:145-475):
 * which ciphertext meets which, and how many limbs every call consumes, does not depend on the data.  A pass run with
 * fhelin_level_plan_begin(ctx, 1) RECORDS, for every handle this boundary gives out, the handles the producing call read
 * and the result's limb count; fhelin_level_plan_end then derives, back to front from the terminals (the input of a
 * bootstrap needs two limbs, as does a decryption / export), the fewest limbs every value may have, and from that the limb
 * count each SOURCE of the pass - the k-th fhelin_encrypt / fhelin_encrypt_batch vector / fhelin_bootstrap call, in call
 * order - should start with.  A later pass of the same program run with fhelin_level_plan_begin(ctx, 2) APPLIES the plan:
 * encryptions are made at the planned level and bootstraps raise to fewer limbs, so that limbs nothing downstream reads
 * (the reference carries e.g. 20 through the V projection, src/main.cpp:212-215, and 4 from the GELU bootstraps to the
 * pooler's, :354-420) are not dragged through the key switches in between.  Values are unchanged up to the noise; a pass
 * that does not follow the recorded program fails loudly at the first bootstrap / decryption that is short of limbs.
 * get/set move the plan (one int32 per source: limbs to start with, -1 = as asked) so that a driver process can keep it
 * next to its keys.  fhelin_ct_import / _import_device values are never lowered; exporting is a terminal. */
int fhelin_level_plan_begin(fhelin_ctx* c, int32_t mode);            /* 0 off, 1 record, 2 apply; resets the source counter */
int fhelin_level_plan_seek(fhelin_ctx* c, int32_t source);           /* apply: the next source is the source-th of the program
                                                                        (a server picking up after the client's encryptions) */
int fhelin_level_plan_tell(fhelin_ctx* c, int32_t* mode, int32_t* source);   /* the mode and the index the NEXT source call will take: a
                                                                        driver that leaves out sources other processes run (rows and
                                                                        bootstraps of one sample sharded over GPUs) reads the position,
                                                                        seeks past the call it skips and back for the ones it runs */
int fhelin_level_plan_end(fhelin_ctx* c, int32_t* n_sources);        /* record: derive the plan; back to mode 0 */
int fhelin_level_plan_get(fhelin_ctx* c, int32_t* target, int32_t cap, int32_t* n);   /* *n = length; fills min(cap, *n) */
int fhelin_level_plan_set(fhelin_ctx* c, const int32_t* target, int32_t n);
int fhelin_sync(fhelin_ctx* c);
/* Lanes: a context owns a few extra HIP streams ("lanes" 1..n, FHELIN_LANES, default 2) besides its main stream (lane 0), each with
 * its own arena of device memory.  After fhelin_ctx_set_lane(c, k) every call launches on lane k and allocates there, until the next
 * set_lane; deferred operations (fhelin_bootstrap, ...) issued under a lane are evaluated on that lane.  Independent work - the two
 * halves of a batch of samples, src/main.cpp:145-475 once per sample - issued alternately under two lanes runs CONCURRENTLY on the
 * GPU from ONE host thread and ONE context (one key set, one plaintext cache): the tail of one lane's launch is filled by the
 * other's.  lanes_fork: lanes 1..n wait for everything the main stream has been given so far (the inputs); lanes_join: the main
 * stream waits for every lane (before decrypting / exporting under lane 0).  A value must be consumed under the lane that produced it,
 * after a join, or after fhelin_ctx_lane_wait(producer's lane) under the consuming lane (a value of one branch of a circuit meeting
 * another branch's); results are bit-identical to lane 0 (scheduling only). */
int fhelin_ctx_set_lane(fhelin_ctx* c, int32_t lane);
int fhelin_ctx_lane_wait(fhelin_ctx* c, int32_t from_lane);   /* the current lane's stream waits for everything issued under from_lane so far */
/* mark: remember the present point of the current lane's stream; wait_mark: the current lane waits for from_lane's last mark (not for what
 * was issued there after it).  A scheduler that starts a new branch of a circuit on a free lane holds it back until the other lane's
 * last BULK call (a row loop that fills the GPU by itself) has drained: the new branch then runs beside the small launches that follow
 * it there, instead of beside the bulk call, where it would gain nothing. */
int fhelin_ctx_lane_mark(fhelin_ctx* c);
int fhelin_ctx_lane_wait_mark(fhelin_ctx* c, int32_t from_lane);
int fhelin_ctx_lanes_fork(fhelin_ctx* c);
int fhelin_ctx_lanes_join(fhelin_ctx* c);
/* give the device memory the context's caching pool holds but does not use back to the driver (another context / process
 * on the same GPU can then have it); synchronises first */
int fhelin_ctx_trim(fhelin_ctx* c);
/* HIP-event timer on the context's stream (bench.py measures kernel time with these) */
int fhelin_timer_start(fhelin_ctx* c);
int fhelin_timer_stop(fhelin_ctx* c, float* ms);

/* ---- raw device buffers + residue-polynomial kernels (parity tests and bench call these) ------- */
int fhelin_dev_alloc(fhelin_ctx* c, size_t bytes, void** out);
int fhelin_dev_free(fhelin_ctx* c, void* p);
int fhelin_dev_upload(fhelin_ctx* c, void* dst, const void* src, size_t bytes);
int fhelin_dev_download(fhelin_ctx* c, void* dst, const void* src, size_t bytes);

/* K1: in-place negacyclic NTT/INTT of nvec limb vectors d_data[v][N]; vector v uses limb
 * limb_first + (v % limb_count).  Stands in for DCRTPoly::SetFormat inside OpenFHE. */
int fhelin_ntt(fhelin_ctx* c, uint64_t* d_data, int32_t nvec, int32_t limb_first, int32_t limb_count, int32_t inverse);

/* host-side operation counters since the last reset: [0] limb-NTTs, [1] key switches, [2] sum of live limbs over
 * key switches, [3] rescales, [4] ct x pt products, [5] bootstraps, [6] plaintext encodes, and with cap >= 9:
 * [7] sum of live limbs over rescales, [8] sum of live limbs over ct x pt products, and with cap >= 12 the growth of the
 * device pool: [9] blocks obtained from hipMalloc, [10] their bytes, [11] host nanoseconds spent inside hipMalloc, and with
 * cap >= 16: [12] bytes the pool holds from the driver now, [13] / [14] high-water marks of bytes in use / held since the last
 * reset, [15] out-of-memory events (everything idle handed back: a device-wide synchronisation each), and with cap >= 18:
 * [16] device bytes of the encodings the plaintext cache holds (fhelin_encode), [17] bytes the pool has handed out and not got back, and with
 * cap >= 19: [18] plaintexts the cache holds */
int fhelin_stats(fhelin_ctx* c, uint64_t* out, int32_t cap, int32_t reset);
/* host-side self-test of the device memory arena (slabs, best fit, coalescing) against a pretend device of device_bytes: n_ops random
 * allocations / frees in the engine's size mix; checks that blocks never overlap, lie inside a slab, that freeing everything leaves one
 * free range per slab and that a trim returns every slab.  out (cap >= 6): [0] peak bytes in use, [1] peak bytes held, [2] slabs
 * obtained, [3] out-of-memory events, [4] coalesced-to-one-range-per-slab (1/0), [5] trim-returned-everything (1/0).  No GPU needed. */
int fhelin_debug_pool_selftest(uint64_t seed, int32_t n_ops, uint64_t device_bytes, uint64_t* out, int32_t cap);
/* FHELIN_POOL_FILL=<w>, w in 1..4095 (a test aid; unset or 0: off; any other value: fhelin_ctx_create fails with FHELIN_ERR_ARG): the
 * arena hands out every block with w in each 32-bit word of its rounded size, so that a result which depends on memory nobody wrote
 * depends on w.  _fill_stats: blocks and bytes filled so far (both 0 with the knob off).  _fill_selftest: the knob on host memory
 * (host malloc as the backend, a host fill): n_ops seeded allocations / frees over both granule classes and more than one slab; every
 * handed-out word is w, every other live block keeps its own marker, w = 0 writes nothing.  out (cap >= 6): [0] blocks handed out,
 * [1] the sum of their rounded sizes, [2] blocks filled, [3] bytes filled, [4] slabs obtained, [5] hand-outs at the 4 KiB granule. */
int fhelin_debug_pool_fill_stats(fhelin_ctx* c, uint64_t* blocks, uint64_t* bytes);
int fhelin_debug_pool_fill_selftest(uint64_t seed, int32_t n_ops, uint32_t w, uint64_t* out, int32_t cap);


/* ---- keys (client side; sampling on the host, polynomial arithmetic on the GPU) ---------------- */
int fhelin_keygen(fhelin_ctx* c);                       /* context->KeyGen()                  FHEController.cpp:47  */
int fhelin_gen_relin_key(fhelin_ctx* c);                /* context->EvalMultKeyGen(sk)        :49                   */
int fhelin_gen_rotation_keys(fhelin_ctx* c, const int32_t* indices, int32_t n);  /* EvalRotateKeyGen  :248       */
int fhelin_gen_conj_key(fhelin_ctx* c);
/* raw key material, [L+1+k][N] (secret, NTT form) and [dnum][2][L+1+k][N] (switching keys): parity tests
 * hand the same arrays to the oracle.  kind: 0 = relinearisation key, 1 = rotation key for `index`, 2 = conjugation key. */
int fhelin_secret_export(fhelin_ctx* c, uint64_t* out, size_t cap_words);
int fhelin_secret_import(fhelin_ctx* c, const uint64_t* in, size_t words);
int fhelin_key_export(fhelin_ctx* c, int32_t kind, int32_t index, uint64_t* out, size_t cap_words);
int fhelin_key_import(fhelin_ctx* c, int32_t kind, int32_t index, const uint64_t* in, size_t words);

/* ---- plaintexts: context->MakeCKKSPackedPlaintext(vec, 1, level, nullptr, slots)  :353,:368 ---- */
/* Plaintexts are cached per context BY CONTENT: a second encode of the same (n, slots, level, value bytes) gives a handle that shares the
 * first one's device encodings at exactly equal (limbs, scale) (a model's weights and masks are encoded once, not once per pass).  `vals` is copied: changing the array
 * afterwards changes nothing.  fhelin_pt_free drops the handle's reference only; the cache itself is bounded (FHELIN_PT_CACHE_MB, default
 * 1024, least recently used plaintext first) and emptied by fhelin_ctx_trim and fhelin_ctx_destroy.  FHELIN_PT_CACHE=0: no cache.
 * DOMAIN of the encoder: every value that becomes part of the plaintext (the first min(n, slots)) must be finite - a NaN or an infinity
 * is refused here with FHELIN_ERR_ARG (no device needed), no handle is made.  A plaintext is encoded when an operation first needs it at
 * some (limbs, scale); an encoding is refused there with FHELIN_ERR_ARG (fhelin_pt_export, fhelin_encrypt, every ct x pt / ct + pt
 * operation) unless floor(log2 max|vals[i]|) + floor(log2 scale) <= 123.  The test reads the two exponents only: it guarantees
 * max|vals[i]| * scale < 2^125, so everything that reaches 2^125 is refused (and some products from 2^123 on: at a Delta just below 2^52
 * values below 2^73 are accepted, at one just above 2^52 values below 2^72).  The rounding code takes integers below 2^126, and every
 * coefficient of an encoding is an average of slot values.  A refusal launches nothing and leaves the plaintext, the cache and the context as they were;
 * neither check changes a residue of an accepted input. */
int fhelin_encode(fhelin_ctx* c, const double* vals, int32_t n, int32_t level, int32_t slots, fhelin_pt** out);
void fhelin_pt_free(fhelin_pt* p);
/* the residues [ell][N] (NTT form) this plaintext multiplies / adds with at `ell` live limbs and real scaling factor
 * scale_hi + scale_lo (the library keeps scales as 80-bit long double: two doubles carry one exactly; scale_hi <= 0:
 * the context's Delta of that level) — exactly the encoding EvalMult(ct,pt) / EvalAdd(ct,pt) use for a ciphertext of that
 * shape (parity tests hand them to the oracle's dyadic functions).  ell = L + 1 + k (all limbs of the chain and the special
 * limbs; explicit scale required): the encoding over the full key basis, [L + 1 + k][N], as fhelin_hoisted_dot folds it into keys */
int fhelin_pt_export(fhelin_ctx* c, const fhelin_pt* p, int32_t ell, double scale_hi, double scale_lo, uint64_t* out,
                     size_t cap_words);

/* ---- ciphertexts ----------------------------------------------------------------------------- */
int fhelin_encrypt(fhelin_ctx* c, const fhelin_pt* p, fhelin_ct** out);                 /* context->Encrypt   :380,:384 */
/* n_vec inputs at once (the driver's 194 read_expanded_input calls per sample, src/main.cpp:159-173; FHEController.cpp:623-650):
 * vals [n_vec][n_per] real slot values -> n_vec fresh ciphertexts at `level`.  Encoding (special FFT in fp64, scaling,
 * rounding), the sampling of the encryption randomness (ChaCha20 on the GPU, keyed from the client's generator) and the
 * dyadic combination run as batched kernels.
 * The same DOMAIN as fhelin_encode: a NaN or an infinity among the values read (the first min(n_per, slots) of every vector), or
 * floor(log2 max|vals|) + floor(log2 Delta) > 123 with Delta the scale of the level a vector starts at (`level`, lower by what an
 * applied level plan takes off), fails the whole call with FHELIN_ERR_ARG and gives no handle.  The values are checked as they are
 * staged, one chunk of 32 vectors after the other: the context's generator may have advanced by the draws of the chunks before the
 * refused one.  The level plan does not move: a failed fhelin_encrypt or fhelin_encrypt_batch has made no source, and the plan's
 * source counter is where the call found it. */
int fhelin_encrypt_batch(fhelin_ctx* c, const double* vals, int32_t n_vec, int32_t n_per, int32_t level, int32_t slots, fhelin_ct** outs);
/* The client side of ONE sample on the device: what the reference does in NumPy before the server sees anything
 * (src/python/dimReduce.py:141-160: x_in = [cls; emb + pos/3], X_E = E[:, :S+1] x_in + b_E, X_F likewise) followed by the 64 + S + 1
 * read_expanded_input calls of the driver (src/main.cpp:159-173, src/FHEController.cpp:623-650) - gather / projection / packing /
 * encoding / sampling / encryption as GPU kernels, fp64 with the operation order of the NumPy statement (sequential sums, no FMA).
 * Give the S token embeddings as emb [S][128], or token ids tokens [S] into table [vocab][128].  pos [>= S][128], cls [128],
 * E_w / F_w [32][w_cols] row-major (w_cols >= S + 1), E_b / F_b [32].  outs: 64 + S + 1 handles in the order of the driver's reads:
 * the 32 E-projected rows, the 32 F-projected rows, then the S + 1 tokens (CLS first).  Every output is a source of the level plan.
 * proj_out (optional, (S + 1 + 64) * 128 doubles): x_in rows then the projected rows as the device computed them (parity tests).
 * The rows that are encoded are computed on the device: the encoder's DOMAIN (fhelin_encode) is NOT checked here - finite inputs whose
 * sums stay far below 2^125 / Delta are the caller's to give. */
int fhelin_client_ingest(fhelin_ctx* c, const double* emb, const int32_t* tokens, const double* table, int32_t vocab, int32_t S,
                         const double* cls, const double* pos, const double* E_w, const double* E_b, const double* F_w, const double* F_b,
                         int32_t w_cols, int32_t level, fhelin_ct** outs, double* proj_out);
/* 1: the special FFT of CKKS encoding runs on the host (the original encoder, the reference the device encoder is compared
 * with bit for bit); 0 (default): on the GPU.  Both produce identical residues. */
int fhelin_ctx_set_host_encode(fhelin_ctx* c, int32_t on);
/* test hook: n_poly polynomials of N centred coefficients straight from the device sampler (kind 0: rounded Gaussian
 * sigma 3.19, 1: uniform ternary) */
int fhelin_debug_sample(fhelin_ctx* c, int32_t kind, int32_t n_poly, int64_t* out, size_t cap);
int fhelin_decrypt(fhelin_ctx* c, const fhelin_ct* ct, double* out, int32_t slots);     /* context->Decrypt + GetRealPackedValue :387-404 */
int fhelin_ct_import(fhelin_ctx* c, const uint64_t* limbs, int32_t npoly, int32_t ell, int32_t deg, double scale,
                     int32_t slots, fhelin_ct** out);
int fhelin_ct_export(fhelin_ctx* c, const fhelin_ct* ct, uint64_t* out, size_t cap_words);
/* the same with DEVICE buffers (a torch / RCCL tensor): ciphertext rows exchanged between the GPUs of a node travel
 * without a host round trip.  The scale is the library's 80-bit value as hi + lo doubles. */
int fhelin_ct_export_device(fhelin_ctx* c, const fhelin_ct* ct, uint64_t* d_out, size_t cap_words);
int fhelin_ct_import_device(fhelin_ctx* c, const uint64_t* d_limbs, int32_t npoly, int32_t ell, int32_t deg, double scale_hi,
                            double scale_lo, int32_t slots, fhelin_ct** out);
int fhelin_ct_scale(const fhelin_ct* ct, double* scale_hi, double* scale_lo);
int fhelin_ct_info(const fhelin_ct* ct, int32_t* npoly, int32_t* ell, int32_t* level, int32_t* deg, double* scale,
                   int32_t* slots);                                                     /* ct->GetLevel() / GetSlots()  */
int fhelin_ct_clone(fhelin_ctx* c, const fhelin_ct* ct, fhelin_ct** out);                /* ct->Clone()  (main.cpp:223) */
void fhelin_ct_free(fhelin_ct* ct);

/* ---- leveled evaluation (FLEXIBLEAUTO bookkeeping included) ------------------------------------ */
int fhelin_add(fhelin_ctx* c, const fhelin_ct* a, const fhelin_ct* b, fhelin_ct** out);          /* EvalAdd(ct,ct)   :410 */
int fhelin_sub(fhelin_ctx* c, const fhelin_ct* a, const fhelin_ct* b, fhelin_ct** out);
int fhelin_negate(fhelin_ctx* c, const fhelin_ct* a, fhelin_ct** out);
int fhelin_add_plain(fhelin_ctx* c, const fhelin_ct* a, const fhelin_pt* p, fhelin_ct** out);    /* EvalAdd(ct,pt)   :414 */
int fhelin_mult_plain(fhelin_ctx* c, const fhelin_ct* a, const fhelin_pt* p, fhelin_ct** out);   /* EvalMult(ct,pt)  :427 */
int fhelin_mult(fhelin_ctx* c, const fhelin_ct* a, const fhelin_ct* b, fhelin_ct** out);         /* EvalMult(ct,ct)  :431 */
int fhelin_rotate(fhelin_ctx* c, const fhelin_ct* a, int32_t index, fhelin_ct** out);            /* EvalRotate       :435,:833,:843 */
/* hoisted rotations: outs[i] = EvalRotate(a, indices[i]) for all i with ONE decomposition of a (OpenFHE's
 * EvalFastRotationPrecompute + EvalFastRotation pair); the results are bit-identical to n calls of fhelin_rotate */
int fhelin_rotate_many(fhelin_ctx* c, const fhelin_ct* a, const int32_t* indices, int32_t n, fhelin_ct** outs);
/* outs[i] = EvalRotate(v[i], indices[i]): rows of identical (level, degree, scale) share one batched key switch */
int fhelin_rotate_each(fhelin_ctx* c, const fhelin_ct* const* v, const int32_t* indices, int32_t n, fhelin_ct** outs);
/* outs[i] = v[i] + sum_r EvalRotate(v[i], indices[r]) (1 <= n_rot <= 7) with one decomposition and ONE ModDown per
 * row: the rotated terms are accumulated in the extended basis QP.  Two steps of the reference's rotsum loop (:829-837),
 * x += rot(x, s); x += rot(x, 2s), are the call {s, 2s, 3s}.  Needs the rotation keys of all indices. */
int fhelin_rotate_sum(fhelin_ctx* c, const fhelin_ct* const* v, int32_t n, const int32_t* indices, int32_t n_rot, fhelin_ct** outs);
/* outs[i] = v[i] * pts[0] + sum_r EvalRotate(v[i], indices[r]) * pts[r + 1] (1 <= n_rot <= 7; pts: n_rot + 1 plaintexts) with one
 * decomposition and ONE ModDown per row ("double hoisting"): the plaintext products are taken in the extended basis QP, through
 * rotation keys with the plaintext folded in (built once per (plaintext, index, scale) and cached: one full key copy each - meant
 * for few plaintexts shared by many rows).  The first step of matmulRElarge (src/FHEController.cpp:915-944 re-associated, DESIGN.md
 * §7) is the call {128, 256, 384} over all rows.  Result: noise degree + 1, scale x the level's plaintext scale.  The plaintext
 * encodings over the full key basis are fhelin_pt_export(p, L + 1 + k, scale).
 * rescale != 0: the result rescaled, with ModDown and rescale as ONE basis conversion (P and the top limb dropped together: one rounding
 * instead of two, 2 ell fewer transforms per row): one limb fewer, the input's noise degree, scale / q_top.  That conversion takes at
 * most 16 sources: with k = 16 the ModDown and the rescale run one after the other (two roundings). */
int fhelin_hoisted_dot(fhelin_ctx* c, const fhelin_ct* const* v, int32_t n, const fhelin_pt* const* pts, const int32_t* indices,
                       int32_t n_rot, int32_t rescale, fhelin_ct** outs);
/* out = sum_i EvalRotate(v[i], indices[i]) (index 0 = plain addend): the giant steps of EvalBootstrap's linear
 * transforms (:445) — one ModUp per term, inner products accumulated in QP, ONE ModDown per group of <= 7 terms */
int fhelin_rotate_each_sum(fhelin_ctx* c, const fhelin_ct* const* v, const int32_t* indices, int32_t n, fhelin_ct** out);
int fhelin_rescale(fhelin_ctx* c, const fhelin_ct* a, fhelin_ct** out);                          /* ModReduce (implicit in :427/:431) */
/* the leaf operations over n independent ciphertexts (the rows of the reference's matmul loops, :872,:888,:904,:918,
 * :949,:963,:985,:1001) in one call: same results as n single calls, one launch set per chunk of rows of equal shape */
int fhelin_rotate_batch(fhelin_ctx* c, const fhelin_ct* const* v, int32_t n, int32_t index, fhelin_ct** outs);
int fhelin_rescale_batch(fhelin_ctx* c, const fhelin_ct* const* v, int32_t n, fhelin_ct** outs);
int fhelin_mult_plain_batch(fhelin_ctx* c, const fhelin_ct* const* v, int32_t n, const fhelin_pt* p, fhelin_ct** outs);
int fhelin_mult_batch(fhelin_ctx* c, const fhelin_ct* const* a, const fhelin_ct* const* b, int32_t n, fhelin_ct** outs);
int fhelin_add_batch(fhelin_ctx* c, const fhelin_ct* const* a, const fhelin_ct* const* b, int32_t n, fhelin_ct** outs);
/* outs[i] = Rescale(f[i] * EvalMult(a[i], b[i]) + cadd[i] +- addend[i]): relinearised products that are rescaled right away (the power
 * steps T_2k = 2 T_k^2 - 1, T_(j+k) = 2 T_j T_k - T_(j-k) of a Chebyshev evaluation), all through ONE batched key switch.  f[i] is 1 or 2;
 * addend may be null, and so may each addend[i]; negate[i] != 0 subtracts the addend.  The residues are those of fhelin_mult_batch,
 * fhelin_add_batch, fhelin_add_real / fhelin_add_batch, rescale - bit for bit; FHELIN_EXACT_PRODUCTS=0 runs that sequence itself. */
int fhelin_mult_affine_batch(fhelin_ctx* c, const fhelin_ct* const* a, const fhelin_ct* const* b, int32_t n, const int32_t* f, const double* cadd,
                             const fhelin_ct* const* addend, const int32_t* negate, fhelin_ct** outs);
int fhelin_level_reduce(fhelin_ctx* c, const fhelin_ct* a, int32_t new_ell, fhelin_ct** out);

/* ---- Linear transforms: matrix x ciphertext by the diagonal method, baby-step/giant-step (OpenFHE EvalLinearTransform, Lattigo
 * LinearTransform).  out = sum_d diag_d (.) rot(x, d), rot = EvalRotate (left rotation): M x for the matrix whose generalised diagonals are
 * diag_d.  Every index splits as d = g + b with 0 <= b < n1; the term's plaintext is V_{g,b} = rot(diag_{g+b}, -g) and
 *     inner_g = x V_{g,0} + sum_{b>0} rot(x, b) V_{g,b},        out = sum_g rot(inner_g, g)      (g = 0: a plain addend).
 * The baby steps share ONE decomposition of x and their key products are formed once, in the extended basis QP, for all groups: no
 * rotated ciphertext and no plaintext-folded key is ever stored, and a call costs one ModDown per group plus one per <= 7 rotated groups.
 *
 * A plan (fhelin_lt) is host data: the split, the two index lists and one plaintext per term.  Creating one needs no device; the
 * encodings are made on first use per (limb count, scale) and stay with the plan's plaintexts.  An encoding is LIMB-SLICED: a term
 * applied at ell limbs holds the rows the inner product reads - Q limbs 0..ell-1, then the k special limbs, (ell + k) N words - with the
 * residues of the encoding over the full key basis on those rows.  fhelin_lt_encoding_bytes: the device bytes the plan's plaintexts hold
 * that way, sum over (term, distinct (ell, scale) applied at) of (ell + k) N 8.
 *
 * fhelin_lt_create: diags [n_diag][slots], diag_idx [n_diag] (reduced mod slots; duplicates, n_diag < 1, a slots that is not the
 * context's packing, n1 outside 0..32 and non-finite values are FHELIN_ERR_ARG); n1 = 0 lets the planner choose n1 <= 32.  It builds
 * the V_{g,b} and calls fhelin_lt_create_pts, the one constructor: pts [n2][n1] (NULL = term absent), baby [n1] with baby[0] == 0,
 * giant [n2], indices distinct mod slots.  The plan shares the plaintexts: the caller's handles may be freed afterwards.
 * fhelin_lt_rotations: the EvalRotateKeyGen list the plan needs (baby steps that carry a term, rotated giant steps); *n = its length,
 * min(cap, *n) entries written.
 *
 * fhelin_lt_apply: outs[i] = the transform of v[i]; rows of one shape share every launch.  Bit for bit - limbs, noise degree, scale -
 *     fhelin_rotate_each_sum([ fhelin_hoisted_dot(v[i], {V_{g,0..n1-1}}, baby[1..], rescale = 0) for g ], giant)
 * as oracle/residue_eval.py states the two (hoisted_dot reaches only 7 rotations through this ABI; the oracle takes any number): a
 * degree-2 input is rescaled first, the result has noise degree + 1 and scale x the level's plaintext scale; an absent term contributes
 * what a plaintext of zeros would.  rescale != 0: the final sum goes through fhelin_rescale.
 * Errors: a missing rotation key FHELIN_ERR_KEY naming the index; an interleave stride other than 1 FHELIN_ERR_STATE; no device
 * FHELIN_ERR_NO_DEVICE.  A failed call launches nothing that outlives it, returns no handle and leaves the level plan as it was.
 * Works on an evaluation context (fhelin_evalkeys_load). */
typedef struct fhelin_lt fhelin_lt;
int fhelin_lt_create(fhelin_ctx* c, const double* diags /* [n_diag][slots] */, const int32_t* diag_idx, int32_t n_diag, int32_t slots,
                     int32_t n1 /* 0 = choose */, fhelin_lt** out);
int fhelin_lt_create_pts(fhelin_ctx* c, const fhelin_pt* const* pts /* [n2][n1], NULL = absent */, const int32_t* baby /* [n1], baby[0] == 0 */,
                         const int32_t* giant /* [n2] */, int32_t n1, int32_t n2, fhelin_lt** out);
int fhelin_lt_info(const fhelin_lt* lt, int32_t* n1, int32_t* n2, int32_t* n_terms, int32_t* slots);
int fhelin_lt_rotations(const fhelin_lt* lt, int32_t* out, int32_t cap, int32_t* n);
int fhelin_lt_apply(fhelin_ctx* c, const fhelin_lt* lt, const fhelin_ct* const* v, int32_t n, int32_t rescale, fhelin_ct** outs);
int fhelin_lt_encoding_bytes(const fhelin_lt* lt, uint64_t* bytes);
void fhelin_lt_free(fhelin_lt* lt);

/* ---- the same residue functions without scale/level bookkeeping (bit-exact parity vs oracle/) -- */
int fhelin_raw_rescale(fhelin_ctx* c, const fhelin_ct* a, fhelin_ct** out);                      /* K5            */
int fhelin_raw_rotate(fhelin_ctx* c, const fhelin_ct* a, int32_t index, fhelin_ct** out);        /* K4 + K6-K8    */
int fhelin_raw_mult_relin(fhelin_ctx* c, const fhelin_ct* a, const fhelin_ct* b, fhelin_ct** out);/* K2 + K6-K8   */
/* K9 ModRaise, first step of EvalBootstrap (:445): a ciphertext with ONE limb -> new_ell limbs (centred lift) */
int fhelin_raw_modraise(fhelin_ctx* c, const fhelin_ct* a, int32_t new_ell, fhelin_ct** out);
/* the decryption phase c0 + c1 s (+ c2 s^2) on every live limb, as a 1-component handle (context->Decrypt :389 before
 * decoding; client side: needs the secret key) */
int fhelin_raw_phase(fhelin_ctx* c, const fhelin_ct* a, fhelin_ct** out);

/* ---- test hooks: the ciphertext x plaintext inner-sum kernels on operands chosen residue by residue --------
 * No driver calls these.  Ciphertexts arrive through fhelin_ct_import (degree 1, two components, one limb count and scale per call),
 * plaintexts through fhelin_debug_pt_from_residues, results leave through fhelin_ct_export (noise degree 2).
 *
 * A plaintext whose ONLY encoding is `residues` [ell][N] (NTT form, every word below its limb's modulus, else FHELIN_ERR_ARG) at ell limbs
 * and the scale the inner sums ask for at that limb count (Delta of level n_q - ell).  It has no slot values: used at any other (limb
 * count, scale) it fails with FHELIN_ERR_STATE.  It never enters the content-keyed plaintext cache of fhelin_encode. */
int fhelin_debug_pt_from_residues(fhelin_ctx* c, const uint64_t* residues, int32_t ell, fhelin_pt** out);
/* the same over the FULL key basis: residues [n_q + n_p][N] (Q limbs, then the special limbs) at the scale scale_hi + scale_lo - what
 * fhelin_hoisted_dot and fhelin_lt_apply ask a plaintext for (the level's Delta, exactly) */
int fhelin_debug_pt_from_residues_full(fhelin_ctx* c, const uint64_t* residues, double scale_hi, double scale_lo, fhelin_pt** out);
/* out = sum_i cts[i] * pts[i]: one launch per 32 terms */
int fhelin_debug_dot_plain(fhelin_ctx* c, const fhelin_ct* const* cts, const fhelin_pt* const* pts, int32_t n, fhelin_ct** out);
/* outs[x][g] = sum_b cts[x][b] * pts[g][b] for x < nb, g < ng (na <= 16 columns, ng <= 8 groups; pts[g][b] NULL = term absent) in ONE
 * launch.  nb >= 2: the same plaintexts over nb sets of ciphertexts, which are first copied into equally spaced views of one block.
 * Operands the kernel does not take are an error (FHELIN_ERR_STATE), never another path. */
int fhelin_debug_dot_groups(fhelin_ctx* c, const fhelin_ct* const* cts /* [nb][na] */, int32_t nb, int32_t na,
                            const fhelin_pt* const* pts /* [ng][na] */, int32_t ng, fhelin_ct** outs /* [nb][ng] */);
/* outs[k] = sum_{i<n} cts[i] * pts[(i + k) mod 32] for k < 32, n <= 32 */
int fhelin_debug_dot_cyclic(fhelin_ctx* c, const fhelin_ct* const* cts, int32_t n, const fhelin_pt* const* pts /* [32] */,
                            fhelin_ct** outs /* [32] */);
/* dest[t] (+)= sum_{j<32} (j <= t ? cur[j] : prev[j]) * pts[(t - j) mod 32] for t < 32; cur[j], prev[j] NULL = zero (at least one entry
 * present).  dest is in/out: 32 imported ciphertexts of the operands' shape, overwritten - accumulate != 0: added to. */
int fhelin_debug_dot_window(fhelin_ctx* c, const fhelin_ct* const* cur /* [32] */, const fhelin_ct* const* prev /* [32] */,
                            const fhelin_pt* const* pts /* [32] */, fhelin_ct* const* dest /* [32] */, int32_t accumulate);
/* outs[i][k] = rot(cts[i], indices[k]) for i < n_ct, k < n: the hoisted rotations of MANY inputs behind one ModUp
 * (Evaluator::rotate_many_batch, which the composites and bootstrapping call), bit-identical to fhelin_rotate.  Two or more inputs of one
 * shape and more than 16 non-zero indices take its per-input, per-16-row chunks. */
int fhelin_debug_rotate_many_batch(fhelin_ctx* c, const fhelin_ct* const* cts, int32_t n_ct, const int32_t* indices, int32_t n,
                                   fhelin_ct** outs /* [n_ct][n] */);
/* The special-limb half of a key switch's inner product over digits chosen residue by residue (any value below 2^60), followed by its
 * inverse transform, through the evaluator's own stages (FHELIN_FUSE_ACCP_ROWS decides which launches run):
 *   n_rot = 0: out[b][c][p] = INTT( sum_j digits[b][j][ell+p] * relin[j][c][p] * 2^-64 )   (the identity form: digits come times 2^64)
 *   n_rot > 0: out[b][c][p] = INTT( sum_r sigma_r( sum_j digits[b][j][ell+p] * key_r[j][c][p] ) ),  r over the n_rot <= 7 indices
 * digits [batch][beta(ell)][ell + n_p][N]; the own-digit slots of the Q limbs count as zero and the Q half is dropped. */
int fhelin_debug_ks_accp(fhelin_ctx* c, const uint64_t* digits, int32_t ell, int32_t batch, const int32_t* indices, int32_t n_rot,
                         uint64_t* out /* [batch][2][n_p][N] */);
/* The Q-limb half of a single-key inner product and the row-pass finish of its ModDown over operands chosen residue by residue, through
 * the evaluator's own stages (FHELIN_FUSE_ACCQ_ROWS decides which launches run):  out[b][c][t] = (acc[b][c][t] - NTT(conv[b][c][t])) * P^-1,
 *   index = 0: acc[b][c][t] = sum_{j != t / alpha} digits[b][j][t] * relin[j][c][t] * 2^-64 + own[b][t] * relin[t / alpha][c][t]
 *   index != 0: acc[b][c][t] = sigma_g( sum_{j != t / alpha} digits[b][j][t] * key[j][c][t] + own[b][t] * key[t / alpha][c][t] ),  g of that rotation
 * digits [batch][beta(ell)][ell + n_p][N] below 2^60 (the own-digit slots are not read); own [batch][ell][N] and conv [batch][2][ell][N]
 * (coefficient form) canonical. */
int fhelin_debug_ks_accq(fhelin_ctx* c, const uint64_t* digits, const uint64_t* own, const uint64_t* conv, int32_t ell, int32_t batch,
                         int32_t index, uint64_t* out /* [batch][2][ell][N] */);
/* The two kernels of a paired bootstrap on their own, over n <= 32 pairs of (imported) ciphertexts in ONE launch each; they need no key
 * and no bootstrap set-up.
 *   pack:  outs[i] = (k0_a[i] a[i] + X^(N/2) k0_b[i] b[i]) mod q_l on the two bottom limbs l < 2 of both components; a[i], b[i] with two
 *          components and any limb count >= 2 (FHELIN_ERR_STATE otherwise), read in place; k0 any 64-bit integers, reduced per limb.
 *          outs[i]: 2 limbs, a[i]'s degree + 1, scale a[i]'s x k0_a[i].
 *   split: out_a[i] = w[i] + wc[i], out_b[i] = X^(N/2) (wc[i] - w[i]) mod q_l over all limbs; all operands of one shape (FHELIN_ERR_STATE
 *          otherwise); degree, scale and slots of w[i]. */
int fhelin_debug_pair_pack(fhelin_ctx* c, const fhelin_ct* const* a, const fhelin_ct* const* b, const uint64_t* k0_a, const uint64_t* k0_b,
                           int32_t n, fhelin_ct** outs);
int fhelin_debug_pair_split(fhelin_ctx* c, const fhelin_ct* const* w, const fhelin_ct* const* wc, int32_t n, fhelin_ct** out_a,
                            fhelin_ct** out_b);

/* ---- FHEController composite circuit ops (callers of the hot path) --------
 * One entry point per reference method; `vector<Ctxt>` travels as (array of handles, count); outputs are
 * written to caller-provided handle arrays.  A NULL bias means `bias == nullptr` in the reference. */
int fhelin_fc_mult_const(fhelin_ctx* c, const fhelin_ct* a, double d, fhelin_ct** out);                 /* mult(ct,double) :421 */
/* kind 0 mask_block(from=a,to=b,v) :1207 | 1 mask_heads(v) :1221 | 2 mask_heads_128(v) :1235 |
 *      3 mask_mod_n(n=a,padding=b) :1249,:1262 | 4 mask_first_n(n=a,v) :1275 */
int fhelin_fc_mask(fhelin_ctx* c, const fhelin_ct* a, int32_t kind, int32_t x, int32_t y, double v, fhelin_ct** out);
int fhelin_fc_rotsum(fhelin_ctx* c, const fhelin_ct* a, int32_t slots, int32_t padding, fhelin_ct** out);  /* rotsum :829, rotsum_padded :839 */
int fhelin_fc_repeat(fhelin_ctx* c, const fhelin_ct* a, int32_t slots, int32_t padding, fhelin_ct** out);  /* repeat :849,:859 */
int fhelin_fc_add_many(fhelin_ctx* c, const fhelin_ct* const* v, int32_t n, fhelin_ct** out);            /* add(vector) :417 */
/* matmulRE :869,:885 (slots=row_size, padding) and matmulCR :982 (slots=128, padding=1), plaintext weight */
int fhelin_fc_matmul_pt(fhelin_ctx* c, const fhelin_ct* const* rows, int32_t n, const fhelin_pt* w, const fhelin_pt* bias,
                        int32_t slots, int32_t padding, fhelin_ct** outs);
/* matmulRE(ct weight) :901, matmulCR(ct) :946 (64,1), matmulCR_128 :960,:974 (128,1) */
int fhelin_fc_matmul_ct(fhelin_ctx* c, const fhelin_ct* const* rows, int32_t n, const fhelin_ct* w, int32_t slots,
                        int32_t padding, fhelin_ct** outs);
int fhelin_fc_matmulRElarge(fhelin_ctx* c, const fhelin_ct* const* rows, int32_t n, const fhelin_pt* const* weights,
                            int32_t nw, const fhelin_pt* bias, double mask_val, fhelin_ct** outs);      /* :915 */
/* rows: n x 4 handles, row-major */
int fhelin_fc_matmulCRlarge(fhelin_ctx* c, const fhelin_ct* const* rows, int32_t n, const fhelin_pt* const* weights,
                            const fhelin_pt* bias, fhelin_ct** outs);                                   /* :998 */
int fhelin_fc_matmulScores(fhelin_ctx* c, const fhelin_ct* const* queries, int32_t n, const fhelin_ct* key, fhelin_ct** out); /* :1028,:1050 */
int fhelin_fc_wrapUpRepeated(fhelin_ctx* c, const fhelin_ct* const* v, int32_t n, fhelin_ct** out);       /* :1060 */
int fhelin_fc_wrapUpExpanded(fhelin_ctx* c, const fhelin_ct* const* v, int32_t n, fhelin_ct** out);       /* :1070 */
int fhelin_fc_unwrapExpanded(fhelin_ctx* c, const fhelin_ct* a, int32_t inputs_num, fhelin_ct** outs);    /* :1086 */
int fhelin_fc_unwrapScoresExpanded(fhelin_ctx* c, const fhelin_ct* a, int32_t inputs_num, fhelin_ct** outs); /* :1125 */
int fhelin_fc_unwrap_512_in_4_128(fhelin_ctx* c, const fhelin_ct* a, int32_t index, fhelin_ct** outs4);   /* :1142 */
/* outs: input_number x 4 handles, row-major */
int fhelin_fc_unwrapRepeatedLarge(fhelin_ctx* c, const fhelin_ct* const* containers, int32_t nc, int32_t input_number,
                                  fhelin_ct** outs);                                                    /* :1102 */
/* the tokens [first, first + count) only (rows partitioned over the GPUs of a node): outs = count x 4 handles */
int fhelin_fc_unwrapRepeatedLarge_range(fhelin_ctx* c, const fhelin_ct* const* containers, int32_t nc, int32_t input_number,
                                        int32_t first, int32_t count, fhelin_ct** outs);
/* outs must hold ceil(n/32) handles; *n_out receives the count */
int fhelin_fc_generate_containers(fhelin_ctx* c, const fhelin_ct* const* inputs, int32_t n, const fhelin_pt* bias,
                                  fhelin_ct** outs, int32_t* n_out);                                    /* :1164 */
int fhelin_fc_wrap_containers(fhelin_ctx* c, const fhelin_ct* const* v, int32_t n, int32_t inputs_number, fhelin_ct** out); /* :1193 */

/* ---- the same FHEController calls on a BATCH OF B SAMPLES through one context (BASELINE config 4's per-GPU unit: "the batch of
 * independent input ciphertexts"; a sample is one run of the driver, src/main.cpp:145-475, and samples never meet).  Arrays are
 * sample-major: v[x * n + i] = row i of sample x; all samples of a call have one row count.  Sample x's outputs hold EXACTLY the
 * residues the single-sample entry point gives on sample x's inputs - rows of a batched key switch are independent - but the small
 * launches of one pass (a single query row, a container tail, one wrapped ciphertext: single-digit row counts that cannot fill 256
 * CUs) now carry the rows of every sample: one key set, one plaintext cache, one launch set.  The row loops proper
 * (fhelin_fc_matmul_pt, _matmulRElarge, _matmulCRlarge, fhelin_*_batch, fhelin_bootstrap_batch, fhelin_eval_chebyshev_batch) take the
 * samples' rows concatenated as they are; deferred rows of several samples that are read by ONE call are evaluated together. */
int fhelin_fcb_matmulScores(fhelin_ctx* c, const fhelin_ct* const* queries, int32_t n, const fhelin_ct* const* keys, int32_t B,
                            fhelin_ct** outs);                                                        /* :1028,:1050; outs[B] */
/* matmulRE / matmulCR with a ciphertext weight PER ROW (sample x's rows against sample x's wrapped keys / values, :901,:946,:960) */
int fhelin_fcb_matmul_ct(fhelin_ctx* c, const fhelin_ct* const* rows, const fhelin_ct* const* ws, int32_t n, int32_t slots, int32_t padding,
                         fhelin_ct** outs);
int fhelin_fcb_wrapUpRepeated(fhelin_ctx* c, const fhelin_ct* const* v, int32_t n, int32_t B, fhelin_ct** outs);       /* :1060; outs[B] */
int fhelin_fcb_wrapUpExpanded(fhelin_ctx* c, const fhelin_ct* const* v, int32_t n, int32_t B, fhelin_ct** outs);       /* :1070; outs[B] */
int fhelin_fcb_unwrapExpanded(fhelin_ctx* c, const fhelin_ct* const* cs, int32_t B, int32_t inputs_num, fhelin_ct** outs); /* :1086; outs[B * inputs_num] */
int fhelin_fcb_unwrapRepeatedLarge(fhelin_ctx* c, const fhelin_ct* const* containers, int32_t nc, int32_t B, int32_t input_number,
                                   fhelin_ct** outs);                                                 /* :1102; outs[B * input_number * 4] */
/* outs: B x ceil(n/32) handles; *n_out = containers per sample */
int fhelin_fcb_generate_containers(fhelin_ctx* c, const fhelin_ct* const* inputs, int32_t n, int32_t B, const fhelin_pt* bias,
                                   fhelin_ct** outs, int32_t* n_out);                                 /* :1164 */
/* rotsum (:829) / repeat (:849, repeat != 0) over n independent ciphertexts: one batched key switch per tree step */
int fhelin_fc_rotsum_batch(fhelin_ctx* c, const fhelin_ct* const* v, int32_t n, int32_t slots, int32_t padding, int32_t repeat, fhelin_ct** outs);
int fhelin_add_plain_batch(fhelin_ctx* c, const fhelin_ct* const* v, int32_t n, const fhelin_pt* p, fhelin_ct** outs);  /* EvalAdd(ct,pt) per row */
/* EvalPoly (:1291) on n ciphertexts, EvalMultMany (:1297) on B operand lists of n handles: one batched relinearisation per round */
int fhelin_eval_poly_batch(fhelin_ctx* c, const fhelin_ct* const* xs, int32_t n, const double* coeffs, int32_t n_coeffs, fhelin_ct** outs);
int fhelin_mult_many_batch(fhelin_ctx* c, const fhelin_ct* const* v, int32_t n, int32_t B, fhelin_ct** outs);

/* ---- polynomial evaluation (ADVANCEDSHE) -------------------------------------------------------- */
int fhelin_mult_real(fhelin_ctx* c, const fhelin_ct* a, double k, fhelin_ct** out);              /* EvalMult(ct, double)            */
int fhelin_add_real(fhelin_ctx* c, const fhelin_ct* a, double k, fhelin_ct** out);               /* EvalAdd(ct, double)             */
int fhelin_mult_many(fhelin_ctx* c, const fhelin_ct* const* v, int32_t n, fhelin_ct** out);      /* EvalMultMany       :1297        */
/* sum_k coeffs[k] * v[k] + c0 (OpenFHE's EvalLinearWSum, the inner sums of EvalPoly / EvalChebyshevSeries :1291,:1319-1335):
 * ciphertexts of one (level, degree 1, scale) are combined in a single kernel pass; same residues as the chain of
 * EvalMult(ct,double) / EvalAdd / EvalAdd(ct,double) */
int fhelin_lincomb(fhelin_ctx* c, const fhelin_ct* const* v, const double* coeffs, int32_t n, double c0, fhelin_ct** out);
/* power-basis polynomial sum_i coeffs[i] x^i                                                      EvalPoly           :1291        */
int fhelin_eval_poly(fhelin_ctx* c, const fhelin_ct* x, const double* coeffs, int32_t n, fhelin_ct** out);
/* Chebyshev series coeffs[0]/2 + sum_{k>=1} coeffs[k] T_k(u), u = (2x-(a+b))/(b-a)     EvalChebyshevFunction :1319-1335
 * (the shim computes the coefficients from the C++ lambda exactly like EvalChebyshevCoefficients) */
int fhelin_eval_chebyshev(fhelin_ctx* c, const fhelin_ct* x, const double* coeffs, int32_t n, double a, double b, fhelin_ct** out);
/* the same series on n ciphertexts at once (EvalChebyshevFunction in a driver's loop over independent ciphertexts,
 * src/main.cpp:354-358): every multiplication round is ONE batched relinearisation over all of them; residues identical to n calls */
int fhelin_eval_chebyshev_batch(fhelin_ctx* c, const fhelin_ct* const* xs, int32_t n, const double* coeffs, int32_t n_coeffs, double a,
                                double b, fhelin_ct** outs);
/* CKKS bootstrapping: EvalBootstrapSetup/KeyGen :238-239 and EvalBootstrap :445 */
int fhelin_bootstrap_setup(fhelin_ctx* c, int32_t level_budget_enc, int32_t level_budget_dec, int32_t slots);
int fhelin_bootstrap(fhelin_ctx* c, const fhelin_ct* a, fhelin_ct** out);
/* EvalBootstrap on n independent ciphertexts (the reference's loop over the GELU containers, src/main.cpp:354-358; the two
 * halves of affine-1, :313-314): every launch of the pipeline carries all of them.  outs[i] holds exactly the residues of
 * fhelin_bootstrap(v[i]).  fhelin_bootstrap / fhelin_eval_chebyshev calls issued back to back on independent ciphertexts are
 * batched the same way by themselves: their results are evaluated when first read (FHELIN_LAZY_HEAVY=0: at the call). */
int fhelin_bootstrap_batch(fhelin_ctx* c, const fhelin_ct* const* v, int32_t n, fhelin_ct** outs);
/* approximation parameters (before setup): |I| bound K, double-angle count R, cosine-fit degree, message correction 2^-c */
int fhelin_bootstrap_config(fhelin_ctx* c, int32_t K, int32_t R, int32_t cheb_degree, int32_t correction);
/* test hook: stop after 1 = ModRaise(+SubSum), 2 = CoeffsToSlots (real part), 3 = approximate mod (real part) */
int fhelin_bootstrap_partial(fhelin_ctx* c, const fhelin_ct* a, int32_t stage, fhelin_ct** out);
/* fhelin_bootstrap raising to L+1-drop limbs only: what a level plan (fhelin_level_plan_*) asks of the k-th bootstrap of a
 * recorded program, here with the number given by the caller */
int fhelin_bootstrap_drop(fhelin_ctx* c, const fhelin_ct* a, int32_t drop, fhelin_ct** out);
/* Iterative (two-pass) bootstrapping, the reference's EvalBootstrap(c, 2, precision) (src/FHEController.cpp:454-469): a second
 * bootstrap of 2^p (y - x) removes most of the first one's error y - x, so the result keeps about twice the bits of one bootstrap.
 * The engine's definition, residue-exact: y = BTS(x); e = 2^p (y - x) at x's two limbs and exact scale; z = BTS(e);
 * out = rescale(k (2^p y - z)), k = round(Delta_next q_top / (2^p s_y)).  The result has one limb fewer than a single bootstrap's.
 * precision p: 1 <= p <= 30, else FHELIN_ERR_ARG (checked before any device work).  2^p |y - x| must stay inside the bootstrap's
 * input range: useful values are at or below the precision of ONE bootstrap (about 14 bits at the headline ring); larger ones
 * make the second bootstrap fail silently.  Two iterations only, as the reference.  Deferred and batched like fhelin_bootstrap
 * (calls with equal precision and planned drop share a batch); each call is a source of the level plan of its own. */
int fhelin_bootstrap_iter(fhelin_ctx* c, const fhelin_ct* a, int32_t precision, fhelin_ct** out);
/* fhelin_bootstrap_iter on n independent ciphertexts, both bootstraps batched over all of them; outs[i] holds exactly the residues
 * of fhelin_bootstrap_iter(v[i], precision) */
int fhelin_bootstrap_iter_batch(fhelin_ctx* c, const fhelin_ct* const* v, int32_t n, int32_t precision, fhelin_ct** outs);
/* test hook: fhelin_bootstrap_iter with both bootstraps raising to L+1-drop limbs (fhelin_bootstrap_drop); a drop that leaves a
 * single bootstrap fewer than 3 limbs is FHELIN_ERR_STATE */
int fhelin_bootstrap_iter_drop(fhelin_ctx* c, const fhelin_ct* a, int32_t precision, int32_t drop, fhelin_ct** out);
/* Paired bootstrapping: two ciphertexts whose slot values are REAL are refreshed by ONE bootstrap, as a + i b, and taken
 * apart by one conjugation at the output level.  The engine's definition, residue-exact (corr = the correction of fhelin_bootstrap_config,
 * target = q_0 / 2^corr): for x in {a, b} (rescaled first if degree 2, two components, >= 2 limbs, equal slot counts) k0_x =
 * round(target q_1 / scale_x) and rho_x = (scale_x k0_x / q_1) 2^corr / q_0, exactly as fhelin_bootstrap computes them for x alone;
 * p = rescale(k0_a a + i k0_b b) on the two bottom limbs; the pipeline of fhelin_bootstrap from ModRaise on; v = 2^(corr-1) v (half of
 * the single bootstrap's exact 2^corr: the slots hold (a + i b) / 2 and no level is spent on the 1/2), rescaled if degree 2;
 * out_a = v + conj(v) at scale scale_v rho_a, out_b = i (conj(v) - v) at scale scale_v rho_b.  Both have the limbs, degree and nominal
 * scale of fhelin_bootstrap(a) / fhelin_bootstrap(b).  The inputs' imaginary parts must be zero (every ciphertext the drivers make): an
 * imaginary part of b would land in out_a.  No new key: the conjugation key of fhelin_bootstrap_setup (stored in evaluation-key sets).
 * Errors: as fhelin_bootstrap, plus unequal slot counts FHELIN_ERR_ARG and correction 0 FHELIN_ERR_STATE.  The `bootstrap` counter of
 * fhelin_stats advances by one per pipeline.  Each output is a source of the level plan of its own (a first); the pipeline raises to
 * the limbs the larger of the two planned targets asks for. */
int fhelin_bootstrap_pair(fhelin_ctx* c, const fhelin_ct* a, const fhelin_ct* b, fhelin_ct** out_a, fhelin_ct** out_b);
/* n ciphertexts through ONE batched pipeline of ceil(n / 2) bootstraps: consecutive inputs are paired, (0,1), (2,3), ...; an odd last
 * input, and both inputs of a pair whose slot counts differ, travel in the same pipeline as singles and come out with exactly the
 * residues of fhelin_bootstrap.  Level plan as in fhelin_bootstrap_batch: every output is a source of its own in call order; inputs with
 * different planned drops are grouped by drop first and paired inside their group. */
int fhelin_bootstrap_paired_batch(fhelin_ctx* c, const fhelin_ct* const* v, int32_t n, fhelin_ct** outs);
/* test hooks: fhelin_bootstrap_pair raising to L+1-drop limbs only; and the pair's pipeline stopped after stage 1 (pack + ModRaise +
 * SubSum), 2 (CoeffsToSlots + conjugation, real part) or 3 (approximate mod), as fhelin_bootstrap_partial */
int fhelin_bootstrap_pair_drop(fhelin_ctx* c, const fhelin_ct* a, const fhelin_ct* b, int32_t drop, fhelin_ct** out_a, fhelin_ct** out_b);
int fhelin_bootstrap_pair_partial(fhelin_ctx* c, const fhelin_ct* a, const fhelin_ct* b, int32_t stage, fhelin_ct** out);
/* Runtime knob, off by default (FHELIN_BOOT_PAIRS=1 turns it on at context creation): deferred fhelin_bootstrap calls (not the iterative
 * ones) of one lane and one planned drop that are ready together are evaluated through the paired pipeline, in call order, as
 * fhelin_bootstrap_paired_batch would.  The results are bootstraps of the same values with different residues; off, nothing changes. */
int fhelin_ctx_set_bootstrap_pairing(fhelin_ctx* c, int32_t on);
int fhelin_ctx_bootstrap_pairing(fhelin_ctx* c, int32_t* on);
/* ---- Bootstrap linear stages on the linear-transform engine (runtime knob, OFF by default; FHELIN_BOOT_LT=1 and FHELIN_BOOT_LT_N1=k are
 * read at context creation).  On: every CoeffsToSlots / SlotsToCoeffs stage is split as a linear transform above - d = g + b with at most
 * 32 baby steps, all indices multiples of the stage's stride, V_{g,b} = rot(diag_{g+b}, -g) - and applied as ONE fhelin_lt_apply-shaped
 * call over all ciphertexts of the batch (single, batched, dropped, level-planned, paired and iterative bootstraps alike): one ModUp per
 * stage, the baby steps' key products formed once in QP, n2 + ceil(R / 7) pair-ModDowns.  Bit for bit the composition stated for
 * fhelin_lt_apply, with the diagonals at sf[level + 1] q_{ell-1} / scale where a stage's input is not at its level's own scale (the first
 * stage after a ModRaise to fewer limbs).  The plaintext products are taken in QP before the ModDown, so the residues (not the values)
 * differ from the default path's.  n1 = 0: the linear-transform planner's cost, 4 (n2 + ceil(R / 7)) + baby keys, chooses per stage;
 * 1 <= n1 <= 32 forces the baby-step count (capped by the number of indices a stage can hold); anything else is FHELIN_ERR_ARG.
 * The knob chooses the split, and with it the diagonals' pre-rotation and the rotation-key list: it binds at fhelin_bootstrap_setup and
 * changing it afterwards is FHELIN_ERR_STATE.  An evaluation-key set holds the keys of the setting its client had; loading it under the
 * other setting names the missing key at fhelin_bootstrap_setup (FHELIN_ERR_KEY).  Off: describe, key list and every residue are unchanged. */
int fhelin_ctx_set_bootstrap_lt(fhelin_ctx* c, int32_t on, int32_t n1);
int fhelin_ctx_bootstrap_lt(const fhelin_ctx* c, int32_t* on, int32_t* n1);
/* ---- Sparse-secret bootstrapping (runtime knob, OFF by default = 0; FHELIN_BOOT_SPARSE_H=h is read at context creation).  Sparse-secret
 * encapsulation (Bossuat, Troncoso-Pastoriza, Hubaux 2022): the ciphertext is key-switched to a much sparser EPHEMERAL secret s~ only
 * around the ModRaise and back to s right after it, so that I in t = Delta m + q0 I has the spread of s~: with Hamming weight h~ = 32 a
 * bound K = 12 keeps the default's K / sigma, the cosine fit needs five levels instead of six, and a bootstrap spends 3 + 5 + 3 + 3 = 14.
 * The price is two key switches per bootstrap.  No security claim is made or changed; what is structural: the key that targets s~
 * exists on two Q limbs and the special limbs only.
 * Definition (residue-exact).  On a client context with the knob on, fhelin_bootstrap_setup draws and generates, in this order, before
 * anything else it draws: (1) s~, ternary with exactly h~ non-zero coefficients, by fhelin_keygen's placement loop on the context's
 * generator; (2) the to-sparse key, a switching key from s to s~, ALWAYS capped at max_ell = 2 whatever the cap table says; (3) the
 * from-sparse key from s~ to s, uncapped or capped by a fhelin_ctx_set_key_caps entry of kind 5 (set the knob first).  Once per context, as the conjugation
 * key; seeded-key mode gives them the nonce kinds 4 and 5 (Galois field 0).  switch(ct, key) = (c0 + KS(c1)[0], KS(c1)[1]) with KS the
 * hybrid key switch, no automorphism (oracle: orc.keyswitch).  The ModRaise step of every pipeline (single, batched, paired, iterative,
 * dropped, level-planned, linear-transform knob, interleaved) is then: y = switch(x2, to-sparse) at two limbs, x2 the two-limb ciphertext
 * the step is about to rescale to q0 (k0 x for a single, the packed k0_a a + i k0_b b for a pair); x1 = rescale(y); up = modraise(x1,
 * top_ell); up = switch(up, from-sparse) at top_ell; SubSum and everything after it unchanged.  Degree, scale and slots pass through the
 * switches; a batch runs each switch as one batched key switch and keeps the residues of the single calls.
 * The setter writes what fhelin_bootstrap_config holds: K = ceil(28 sqrt((h~ + 1) / 193)), R = 3, cheb_degree = 28 when K <= 12 (the
 * largest degree the Chebyshev evaluator takes in five levels; degree 31 takes six) else 47, correction unchanged; a later
 * fhelin_bootstrap_config overrides them.  With the knob on the fit is the Chebyshev series truncated at the degree (from twice the
 * nodes) instead of the interpolant.  depth = budget_enc + budget_dec + R + (levels the evaluator spends on cheb_degree; 6 at 47).
 * 8 <= h~ <= N, anything else FHELIN_ERR_ARG; after fhelin_bootstrap_setup FHELIN_ERR_STATE.  fhelin_key_export / fhelin_key_info kinds
 * 3 (to-sparse, max_ell 2) and 4 (from-sparse); usage recorder and cap table kinds 4 and 5 (Galois element 0; a kind-4 entry is accepted
 * and the to-sparse key still held at two limbs, so a recorded table goes back in as it is).  fhelin_key_info and the cap table know
 * these kinds on a context with the knob on, and refuse them as unknown (FHELIN_ERR_ARG) otherwise.  fhelin_bootstrap_describe
 * appends the pair (2, h~).  Key sets (all formats, always with 48-byte entries): entry kinds 4 and 5 after the conjugation key, Galois
 * field 0, the entry's last word = h~; a context that loads the set adopts h~ and the approximation parameters.  A set written with the
 * knob off is byte for byte what it was; loading one into a context with the knob on names the missing key at fhelin_bootstrap_setup
 * (FHELIN_ERR_KEY).  An evaluation context never holds s~.  Off: no residue, key, file byte or generator draw changes. */
int fhelin_ctx_set_bootstrap_sparse_secret(fhelin_ctx* c, int32_t hamming);
int fhelin_ctx_bootstrap_sparse_secret(const fhelin_ctx* c, int32_t* hamming);
/* test hook: the N coefficients (-1, 0, 1) of s~; client contexts only (FHELIN_ERR_KEY on an evaluation context, FHELIN_ERR_STATE
 * before the set-up made it) */
int fhelin_debug_boot_sparse_secret(fhelin_ctx* c, int8_t* out, size_t cap);
/* test hook, host only: the levels the bootstrap's depth counts for a cosine fit of this degree (>= 1, else FHELIN_ERR_ARG) - the host's
 * restatement of the level bookkeeping of fhelin_eval_chebyshev with every knob at its default and no vanishing coefficient, the
 * result's pending rescale counted.  The tests hold it to the limbs the evaluation really spends. */
int fhelin_debug_cheb_depth(int32_t degree, int32_t* levels);
/* ---- read-only views of the bootstrapping set-up: the residue-level oracle (oracle/residue_boot.py, tests only) composes
 * EvalBootstrap (:445) from the same linear stages, Chebyshev coefficients and keys and must reach the same residues.
 * describe: out = {packed, slots, K, R, cheb_degree, correction, depth, n_c2s, n_s2c, then per stage (CoeffsToSlots stages
 * first): stage_slots, n_terms, n_terms x (giant, baby)}; *n = words needed (fills min(cap, *n)).  With the linear-transform knob on
 * a trailer follows: 1, the n1 asked for, per stage (same order) n1, n2 of the split in use, and the device bytes of the stages'
 * limb-sliced encodings as two words (low, high) - sum over (term, distinct (ell, scale) applied at) of (ell + k) N 8.
 * diag: the plaintext diagonal of term `term` of stage `stage` (which: 0 CoeffsToSlots, 1 SlotsToCoeffs) as a handle for
 * fhelin_pt_export.  cheb: the cosine-fit coefficients EvalMod evaluates.  Key kind 2 of fhelin_key_export = conjugation key. */
int fhelin_bootstrap_describe(fhelin_ctx* c, int32_t* out, int32_t cap, int32_t* n);
int fhelin_bootstrap_diag(fhelin_ctx* c, int32_t which, int32_t stage, int32_t term, fhelin_pt** out);
int fhelin_bootstrap_cheb(fhelin_ctx* c, double* out, int32_t cap, int32_t* n);

/* ---- evaluation-key sets: the server side without the secret key --------------------------------
 * A client context writes its public parameters and all of its PUBLIC key material to one file; a context that never held a
 * secret loads it and then evaluates bit-identically to the client's context ("Client / server split").
 *
 * File format, version 1 (all integers little-endian):
 *   offset  0  char[8]  magic "FHELINEK"
 *           8  u32      version = 1
 *          12  u32      n_keys
 *          16  i32[9]   log_n, n_q, first_bits, scale_bits, n_p (resolved, >= 0), special_bits, dnum, log_slots, hamming
 *                       (fhelin_params without seed and device)
 *          52  i32[7]   bootstrapping as the client set it up: budget_enc, budget_dec, slots, K, R, cheb_degree, correction
 *                       (fhelin_bootstrap_setup / _config); all zero when it was not set up
 *          80  u64      data_offset: first payload byte = (end of the key table) rounded up to a multiple of 4096
 *          88  u64      0, or the interleave stride when it is not 1 ("Interleaved samples": 2, 4, ...; log_slots and the
 *                       bootstrap's slots above stay LOGICAL).  A set written at stride 1 keeps 0 here.
 *          96  u64[n_q + n_p]  the moduli, Q then P: a set whose moduli differ from the chain its parameters give is refused
 *   then the key table, n_keys entries of 40 bytes:
 *           0  u32 kind     0 public key, 1 relinearisation key, 2 rotation key, 3 conjugation key (at most one each of 0, 1, 3)
 *           4  u32 digits   0 for the public key, else the switching key's digit count dnum' = ceil(n_q / alpha)
 *           8  u64 galois   rotation: the Galois element 5^r mod 2N (entries of kind 2 in increasing order); conjugation: 2N - 1;
 *                           else 0.  The conjugation key is stored once (the engine also files it as the rotation key of 2N - 1).
 *          16  u64 offset   byte offset of the payload: payloads follow each other in table order from data_offset, no gaps,
 *                           and the last one ends the file
 *          24  u64 words    payload length in u64 words
 *          32  u64 digest   the key's digest (below)
 *   then the payloads: u64 residues in NTT form, the engine's at-rest layout.  Public key [2][n_q][N] (b = -a s + e, then a);
 *   switching keys [digits][2][n_q + n_p][N] (fhelin_key_export).  Derived copies (permuted / pre-scaled key copies, the
 *   bootstrap's diagonals and Chebyshev coefficients) are not stored: the loading context rebuilds them.  Never stored: the
 *   secret, its 32-byte seed or any generator state.
 * Digest, P = 2^61 - 1, mix(x) = lowbias32 on u32 (x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16):
 *   limb digest of a vector v[0..N) of the payload:  d(v) = sum_i (v_i mod P) * mix(i ^ 0x9E3779B9) mod P
 *   key digest over its n_vec = words / N limb vectors in storage order:  D = sum_j d(v_j) * mix(j | 0x80000000) mod P
 * Every residue must also be below its limb's modulus (vector j of a payload belongs to limb j mod n_q for the public key and
 * j mod (n_q + n_p) for a switching key).  Both are checked on the device (one streaming kernel) before a save writes and after
 * a load uploads, before anything is installed. */
/* write every key the context holds (any context that holds at least one key; FHELIN_ERR_KEY when it holds none) */
int fhelin_evalkeys_save(fhelin_ctx* c, const char* path);
/* the header's parameters (seed and device 0); host-only, no device needed.  A malformed header or key table, or moduli that
 * differ from the chain the parameters give: FHELIN_ERR_ARG */
int fhelin_evalkeys_params(const char* path, fhelin_params* out);
/* the header's bootstrapping configuration (boot7: budget_enc, budget_dec, slots, K, R, cheb_degree, correction; slots 0 = none)
 * and key count; host-only */
int fhelin_evalkeys_info(const char* path, int32_t* boot7, int32_t* n_keys);
/* load a set into a FRESH context with the same parameters (no keygen, no key, no bootstrap set-up: FHELIN_ERR_STATE otherwise;
 * other parameters: FHELIN_ERR_STATE; other moduli, a malformed file, a residue out of range or a digest mismatch:
 * FHELIN_ERR_ARG).  All or nothing: on failure the context holds none of the file's keys.  Afterwards the context is an
 * EVALUATION CONTEXT: decryption, fhelin_secret_export / _import, fhelin_ctx_secret_seed and fhelin_keygen return FHELIN_ERR_KEY;
 * fhelin_gen_relin_key / _rotation_keys / _conj_key succeed when every requested key is present and otherwise return
 * FHELIN_ERR_KEY naming the missing one; fhelin_bootstrap_setup builds its stages from the loaded keys (FHELIN_ERR_KEY naming a
 * missing key); the bootstrap's approximation parameters are taken from the header (call fhelin_bootstrap_setup with its budgets
 * and slots, fhelin_evalkeys_info).  Public-key encryption draws its randomness from this context's own generator (params.seed:
 * 0 = OS entropy). */
int fhelin_evalkeys_load(fhelin_ctx* c, const char* path);
/* test hook: the digest kernel on n_limbs limb vectors words[n_limbs][N] (vector i belongs to limb limb_first + i):
 * out_digests[i] = d(words[i]), out_ok[i] = 1 if every residue is below the limb's modulus */
int fhelin_debug_key_digest(fhelin_ctx* c, const uint64_t* words, int32_t n_limbs, int32_t limb_first, uint64_t* out_digests,
                            int32_t* out_ok);

/* ---- seeded secret-key encryption and compact ciphertexts -------------------------------------------
 * The party that encrypts is the client, which holds the secret, so it may encrypt with the secret key: c0 = -a s + e + m, c1 = a
 * with a uniform and e one rounded Gaussian (sigma 3.19).  Here a is not random data but the EXPANSION of a public 32-byte seed and a
 * u64 nonce, so c1 never needs to travel: a compact ciphertext carries c0, the seed and the nonce, half the bytes of the full form.
 *
 * Expansion.  c1 of a seeded ciphertext on Q-limb l (ABSOLUTE limb index 0 .. ell-1) at storage position j (the order
 * fhelin_ct_export writes, NTT form): with b = j / 4 and k = j % 4, let W[0..7] be the ChaCha20 block (RFC 8439 block function) for
 * key `seed`, 64-bit block counter (l << 32) | b and 64-bit stream `nonce` - the state layout of fhelin_prng_block: counter in words
 * 12-13, stream in words 14-15 - read as 8 little-endian u64.  Then
 *     c1[l][j] = (W[2k+1] * 2^64 + W[2k]) mod q_l.
 * Every position is independent; the distance from uniform is below 2^-67 per residue.  Since l is the absolute limb index, a
 * ciphertext at a lower level expands to a prefix of the same limbs.
 *
 * Compact format, version 1 (all integers little-endian; exactly 96 + 8 ell + 8 ell N bytes):
 *   offset  0  char[8]  magic "FHELINCC"
 *           8  u32      version = 1
 *          12  u32      header bytes = 96 + 8 ell
 *          16  i32[4]   log_n, ell, deg, slots
 *          32  f64[2]   scale hi, lo (the 80-bit scale as hi + lo, as fhelin_ct_scale gives it)
 *          48  u64      nonce
 *          56  u8[32]   seed
 *          88  u64      digest of c0: the key digest of the evaluation-key format ("Evaluation-key sets" above) over c0's ell limb
 *                       vectors, D = sum_j d(c0[j]) * mix(j | 0x80000000) mod 2^61 - 1
 *          96  u64[ell] q_0 .. q_{ell-1}
 *   then   u64[ell][N]  c0, NTT form */
/* 1: fhelin_encrypt, fhelin_encrypt_batch and fhelin_client_ingest encrypt with the secret key and an expanded c1; 0 (default):
 * public-key encryption.  Each call draws a fresh 32-byte seed from the client's generator; a ciphertext's nonce is its output
 * index within the call.  The calls stay level-plan sources in the same order and count as in public-key mode (a plan recorded in
 * one mode applies in the other).  An evaluation context (no secret): FHELIN_ERR_KEY. */
int fhelin_ctx_set_seeded_encryption(fhelin_ctx* c, int32_t on);
/* size of the compact form; FHELIN_ERR_STATE unless ct is an unmodified seeded encryption (any operation's result, a public-key
 * encryption or an imported value has none) */
int fhelin_ct_compact_bytes(const fhelin_ct* ct, size_t* bytes);
/* write the compact form (fhelin_ct_compact_bytes bytes) to out; an export is a level-plan terminal, as fhelin_ct_export */
int fhelin_ct_export_compact(fhelin_ctx* c, const fhelin_ct* ct, uint8_t* out, size_t cap_bytes);
/* validate a blob's header against itself and its size (magic, version, header size, log_n in [12, 17], 1 <= ell <= 64, exact
 * size, 1 <= deg <= 2, slots a power of two <= N/2, scale): FHELIN_ERR_ARG otherwise.  Host-only, no context. */
int fhelin_compact_info(const uint8_t* blob, size_t bytes, int32_t* log_n, int32_t* ell, int32_t* deg, int32_t* slots);
/* n blobs -> n handles with the full ciphertexts (c0 as stored, c1 expanded; scale, deg and slots exact).  Every c0 is uploaded,
 * range-checked and digested on the device, every c1 expanded in one launch, and the host synchronises once per call.  All or
 * nothing: another log_n or other moduli, a malformed header, a residue >= q or a digest mismatch in ANY blob is FHELIN_ERR_ARG
 * and no handle is created.  Imported values are not level-plan sources and are never lowered (as fhelin_ct_import); works on an
 * evaluation context. */
int fhelin_ct_import_compact(fhelin_ctx* c, const uint8_t* const* blobs, const size_t* sizes, int32_t n, fhelin_ct** outs);
/* test / measurement hook: the expansion kernel alone for n_ct ciphertexts of ell limbs (seed, nonces nonce0 .. nonce0 + n_ct - 1) into
 * scratch, then `reps` more launches timed with device events (ms: mean per launch, 0 when reps = 0); out (optional,
 * [n_ct][ell][N]): the expanded c1 */
int fhelin_debug_seeded_expand(fhelin_ctx* c, const uint8_t* seed32, uint64_t nonce0, int32_t ell, int32_t n_ct, int32_t reps,
                               uint64_t* out, float* ms);

/* ---- seeded evaluation keys: half-size key sets -------------------------------------------------------
 * Half of every key is its uniform part a.  In seeded-key mode a is not random data but the expansion of a public 32-byte
 * KEY-SET SEED and a per-digit nonce, so a compact key set stores the b halves and the seed, and the loading context rebuilds
 * every a on the device.
 *
 * Key-set seed.  Drawn in fhelin_keygen from the client's generator right after the secret is placed and before the public key:
 * the next four u64 of the stream, written little-endian (byte 8 i + k = byte k of word i, as the per-call seeds of seeded
 * encryption).  Two contexts made from the same secret seed therefore make identical keys.  The seed is public.
 *
 * Nonce of digit `digit` of a key:  nonce = (kind << 56) | (digit << 40) | galois, with kind 0 public key (digit 0, galois 0),
 * 1 relinearisation key (galois 0), 2 rotation key (galois 5^r mod 2N), 3 conjugation key (galois 2N - 1, stored once).
 *
 * Expansion.  The formula of "Compact ciphertexts" above with the limb index over the whole key basis Q then P: residue j of limb
 * l (0 <= l < n_q + n_p) of a digit's a half is (W[2k+1] * 2^64 + W[2k]) mod m_l, b = j / 4, k = j % 4, m_l the l-th modulus of Q
 * then P, W the ChaCha20 block for key = seed, counter (l << 32) | b and stream = nonce.  The public key uses l < n_q only.
 * The b halves are those of the full keys: b = -a s_to + e (+ (P mod q_t) s_from on the limbs t of digit j), e one rounded
 * Gaussian (sigma 3.19) per digit.
 *
 * Compact key-set format, version 1: the evaluation-key format above with these changes.
 *   offset  0  char[8]  magic "FHELINEC"
 *           8  u32      version = 1
 *          12 .. 95     as version 1 of "FHELINEK" (n_keys, parameters, bootstrapping, data_offset, reserved)
 *          96  u8[32]   the key-set seed
 *         128  u64[n_q + n_p]  the moduli, then the key table (40-byte entries, as version 1)
 *   data_offset = (end of the key table) rounded up to a multiple of 4096.  An entry's `words` counts what is stored: the b halves
 *   only, [digits][n_q + n_p][N] for a switching key (digit j's b half, then digit j + 1's) and [n_q][N] for the public key.  Its
 *   `digest` is the version 1 digest of the FULL key (b and the expanded a, in version 1 storage order): the loader expands every
 *   a before it digests, so a wrong seed, Galois element or expansion fails the digest, and a compact set's digests equal those
 *   of the version 1 set of the same keys. */
/* on: fhelin_keygen draws a key-set seed and every key the context makes afterwards is seeded (its a half made on the device from
 * the seed, no host sampling).  Call before fhelin_keygen: after keygen, or once the context holds any key, FHELIN_ERR_STATE; on an
 * evaluation context FHELIN_ERR_KEY.  Off (the default): key generation consumes the generator exactly as without this mode. */
int fhelin_ctx_set_seeded_keys(fhelin_ctx* c, int32_t on);
/* the public key-set seed (32 bytes); FHELIN_ERR_STATE when the keys are not seeded.  Works on a context loaded from a compact set. */
int fhelin_ctx_key_set_seed(const fhelin_ctx* c, uint8_t* out32);
/* write every key the context holds as a compact set.  FHELIN_ERR_KEY when it holds none; FHELIN_ERR_STATE, naming the key, when any
 * key it holds is not seeded (made outside seeded-key mode, or installed with fhelin_key_import).  A context loaded from a compact
 * set writes the identical bytes.  fhelin_evalkeys_save still writes version 1 (full keys) for every context.
 * fhelin_evalkeys_params, _info and _load read both formats; loading a compact set streams the b halves, expands every a half in
 * one launch, digests and installs as version 1 does (all or nothing). */
int fhelin_evalkeys_save_compact(fhelin_ctx* c, const char* path);

/* ---- wrapped inputs: a sample uploaded as a few ciphertexts, unwrapped on the server -------------------------------------
 * Layout.  A WRAPPED ciphertext holds count <= 128 inputs of one sample (inputs numbered in the driver's read order: the 32
 * E-projected rows, the 32 F-projected rows, the S + 1 tokens; total = 64 + S + 1): slot j*128 + t = row_t[j] for t < count, the
 * other slots 0 (the reference's wrapUpExpanded, src/FHEController.cpp:1070).  Unwrap output t has exactly the slot values of
 * read_expanded_input(row_t): slot j*128 + k = row_t[j] for all k < 128.
 * Levels.  Inputs wanted at ell limbs travel over the FIRST ell + 1 MODULI OF Q THEN P: q_0..q_ell for ell < n_q, and
 * q_0..q_{n_q-1}, p_0 for ell = n_q.  The client encrypts at Delta_ell, the 80-bit scale of a fresh encryption at ell limbs.  The
 * server multiplies by the 0/1 mask of slot column t encoded at scale q_drop (the extra limb's modulus) and drops that limb as a
 * rescale does: each output has ell limbs, degree 1, the slot count and the bit-identical scale of a fresh encryption at ell limbs.
 * Encryption.  Always a seeded secret-key encryption ("Compact ciphertexts" above); the expansion of c1 runs over the absolute limb
 * index 0..ell of Q then P (the p_0 limb is limb n_q), as for seeded keys.  One fresh seed per call; nonce = the wrapped
 * ciphertext's index within the call.
 * Grouping.  The inputs of one target limb count share wrapped ciphertexts, at most 128 each, filled in read order.  The targets are
 * taken in the order of their first input, and all ciphertexts of one target come out before those of the next.  A wrapped handle
 * carries count, total and its inputs' positions.  Encoding and encryption run once per run of up to 32 ciphertexts of one target
 * (at the headline ring: one run per target, so 1 without a level plan and 2 under one).
 * Unwrap.  out_t = sum_{k<128} rot(x_t, t - k) with x_t the masked drop; with t = a + 8b + 64c that is three merged rotate-and-sum
 * key switches (fhelin_rotate_sum), offsets {a-7..a}, 8{b-7..b} and {64c-64, 64c} without the identity term: every offset is a
 * +-1..7, +-8..56 (step 8) or +-64, all in the circuit's rotation key list.  A missing key: FHELIN_ERR_KEY naming its index.
 * Handles.  A wrapped handle is accepted by fhelin_unwrap_inputs, fhelin_decrypt, fhelin_decrypt_flooded, fhelin_decrypt_interleaved
 * and fhelin_decrypt_batch (the extra limb left out; the slots come back in the wrapped layout), fhelin_ct_info (ell counts the extra limb; level is the inputs' level), fhelin_ct_scale, fhelin_wrapped_info, the compact functions and
 * fhelin_ct_free; every other entry point returns FHELIN_ERR_ARG.
 * Compact form, version 2 (a wrapped ciphertext; version 1 above is unchanged; exactly H + 8 ell N bytes, H = 104 + 8 ell + 8 ceil(count / 2)):
 *   offset  0 .. 95  as version 1 with version = 2 and header bytes = H; ell = the stored limbs (the inputs' limbs + 1, >= 2)
 *          96  u32      count (1 .. 128)
 *         100  u32      total (count .. 65535): inputs of the sample
 *         104  u64[ell] the first ell moduli of Q then P
 *   104 + 8 ell  u32[count] the inputs' positions (strictly increasing, < total), zero padding to H
 *   then   u64[ell][N]  c0, NTT form (digest as version 1, over the ell limb vectors)
 * Import (fhelin_ct_import_compact) checks both versions with the same all-or-nothing digest and range checks and makes wrapped
 * handles of version 2 blobs. */
/* The client side of one sample (fhelin_client_ingest's arguments) as wrapped ciphertexts.  targets [64 + S + 1] (optional): the limbs
 * each input is wanted at (1 .. n_q); NULL: n_q - level for all, or, while a level plan is applied on this context, the plan's targets
 * of the sources the unwrap will produce (read, not consumed: this call is no level-plan source).  outs must hold 64 + S + 1 handles;
 * *n_out = wrapped ciphertexts made.  Needs the secret key (FHELIN_ERR_KEY on an evaluation context) and n_p >= 1.  A context with
 * interleaved samples (stride > 1) gets FHELIN_ERR_STATE: fhelin_client_ingest_wrapped_interleaved ("Interleaved samples" below)
 * takes its place, as fhelin_client_ingest_interleaved takes fhelin_client_ingest's. */
int fhelin_client_ingest_wrapped(fhelin_ctx* c, const double* emb, const int32_t* tokens, const double* table, int32_t vocab, int32_t S,
                                 const double* cls, const double* pos, const double* E_w, const double* E_b, const double* F_w,
                                 const double* F_b, int32_t w_cols, int32_t level, const int32_t* targets, fhelin_ct** outs,
                                 int32_t* n_out, double* proj_out);
/* count, total, the inputs' limbs (stored limbs - 1) and positions (min(cap, count) of them) of a wrapped handle; FHELIN_ERR_ARG otherwise */
int fhelin_wrapped_info(const fhelin_ct* ct, int32_t* count, int32_t* total, int32_t* ell, int32_t* positions, int32_t cap);
/* n wrapped handles -> sum of their counts outputs.  Consecutive handles whose counts add up to their total are one sample (B samples of
 * a batched pass in one call); outs: sample by sample, each in read order - the handles fhelin_client_ingest would have given.  The
 * masked drop of every input is one launch; the replications of all inputs share batched key switches.  The outputs are level-plan
 * sources with the ordinals fhelin_client_ingest's outputs have (a plan recorded with either applies to the other).  Applying, an
 * output whose input was wrapped above its planned limbs tau is made at tau directly: the masked product reads the first tau + 1
 * limbs, with the mask encoded at Delta_tau q_tau / Delta_ell, and the output has the fresh scale Delta_tau, as fhelin_client_ingest's
 * planned output.  Works on an evaluation context that holds the circuit's rotation keys. */
int fhelin_unwrap_inputs(fhelin_ctx* c, const fhelin_ct* const* wrapped, int32_t n, fhelin_ct** outs);

/* ---- interleaved samples: several samples in the idle slots of one ciphertext (slot stride) -------------------------------
 * A ring of dimension N has N/2 slots; a circuit written for n = 2^log_slots slots leaves the rest idle when n < N/2.  With the
 * SLOT STRIDE s (1, 2, 4, ... with n * s <= N/2) a ciphertext carries s sample vectors z_0 .. z_{s-1} of n LOGICAL slots in its
 * n * s PHYSICAL slots, w[s k + i] = z_i[k].  A physical rotation by s r rotates every z_i by r with the cyclic wrap of n, and
 * every slot-wise operation acts sample by sample, so one pass of an unchanged circuit serves s samples.  The client packs
 * (merging separately encrypted samples on the server would be a full linear transform).
 * With the stride set, every entry point keeps its signature and speaks LOGICAL slots and LOGICAL rotation indices:
 *   - fhelin_rotate*, fhelin_hoisted_dot, fhelin_gen_rotation_keys, fhelin_key_export / _import (kind 1), fhelin_raw_rotate, every
 *     fhelin_fc_* / fhelin_fcb_* composite and fhelin_unwrap_inputs use the Galois element 5^(s r) for the index r.  As at stride 1
 *     the index is not reduced modulo n first: r and r + n rotate the samples alike and are different Galois elements (and keys)
 *     unless n * s = N/2.
 *   - fhelin_ct_info and fhelin_compact_info report logical slots.
 *   - fhelin_encode, fhelin_encrypt and fhelin_encrypt_batch REPLICATE their values into all s samples (model weights, masks, the
 *     mask of fhelin_sanitize, a driver's own server-side encryptions).
 *   - fhelin_decrypt and fhelin_decrypt_flooded return sample 0.
 *   - fhelin_bootstrap_setup takes logical slots and sets bootstrapping up for slots * s physical slots; the bootstrap's own
 *     rotations, diagonals and keys belong to the physical packing, and fhelin_bootstrap_describe / _diag describe the PHYSICAL
 *     stages (slot counts, giant and baby shifts of the slots * s packing).
 *   - fhelin_client_ingest and fhelin_client_ingest_wrapped return FHELIN_ERR_STATE; fhelin_client_ingest_interleaved and
 *     fhelin_client_ingest_wrapped_interleaved below take their place.
 *   - wrapped inputs: a wrapped ciphertext of a group holds the same inputs of every sample, logical slot j*128 + t = row_{i,t}[j] of
 *     sample i in the physical slot s (j*128 + t) + i.  fhelin_unwrap_inputs serves all lanes at once - the mask is replicated, the
 *     rotations are 5^(s r), a missing key is named by its logical index - and output t has, in every lane i, the slot values of
 *     read_expanded_input(row_{i,t}), with the limbs, degree, logical slots, 80-bit scale and level-plan ordinal of
 *     fhelin_client_ingest_interleaved's output t.  Every entry point that accepts a wrapped handle does so under a stride:
 *     fhelin_decrypt returns sample 0 in the wrapped layout (the extra limb left out), fhelin_decrypt_interleaved and
 *     fhelin_decrypt_batch(all_lanes) every lane, fhelin_ct_info logical slots.  NO FORMAT CHANGE: a version-2 compact blob is
 *     stride-agnostic, as a version-1 blob of an interleaved ciphertext is; the importing context's stride gives it its meaning, and
 *     the key set carries the stride.
 * Evaluation-key sets record the stride (header offset 88): fhelin_evalkeys_load into a fresh context adopts it; a context whose
 * stride was set explicitly (fhelin_ctx_set_interleave) to another value gets FHELIN_ERR_STATE.  stride 1, the default, changes
 * nothing: no launch, byte, residue or file. */
/* set the stride: before the first key, plaintext, ciphertext or bootstrap set-up exists on the context (FHELIN_ERR_STATE later);
 * FHELIN_ERR_ARG for a stride that is no power of two or with 2^log_slots * stride > N/2.  Works on a host-only context. */
int fhelin_ctx_set_interleave(fhelin_ctx* c, int32_t stride);
int fhelin_ctx_interleave(const fhelin_ctx* c, int32_t* stride);
/* the stride an evaluation-key set (full or compact) was written at; host-only */
int fhelin_evalkeys_interleave(const char* path, int32_t* stride);
/* fhelin_encrypt_batch for n_vec ciphertexts of `stride` samples each: vals [n_vec][stride][n_per].  Domain checks, chunking,
 * level-plan sources and sampler draws of fhelin_encrypt_batch with n_vec vectors; the interleaving happens in front of the encoder
 * and draws nothing. */
int fhelin_encrypt_interleaved_batch(fhelin_ctx* c, const double* vals, int32_t n_vec, int32_t n_per, int32_t level, int32_t slots,
                                     fhelin_ct** outs);
/* every sample of a ciphertext: out [stride][slots] (slots <= 0: the ciphertext's); flood_bits as fhelin_decrypt_flooded, 0 = plain */
int fhelin_decrypt_interleaved(fhelin_ctx* c, const fhelin_ct* ct, int32_t flood_bits, double* out, int32_t slots);
/* fhelin_client_ingest for n_samples == stride samples of one length S: emb / tokens are arrays of n_samples pointers (emb NULL:
 * token ids into the shared table), cls / pos / E / F are shared.  outs: the 64 + S + 1 handles of the GROUP, sample i in the
 * physical slots = i mod stride; proj_out (NULL, or n_samples pointers to [(S + 1 + 64)][128]): per sample exactly what
 * fhelin_client_ingest reports for it.  The sampler draws are those of ONE fhelin_client_ingest. */
int fhelin_client_ingest_interleaved(fhelin_ctx* c, int32_t n_samples, const double* const* emb, const int32_t* const* tokens,
                                     const double* table, int32_t vocab, int32_t S, const double* cls, const double* pos,
                                     const double* E_w, const double* E_b, const double* F_w, const double* F_b, int32_t w_cols,
                                     int32_t level, fhelin_ct** outs, double* const* proj_out);
/* fhelin_client_ingest_wrapped for n_samples == stride samples of one length S (emb / tokens / proj_out as
 * fhelin_client_ingest_interleaved; cls / pos / E / F and targets are shared by the group): the group's wrapped ciphertexts in the
 * layout above, columns without an input 0 in every lane.  Grouping by target, the moduli and the scale, targets == NULL and the peek
 * at an applied level plan, positions, total and *n_out are exactly fhelin_client_ingest_wrapped's; so are the sampler draws (one
 * fresh seed, nonce = the wrapped ciphertext's index: interleaving draws nothing), and a group costs the bytes of one sample.
 * proj_out[i] is bit for bit what fhelin_client_ingest_wrapped reports for sample i alone.  At stride 1 with one sample the call IS
 * fhelin_client_ingest_wrapped.  FHELIN_ERR_ARG: n_samples != stride, a NULL sample, a token id outside the table, bad S / level /
 * targets (before any launch); FHELIN_ERR_KEY on an evaluation context; FHELIN_ERR_STATE with n_p = 0. */
int fhelin_client_ingest_wrapped_interleaved(fhelin_ctx* c, int32_t n_samples, const double* const* emb, const int32_t* const* tokens,
                                             const double* table, int32_t vocab, int32_t S, const double* cls, const double* pos,
                                             const double* E_w, const double* E_b, const double* F_w, const double* F_b, int32_t w_cols,
                                             int32_t level, const int32_t* targets, fhelin_ct** outs, int32_t* n_out,
                                             double* const* proj_out);

/* ---- sanitised replies: mask, shrink, re-randomise and flood what a server hands back -------------------------------------
 * The ciphertext a circuit ends with is no fit reply as it stands: only some slots are the answer (the others hold intermediate
 * values of the model), (c0, c1) is a deterministic function of inputs, keys and model whose limb count, roundings and noise depend on
 * the circuit that ran, and decryption reads two limbs of it.  fhelin_sanitize makes the reply, in this order:
 *   1. degree-2 inputs are rescaled (as fhelin_decrypt does);
 *   2. with a mask - an ordinary plaintext of 0/1 slot values - product and rescale (fhelin_mult_plain_batch, fhelin_rescale_batch):
 *      one limb, the masked-out slots hold rounding noise only;
 *   3. out0 = in0 + pk_b u + NTT(e0 + f), out1 = in1 + pk_a u + e1 on the FIRST out_ell limbs (the level drop is part of the same
 *      pass): u uniform ternary, e0 and e1 rounded Gaussians (sigma 3.19) - a fresh public-key encryption of zero - and f the
 *      flooding term, uniform on [-2^flood_bits, 2^flood_bits) per coefficient.  One fused launch for the whole batch; the
 *      randomness is sampled on the device, transformed by one forward NTT and wiped afterwards.
 * flood_bits = 0: re-randomisation only.  out_ell <= 0: 2.  Outputs: 2 components, out_ell limbs, degree 1, the (masked) input's
 * scale and slots; never seeded.  Needs the public key only: works on an evaluation context (FHELIN_ERR_KEY without a public key).
 * Randomness: a ChaCha20 key per sampler call drawn from the CONTEXT'S OWN generator, exactly as public-key encryption draws it - a
 * server creates its context with a seed of its own (fhelin_ctx_create: OS entropy), never with the client's.
 * FHELIN_ERR_ARG: flood_bits outside [0, 62]; 2^(flood_bits + 2) not below q_0 .. q_{out_ell-1}; fewer limbs than the rescales, the
 * mask and out_ell need; a 3-component input; a wrapped input; n < 1.  FHELIN_ERR_NO_DEVICE on a host-only context.  Nothing is
 * launched when a call is refused.
 * What flooding hides: the noise the circuit left (key-switch and rescale roundings, whose distribution depends on the model) under
 * a term 2^flood_bits / that noise times larger.  What it does not: the approximation error of the circuit is part of the MESSAGE,
 * and the kept slots carry it.  flood_bits is the caller's trade: the slot error it adds is about 2^flood_bits sqrt(N/3) / scale.
 * The wide sampler, exactly: coefficient i of polynomial p uses the little-endian u64 word W = word (i mod 8) of ChaCha20 block
 * (key, counter = i / 8, stream + p); f_i = (W >> (63 - B)) - 2^B for 1 <= B <= 62; the residue on limb l is f_i mod q_l in [0, q_l). */
int fhelin_sanitize(fhelin_ctx* c, const fhelin_ct* const* v, int32_t n, const fhelin_pt* mask /* may be NULL */, int32_t flood_bits,
                    int32_t out_ell, fhelin_ct** outs);
/* test hook: the flood term alone for an explicit key (32 bytes) and stream, residues [ell][N] in coefficient form; 1 <= flood_bits <= 62 */
int fhelin_debug_flood(fhelin_ctx* c, const uint8_t* key, uint64_t stream, int32_t flood_bits, int32_t ell, uint64_t* out, size_t cap_words);
/* ---- sampler streams: which ChaCha20 key and stream every random polynomial comes from ---------------------------------------
 * The context's generator G is the ChaCha20 stream (key = the secret seed, stream 0, block counter 0, 1, ...) read as little-endian
 * u64 words in order (8 per block).  A KEY DRAW takes the next four words w0..w3 of G: sampler key words k[2i] = low 32 bits of w_i,
 * k[2i+1] = high 32 bits.  The context also keeps a counter C of sampler calls (0 at creation).  Polynomial p of a sampler call made
 * with key K at counter value c uses the blocks ChaCha20(K, block counter = i / 8, stream = (c << 32) + p); W_j is u64 word j of it:
 *   ternary : coefficient 8 b + j = ((W_j * 3) >> 64) - 1                                                   (block b, j = 0..7)
 *   Gaussian: u1 = ((W_2j >> 11) + 1) 2^-53, u2 = (W_2j+1 >> 11) 2^-53, r = 3.19 sqrt(-2 ln u1);
 *             coefficient 8 b + 2 j = round(r cos 2 pi u2), coefficient 8 b + 2 j + 1 = round(r sin 2 pi u2)   (j = 0..3), |e| <= 28
 *   flood   : coefficient 8 b + j = (W_j >> (63 - B)) - 2^B                                                  (as fhelin_sanitize)
 * and the same integer polynomial is written to every limb as its residue in [0, q_l).  Callers, in the order they draw:
 *   fhelin_debug_sample(kind, n)  : one key draw; polynomial p at stream (C << 32) + p; C += 1.
 *   public-key encryption of n <= 32 vectors (fhelin_encrypt: n = 1; fhelin_encrypt_batch and fhelin_client_ingest: once per chunk of
 *     at most 32 vectors of one level, chunks in order): key draw 1, u_b (ternary) at (C << 32) + b; key draw 2, e0_b (Gaussian) at
 *     ((C + 1) << 32) + b and e1_b at ((C + 1) << 32) + n + b - one call of 2 n polynomials; C += 2.
 *     c0_b = pk_b NTT(u_b) + NTT(e0_b) + m_b, c1_b = pk_a NTT(u_b) + NTT(e1_b).
 *   seeded secret-key encryption: the call's 32-byte public seed is the next four words of G (little-endian bytes), drawn once per
 *     fhelin_encrypt / fhelin_encrypt_batch / ingest call; then per chunk of at most 32 vectors one key draw, e_b (Gaussian) at
 *     (C << 32) + b; C += 1.  c0_b = m_b - a_b s + NTT(e_b).
 *   fhelin_sanitize, per chunk of at most 32 ciphertexts (chunks in order; the mask and the rescales draw nothing):
 *     flood_bits = 0: key draw 1, u_b at (C << 32) + b; key draw 2, e0_b at ((C + 1) << 32) + b; key draw 3, e1_b at
 *       ((C + 2) << 32) + b; C += 3.
 *     flood_bits > 0: key draw 1, u_b at (C << 32) + b; key draw 2 serves two stream ranges, f_b (flood) at ((C + 1) << 32) + b and
 *       e0_b (Gaussian) at ((C + 2) << 32) + b; key draw 3, e1_b at ((C + 3) << 32) + b; C += 4.
 *     out0_b = in0_b + pk_b NTT(u_b) + NTT(e0_b + f_b), out1_b = in1_b + pk_a NTT(u_b) + NTT(e1_b) on the first out_ell limbs.
 *   fhelin_decrypt_flooded (flood_bits > 0): one key draw, f (flood, no Gaussian) at (C << 32); C += 2 (the unused Gaussian range
 *     is skipped).
 *   fhelin_decrypt_batch (flood_bits > 0; "Batched decryption"): one key draw per CALL, f_b of ciphertext b at (C << 32) + b; C += 2.
 *   seeded fhelin_keygen: the secret's draws from G, then the key-set seed (the next four words of G), then one key draw: the public
 *     key's e (Gaussian, one polynomial over the Q limbs) at (C << 32); C += 1.  pk_b = NTT(e) - pk_a s.
 *   seeded switching keys (fhelin_gen_relin_key, each rotation key, fhelin_gen_conj_key): one key draw per key; digit j's e_j
 *     (Gaussian, one polynomial over the Q and P limbs) at (C << 32) + j; C += 1.
 * Key generation without seeded keys samples on the host, straight from G.
 * Test hook: the keys the next n_keys key draws will give (key_words [n_keys][8]; computed on a copy of G, nothing is consumed) and
 * the current C.  Works on client and evaluation contexts and without a device.  It reveals nothing the owner of the context cannot
 * derive from fhelin_ctx_secret_seed (an evaluation context: from the seed it was created with).  FHELIN_ERR_ARG: n_keys outside
 * [0, 4096].  key_words may be NULL when n_keys = 0; sample_calls may be NULL. */
int fhelin_debug_sampler_peek(const fhelin_ctx* c, int32_t n_keys, uint32_t* key_words /* [n_keys][8] */, uint64_t* sample_calls);
/* noise-flooding decryption: fhelin_decrypt with one flood polynomial (uniform on [-2^flood_bits, 2^flood_bits), the wide sampler,
 * keyed from the context's generator) added to the phase after the inverse NTT and before the download, on the one or two limbs
 * decryption reads - values a client shares then do not expose the exact noise.  flood_bits = 0: exactly fhelin_decrypt.
 * FHELIN_ERR_ARG: flood_bits outside [0, 62] or 2^(flood_bits + 2) not below the modulus of the limbs read. */
int fhelin_decrypt_flooded(fhelin_ctx* c, const fhelin_ct* ct, int32_t flood_bits, double* out, int32_t slots);

/* ---- batched decryption: a batch of ciphertexts decoded on the device, one download and one synchronisation ------------------
 * fhelin_decrypt computes the phase and one inverse NTT on the device, downloads the one or two limbs it reads (N words each), drains
 * the stream and decodes on one host thread: CRT lift in long double, division by the scale, forward special FFT.
 * fhelin_decrypt_batch does all of that on the device for n ciphertexts at once - one phase launch, ONE inverse NTT over every limb
 * read, the lift and division in integer code, the forward FFT, a gather of the slots that were asked for - and then downloads exactly
 * those doubles with ONE copy and ONE stream synchronisation.  Every double is the one fhelin_decrypt gives, bit for bit.
 *   out    [n][L][W].  L = 1: sample 0 of every ciphertext, as fhelin_decrypt; all_lanes != 0: L = the context's interleave stride and
 *          the lanes in fhelin_decrypt_interleaved's order.  W = slots, or n_idx when idx is given.
 *   idx    NULL, or n_idx logical slot numbers in [0, slots), any order, repeats allowed: out[b][l][k] = slot idx[k].
 *   slots  <= 0: the ciphertexts' own slot count, which must then agree across the batch.
 * The batch may mix limb counts (one limb, two or more), scales, degrees and wrapped inputs.  Degree-2 inputs above two limbs are
 * rescaled first, all of them in one batched rescale; deferred rows are evaluated as for any other reader; under a level plan every
 * ciphertext counts as one decryption, in order.
 * Randomness (flood_bits > 0, "Sampler streams"): ONE key draw per call, the flood of ciphertext b at (C << 32) + b; C += 2.  A batch
 * of one therefore IS fhelin_decrypt_flooded; a batch of n is NOT n single calls (those draw n keys and advance C by 2 n).  The flood
 * scratch is zeroed afterwards.
 * FHELIN_ERR_KEY: an evaluation context.  FHELIN_ERR_NO_DEVICE: a context without a device.  FHELIN_ERR_ARG: a null array, entry or
 * out; n < 0 or above 65535; idx out of range, or n_idx <= 0 with idx given; disagreeing slot counts with slots <= 0; slots x stride
 * not a power of two <= N/2; flood_bits outside [0, 62] or too wide for the limbs read.  n = 0 is FHELIN_OK and touches nothing.  A
 * refused call draws nothing and leaves C where it found it. */
int fhelin_decrypt_batch(fhelin_ctx* c, const fhelin_ct* const* cts, int32_t n, int32_t flood_bits, int32_t all_lanes, const int32_t* idx,
                         int32_t n_idx, double* out, int32_t slots);
/* on != 0: fhelin_decrypt, fhelin_decrypt_flooded and fhelin_decrypt_interleaved run as batches of one through the device decoder (the
 * same doubles; slots x stride must then be a power of two); 0, the default, and they execute the host decoder as before.  Also
 * FHELIN_DEVICE_DECODE=1 in the environment when the context is created. */
int fhelin_ctx_set_device_decode(fhelin_ctx* c, int32_t on);

/* ---- level-capped keys: generate, ship and hold keys only as deep as their use ----------------------------------------------
 * A hybrid key switch at ell live limbs reads the first digits_at(ell) = ceil(ell / alpha) digits of its key and, within them, the Q rows
 * 0 .. ell-1 and the n_p special rows.  A key that is only ever used at ell <= max_ell therefore needs nothing else.  A CAPPED key
 * (relinearisation, rotation or conjugation) carries max_ell, 1 <= max_ell < n_q; max_ell = n_q is an uncapped key, today's in every
 * respect.  Its digit count is digits' = digits_at(max_ell); its PRESENT ROWS are, for digits 0 .. digits'-1 and both halves, the Q limbs
 * 0 .. max_ell-1 and all n_p special limbs.
 *
 * Sub-block rule: a capped key is, residue for residue, the present rows of the key the same context would have made uncapped at that
 * point - in default mode and in seeded-key mode (digit j encrypts (P mod q_t) s_from on digit j's own limbs whatever the level of its
 * later use; the seeded a half's nonce is per digit and its limb index absolute).  Generating it consumes the client generator and the
 * device sampler exactly as generating the uncapped key does, so every key made afterwards is unchanged too; and every operation at
 * ell <= max_ell gives bit-identical results with the capped and with the uncapped key.
 *
 * Device layout: [digits'][2][n_q + n_p][N] - the limb stride of every key, so no key-switch kernel knows about caps; the absent Q rows
 * are zero-filled once, when the key is made.  fhelin_key_export writes exactly that (digits' digits, absent rows zero).  The permuted
 * and the folded copies have the key's own digit count.  What the cap saves in device memory is the digits dropped.  fhelin_key_import
 * installs uncapped keys only.
 *
 * Enforcement: every place that binds a key to a launch at ell limbs checks ell <= max_ell first (rotations of every form, hoisted
 * dots and their folded keys, linear transforms, relinearisation in every product, the bootstrap's SubSum, linear stages and
 * conjugations).  A switch above the cap is FHELIN_ERR_KEY; the message names the key (rotation index where the context generated it,
 * Galois element), its cap and the limbs asked for.  The refused call counts no key switch, returns no handle and leaves the level plan
 * where it was; in a deferred operation the error surfaces where that operation's errors surface.
 *
 * File formats: VERSION 2 of both "FHELINEK" and "FHELINEC".  The header is version 1's; the key table has 48-byte entries - the 40
 * bytes of version 1, then u32 max_ell, then u32 0 (reserved).  The public key and uncapped keys carry n_q in max_ell.
 *   full    payload of a switching key [digits'][2][max_ell + n_p][N]; words counts the stored words; digest covers what is stored
 *   compact payload [digits'][max_ell + n_p][N], the b halves; words counts the stored words; digest is the version 2 FULL form's: b
 *           and the expanded a, in storage order
 * Vector j of a payload belongs to limb r = j mod (max_ell + n_p): Q limb r if r < max_ell, else special limb r - max_ell.  Digest
 * definition and 4096-byte alignment are unchanged.  A context that holds no capped key writes version 1, byte for byte as before;
 * otherwise version 2; a context loaded from a version 2 set rewrites identical bytes.  fhelin_evalkeys_params, _info and _load read
 * versions 1 and 2 of both magics and refuse, all or nothing with FHELIN_ERR_ARG, max_ell outside 1 .. n_q, digits other than
 * digits_at(max_ell), words that do not match, and a non-zero reserved word.  A loaded capped key is enforced like a generated one. */
/* The cap table of a client context: n entries (kind, galois, max_ell); kind 1 relinearisation (galois 0), 2 rotation (its Galois
 * element: valid at any interleave stride), 3 conjugation (galois 2N-1), as in the key-set file.  Every key the context generates
 * AFTERWARDS that matches an entry is generated capped - fhelin_gen_relin_key, fhelin_gen_rotation_keys, fhelin_gen_conj_key, the keys
 * fhelin_bootstrap_setup generates itself, the keys of wrapped inputs and linear transforms.  Keys without an entry, or with
 * max_ell = n_q, are uncapped.  A second call replaces the table (n = 0 clears it).  Checked before anything changes, in this order: an
 * evaluation context FHELIN_ERR_KEY; kind, max_ell or galois out of range, or a duplicate entry FHELIN_ERR_ARG; an entry for a key the
 * context already holds FHELIN_ERR_STATE.  Works on a host-only context. */
int fhelin_ctx_set_key_caps(fhelin_ctx* c, const int32_t* kind, const uint64_t* galois, const int32_t* max_ell, int32_t n);
/* digits held, max_ell and whether the key is seeded; kind / index as fhelin_key_export (0 relinearisation, 1 rotation by index,
 * 2 conjugation); any out pointer may be NULL.  FHELIN_ERR_KEY: key not present. */
int fhelin_key_info(fhelin_ctx* c, int32_t kind, int32_t index, int32_t* digits, int32_t* max_ell, int32_t* seeded);
/* Usage recorder: between _begin and _end every key switch the context issues notes max(ell) for its key - on the host, where the key
 * is bound to its launch (the same place as the cap check).  _end first evaluates everything deferred on all lanes, then returns the
 * table sorted by (kind, galois) in the encoding fhelin_ctx_set_key_caps takes: *n = its length, min(cap, *n) entries filled.  A key
 * that was never used has no entry; the conjugation key is reported once, as kind 3.  Works on evaluation contexts; changes no result
 * and no level-plan state.  _begin clears the table and (re)starts the recording; _end stops it, and the table stays readable through
 * further _end calls until the next _begin (a caller sizes its buffers with cap = 0 first).  The table is a property
 * of the program and its level plan, not of the data: caps recorded under one plan are valid for that plan only - a pass that goes
 * higher is refused with FHELIN_ERR_KEY, it does not silently misdecrypt. */
int fhelin_key_usage_begin(fhelin_ctx* c);
int fhelin_key_usage_end(fhelin_ctx* c, int32_t* kind, uint64_t* galois, int32_t* max_ell, int32_t cap, int32_t* n);

/* ---- packed formats: residues travel at their modulus width -----------------------------------------------------------------
 * No modulus of an accepted chain has more than 60 bits, and a residue below m carries at most bitlen(m) bits.  The packed formats
 * store exactly that many; device memory and every kernel that computes keep the u64 layout.
 *
 * Packed limb vector.  For a modulus m, w(m) is the number of bits of m, 20 <= w <= 60.  A vector v[0..N) of residues below m becomes
 * a bit stream of N w bits: residue j occupies stream bits [j w, (j+1) w), least significant bit first; stream bit t is bit t mod 64
 * of word t / 64; words are little-endian.  N is a multiple of 4096, so a packed vector is exactly N w / 64 words: every vector starts
 * on a word boundary and there is no padding.  A packed payload is the limb vectors of the unpacked payload in the same storage order,
 * each packed at the width of its own limb's modulus.
 *
 * Digests are unchanged: every digest in a packed object is the existing digest ("Evaluation-key sets") of the UNPACKED residues in
 * unpacked storage order.  Unpacking can produce any w-bit value; the range check (residue < modulus) and the digest run on the
 * unpacked data, exactly as the other loaders run them, and decide acceptance, all or nothing.
 *
 * Ciphertext blob "FHELINCP", version 1.  Size exactly H + stored * sum_{l < ell} N w_l / 8 bytes.
 *    0  char[8] "FHELINCP"      8  u32 version = 1      12 u32 header bytes H = 112 + 8 ell + 8 ceil(count / 2)
 *   16  i32[4]  log_n, ell, deg, slots                  32 f64[2] scale hi, lo (as fhelin_ct_scale)
 *   48  u64 nonce   56 u8[32] seed                      88 u64 digest over the stored * ell vectors (vector j belongs to limb j mod ell)
 *   96  u32 stored: 1 = seeded form (c0 stored, c1 = the expansion of seed and nonce, "Compact ciphertexts");
 *                   2 or 3 = every component stored, fhelin_ct_export order; nonce and seed zero
 *  100  u32 count (0 = not wrapped; 1..128 needs stored = 1)   104 u32 total (0 when count = 0)   108 u32 0
 *  112  u64[ell] moduli (first ell of Q; wrapped: of Q then P)  then u32[count] positions, zero padded to 8 bytes
 *  then the packed payload
 *
 * Key set "FHELINEP", version 1: full and compact sets, capped and uncapped keys.  Bytes 8..95 as "FHELINEK" version 1; 96 u8[32]
 * key-set seed, zero for a full set; 128 u32 halves (2 = full keys, 1 = b halves only); 132 u32 0; 136 u64[n_q + n_p] moduli; then the
 * key table with the 48-byte entries of format version 2 (max_ell = n_q marks an uncapped key and the public key); data_offset = the
 * table end rounded up to a multiple of 4096.  An entry's payload is the version 2 dense present-row payload - [digits'][halves]
 * [max_ell + n_p][N] for a switching key, [halves][n_q][N] for the public key - with every vector packed at its limb's width (present
 * row r < max_ell is Q limb r, the rows after it are the special limbs).  words counts the packed words stored; digest is the digest
 * the unpacked set carries, so a packed set's table digests equal those of the unpacked set of the same keys.
 * fhelin_evalkeys_params, _info, _interleave and _load read it beside the other two magics; _load uploads a key's packed payload,
 * unpacks it into the at-rest layout, and then expands, digests and installs as for the other formats. */
/* Writes the packed key set.  compact = 1: the preconditions and errors of fhelin_evalkeys_save_compact; compact = 0: those of
 * fhelin_evalkeys_save.  Keys are packed on the device into scratch of at most one key's payload at a time and streamed through the
 * two pinned staging buffers of the other savers.  fhelin_evalkeys_save and _save_compact write what they always wrote. */
int fhelin_evalkeys_save_packed(fhelin_ctx* c, const char* path, int32_t compact);
/* Size of the packed blob of `ct`.  seeded = 1: the seeded form; accepts exactly what fhelin_ct_export_compact accepts (wrapped
 * handles included), anything else FHELIN_ERR_STATE.  seeded = 0: the full form of any ciphertext fhelin_ct_export accepts; a wrapped
 * handle is FHELIN_ERR_ARG. */
int fhelin_ct_packed_bytes(fhelin_ctx* c, const fhelin_ct* ct, int32_t seeded, size_t* bytes);
/* Writes the blob.  Range check, digest and pack run on the device and only the packed bytes are downloaded; one synchronisation.
 * Level plan: seeded = 1 behaves as fhelin_ct_export_compact, seeded = 0 is a terminal like fhelin_ct_export. */
int fhelin_ct_export_packed(fhelin_ctx* c, const fhelin_ct* ct, int32_t seeded, uint8_t* out, size_t cap);
/* Host-only, no context: validates the header against itself and the exact size computed from the header's own moduli; any out
 * pointer may be NULL.  FHELIN_ERR_ARG on anything inconsistent. */
int fhelin_packed_info(const uint8_t* blob, size_t bytes, int32_t* log_n, int32_t* ell, int32_t* deg, int32_t* slots, int32_t* stored,
                       int32_t* count);
/* n blobs -> n handles, all or nothing.  Every header is checked against the context before anything is allocated; one batch
 * allocation per limb count; the packed payloads are uploaded and unpacked by one launch, then the strided digest and range check, then
 * every seeded c1 is expanded in one launch; one synchronisation.  stored = 1 makes exactly the handle fhelin_ct_import_compact makes
 * from the equivalent version 1 or 2 compact blob; stored >= 2 the handle fhelin_ct_import makes from the same residues, with the exact
 * 80-bit scale.  Imported values are not level-plan sources.  Works on an evaluation context. */
int fhelin_ct_import_packed(fhelin_ctx* c, const uint8_t* const* blobs, const size_t* sizes, int32_t n, fhelin_ct** outs);
/* Test hooks: the two kernels alone.  words[n_vec][N] -> the packed vectors back to back (vector i at width widths[i]); *n_words = the
 * words written (sum N widths[i] / 64), FHELIN_ERR_ARG if cap_words is smaller.  A width outside 20..60, or (pack) an input at or above
 * 2^w - checked on the host here; the format paths rely on the range check that precedes every write - is FHELIN_ERR_ARG. */
int fhelin_debug_pack(fhelin_ctx* c, const uint64_t* words, const int32_t* widths, int32_t n_vec, uint64_t* out, size_t cap_words,
                      size_t* n_words);
int fhelin_debug_unpack(fhelin_ctx* c, const uint64_t* packed, size_t n_words, const int32_t* widths, int32_t n_vec, uint64_t* out);
/* Measurement hook (tools/packed_probe.py): n_vec vectors of the given widths packed, copied device to device (the same unpacked
 * bytes), unpacked and copied again, in turn, reps times after one untimed round; ms[4 reps] = the device-event times of pack, copy,
 * unpack, copy of every round. */
int fhelin_debug_pack_rate(fhelin_ctx* c, const int32_t* widths, int32_t n_vec, int32_t reps, float* ms);

/* ---- device transport: many ciphertexts through one device buffer, no host synchronisation per ciphertext ---------------------
 * The row gather of several GPUs moves a set of ciphertexts at once.  fhelin_ct_export_device / _import_device above move one per
 * call and synchronise the host every time; the calls here write (read) n FRAMES of one device buffer - a collective's send (receive)
 * buffer - in one step and hand the ordering over to the caller's stream.
 *
 * Frames.  Frame i starts at d_buf + i * stride_bytes.  format 0 (raw): the words of fhelin_ct_export, npoly * ell * N * 8 bytes.
 * format 1 (packed): the same limb vectors in the same order, each a "Packed limb vector" (see "Packed formats") at the width of its
 * own limb's modulus: npoly * sum_{l < ell} N w_l / 8 bytes.  No header: the shape travels in `meta`.  d_buf is 16-byte aligned,
 * stride_bytes is a multiple of 16 and at least the largest frame, and n * stride_bytes <= cap_bytes.  The bytes of a frame's stride
 * beyond its payload are neither written nor read.
 *
 * Metadata (host memory).  meta[i] = {npoly, ell, deg, slots, scale_hi, scale_lo, payload_bytes, format} as doubles: the 8-double row
 * the row-sharded driver exchanges next to the payload; the scale is the 80-bit value as fhelin_ct_scale gives it.
 *
 * Stream hand-off (hip_stream, a hipStream_t of the caller's, e.g. the framework's current stream).  NULL means "no stream" here, so
 * the legacy default stream - whose own handle is NULL - is named by hipStreamLegacy ((hipStream_t)1).
 *   NULL      one host synchronisation at the end of the call (one per batch, not one per ciphertext).  The caller makes sure that
 *             whatever produced (import) or still reads (export) the buffer has finished.
 *   non-NULL  no host synchronisation.  At call time the library's stream is ordered behind everything already issued on the caller's
 *             stream (an event recorded there): the producer of the frames of an import, the last reader of the buffer of an export.
 *             After the library's last launch the caller's stream waits for an event of the library's, so work issued on that stream
 *             afterwards - a collective that sends the frames, a framework that reuses the buffer - is ordered behind the call.
 * fhelin_debug_sync_count: the host synchronisations of the context so far (the counter is incremented in the one place the library
 * synchronises a context's streams, and nowhere else); the tests prove the contract above with it. */
/* Payload bytes of every handle's frame (bytes_each[n], may be NULL) and the largest of them (max_bytes, may be NULL).  Deferred
 * handles are evaluated (one batched force).  A wrapped handle, a handle with other than 2 or 3 components, format other than 0 or 1:
 * FHELIN_ERR_ARG.  n = 0: *max_bytes = 0. */
int fhelin_ct_frame_bytes(fhelin_ctx* c, const fhelin_ct* const* cts, int32_t n, int32_t format, size_t* bytes_each, size_t* max_bytes);
/* Writes frame i from cts[i] and fills meta[i].  Deferred handles among cts are evaluated in one batched force; every handle is a
 * level-plan terminal exactly as in fhelin_ct_export_device; a wrapped handle is FHELIN_ERR_ARG.  Packed: one pack table for all
 * n * npoly * ell vectors through pinned staging and one launch of the pack kernel; raw: one device copy per frame.  Arguments are
 * checked before anything is launched (format, stride, capacity and alignment before the handles are looked at); on an error nothing
 * has been written.  n = 0 succeeds and does nothing. */
int fhelin_ct_export_device_many(fhelin_ctx* c, const fhelin_ct* const* cts, int32_t n, int32_t format, uint8_t* d_buf,
                                 size_t stride_bytes, size_t cap_bytes, double* meta, void* hip_stream);
/* n frames -> n handles, all or nothing (on any error outs is untouched).  Every meta row is validated on the host before anything is
 * allocated or launched: npoly 2 or 3, 1 <= ell <= n_q, deg 1 or 2, slots 0 (unset, as fhelin_ct_import leaves it) or a power of two up to N / 2, a finite positive scale,
 * format 0 or 1, payload_bytes equal to the size the context's own moduli give and not above the stride.  One batch allocation per
 * (npoly, ell), rows in frame order, so batched kernels downstream find the rows of a shape contiguous; one unpack launch (raw: one
 * device copy per frame).  check = 1 also runs the range check residue < modulus of the other loaders on the imported residues: it
 * costs the call's one host synchronisation (with a stream: the only one) and gives FHELIN_ERR_ARG and no handles on a violation.
 * check = 0 imports whatever the frames hold: meant for frames this library wrote in the same trust domain (the GPUs of one node).
 * Imported values are not level-plan sources, are never lowered and are never `seeded`.  n = 0 succeeds and does nothing. */
int fhelin_ct_import_device_many(fhelin_ctx* c, const uint8_t* d_buf, size_t stride_bytes, const double* meta, int32_t n, int32_t check,
                                 void* hip_stream, fhelin_ct** outs);
int fhelin_debug_sync_count(fhelin_ctx* c, uint64_t* out);
/* test hook: the device address of an evaluated handle's residues and of the batch allocation they are a view of (0: an allocation
 * of its own).  The rows an import makes for one shape are views of one block, frame order, back to back. */
int fhelin_debug_ct_addr(const fhelin_ct* ct, uint64_t* data, uint64_t* block);

#ifdef __cplusplus
}
#endif
#endif /* FHELIN_H */
