// Engine context: CKKS parameter set -> prime chain -> host/device tables, HIP stream, device pool.
// Mirrors what reference FHEController::generate_context builds through OpenFHE's GenCryptoContext
// (reference src/FHEController.cpp:3-49): ring dimension, 55/52-bit Q chain, HYBRID key switching with
// dnum large digits and 60-bit special primes, SPARSE_TERNARY secret, FLEXIBLEAUTO real scaling factors.
#pragma once
#include <cstdint>
#include <map>
#include <memory>
#include <stdexcept>
#include <string>
#include <unordered_map>
#include <vector>
#include <hip/hip_runtime_api.h>
#include "../../include/fhelin.h"  // status codes
#include "hostmath.h"
#include "pool.h"
#include "kernels_elem.h"

namespace fhelin {

struct Params {
    int log_n = 16;
    int n_q = 24;          // L+1 Q limbs
    int first_bits = 55;
    int scale_bits = 52;
    int n_p = 6;           // special limbs k
    int special_bits = 60;
    int dnum = 4;
    int log_slots = 14;
    int hamming = 192;     // sparse ternary secret weight
    // secret seed of the client-side generator (client.h Prng).  seed == 0: 32 bytes of OS entropy (getrandom) — the
    // default and the only secure choice; seed != 0: a deterministic 64-bit TEST seed (tests, reproducible benchmarks);
    // seed_bytes set explicitly (have_seed_bytes): a stored 256-bit seed (load_context regenerating a client's keys)
    uint64_t seed = 0;
    uint8_t seed_bytes[32] = {};
    bool have_seed_bytes = false;
    int device = 0;        // < 0: host-only context (parameter tables only; every device op fails)
};

// Per-level constants of hybrid key switching / rescale, resident on the device.
struct LevelTables {
    int ell = 0;        // live Q limbs
    int beta = 0;       // digits present at this level
    // ModUp: per source limb i < ell: (Qhat_i^{-1} mod q_i, shoup); and [ell][ell+k] Qhat_i mod t
    const u64* up_hatinv = nullptr;   // [ell][2]
    const u64* up_hatmod = nullptr;   // [ell][ell+k]  (Q_j/q_i) mod m_t times 2^64 (the conversion ends in redc128), pre-split (pack30)
    const u64* up_hatmod_r2 = nullptr;   // the same times 2^128: digits that come out times 2^64, for the inner product over the keys as they are
                                         // stored (ks_inner: it ends in redc128 too and has no scaled key copy to read)
    const int* ext_limb_tab = nullptr;  // [beta*(ell+k)] limb id for the NTT after ModUp, -1 on own-digit slots
    const int* key_limb_tab = nullptr;  // [ell+k] limb ids q_0..q_{ell-1}, p_0..p_{k-1}: the rows of a limb-sliced plaintext encoding
    // ModDown and rescale as ONE basis conversion (kernels_elem.h launch_moddown_rescale_conv; ell >= 2): the dropped basis is
    // B = (p_0..p_{k-1}, q_{ell-1}) with product M = P q_{ell-1}
    const u64* md_hatinv = nullptr;   // [k+1][2]      (M/b)^{-1} mod b, shoup
    const u64* md_hatmod = nullptr;   // [k+1][ell-1]  (M/b) mod q_t, pre-split (pack30)
    const u64* md_minv = nullptr;     // [ell-1][2]    M^{-1} mod q_t, shoup
    const u64* md_mmod = nullptr;     // [ell-1]       M mod q_t (the centred conversion takes one off per source above b/2)
    const int* mdx_limb_tab = nullptr;   // [k+1] limb ids p_0..p_{k-1}, q_{ell-1}: the inverse transform of the exact merged tail (Evaluator::moddown_rescale_exact)
};

// host-side operation counters (bench.py scales the CPU baseline sample with these)
struct OpStats {
    u64 limb_ntt = 0;      // limb vectors transformed (forward + inverse)
    u64 keyswitch = 0;     // hybrid key switches (rotations + relinearisations)
    u64 keyswitch_limbs = 0;  // sum of live Q limbs over those key switches
    u64 rescale = 0;
    u64 ct_pt_mult = 0;
    u64 bootstrap = 0;
    u64 encode = 0;
    u64 rescale_limbs = 0;    // sum of live Q limbs (before the drop) over those rescales
    u64 ct_pt_limbs = 0;      // sum of live Q limbs over those products
};

struct Context {
    Params prm;
    OpStats stats;
    int N = 0;
    int L = 0;       // n_q - 1
    int K = 0;       // n_p
    int alpha = 0;   // limbs per digit
    PrimeChain chain;
    std::vector<u64> moduli;          // Q then P
    std::vector<Barrett> barrett;     // same order
    std::vector<TwiddleTable> tw;     // same order (host copies)
    std::vector<long double> sf_real; // FLEXIBLEAUTO real scaling factor per level (0 = fresh)

    bool has_device = false;
    hipStream_t stream = nullptr;   // the CURRENT stream: main stream, or a lane's stream inside a LaneScope
    hipStream_t main_stream = nullptr;
    bool own_stream = false;
    // worker lanes: independent chunks of a batched op (rows of a matmul) run on different streams so that the
    // VALU-bound NTT passes of one chunk overlap the bandwidth-bound conversion / inner-product kernels of another
    int n_lanes = 0;
    hipStream_t lane_stream[DevicePool::MAX_LANES] = {};
    hipEvent_t lane_event[DevicePool::MAX_LANES] = {};
    hipEvent_t fork_event = nullptr;
    // Heavy single-ciphertext ops (bootstrap, polynomial evaluation) issued back to back by the caller run on
    // alternating lanes WITHOUT joining: the result carries an event, the main stream waits for it only when the result
    // is consumed.  An op's input is kept alive until the main stream has passed the op's event (lane_hold).
    bool async_lanes = true;        // FHELIN_ASYNC=0 disables
    int async_rr = 0;
    u64 lane_seq[DevicePool::MAX_LANES] = {};
    std::vector<std::pair<u64, std::shared_ptr<void>>> lane_hold[DevicePool::MAX_LANES];
    void release_holds(int lane, u64 up_to_seq);
    void fork_lanes();              // lanes wait for everything enqueued on the main stream so far
    void join_lanes();              // the main stream waits for every lane
    DevicePool pool;
    hipStream_t stream_of(int lane) const { return pool.lane_stream[lane]; }   // lane 0: the main stream
    void select_lane(int lane) {    // launches and allocations go to `lane` from here on
        stream = stream_of(lane);
        pool.cur_lane = lane;
    }
    void set_main_stream(hipStream_t s) {   // lane 0 moves to a stream of the caller's
        stream = main_stream = pool.lane_stream[0] = s;
        own_stream = false;
    }
    struct LaneScope {              // lane k until destruction, then back to the stream and lane it was entered from
        Context& c;
        hipStream_t was_stream;
        int was_lane;
        LaneScope(Context& ctx, int k) : c(ctx), was_stream(ctx.stream), was_lane(ctx.pool.cur_lane) { c.select_lane(k); }
        ~LaneScope() {
            c.stream = was_stream;
            c.pool.cur_lane = was_lane;
        }
    };
    DeviceTables dt{};
    std::vector<void*> table_allocs;
    hipEvent_t ev_start = nullptr, ev_stop = nullptr;

    // Pinned staging ring for host->device uploads on the hot path (plaintext encodings, encryption randomness):
    // the copy is queued on the current stream and the host does NOT wait for the stream to drain.  A slot is reused
    // only after the event recorded behind its copy has completed.
    static constexpr int STAGE_SLOTS = 64;   // 64 x 2N words pinned (64 MiB at N=2^16): with 8 the host ran at most eight plaintext encodings ahead of the GPU
    u64* stage_buf[STAGE_SLOTS] = {};
    hipEvent_t stage_ev[STAGE_SLOTS] = {};
    bool stage_used[STAGE_SLOTS] = {};
    int stage_next = 0;
    size_t stage_words = 0;
    // small payloads (the scalar tables of a linear combination: a few KB, hundreds per pass) have a ring of their own with MANY slots:
    // with the eight large slots alone the host could run at most eight uploads ahead of the GPU - harmless on one stream, but a host
    // that waits for lane 1's old upload cannot feed lane 2 (fhelin_ctx_set_lane)
    static constexpr int SMALL_SLOTS = 256;
    static constexpr size_t SMALL_WORDS = 8192;      // 64 KiB
    u64* small_buf = nullptr;                        // SMALL_SLOTS x SMALL_WORDS, pinned
    hipEvent_t small_ev[SMALL_SLOTS] = {};
    bool small_used[SMALL_SLOTS] = {};
    int small_next = 0;
    void upload_async(u64* dst, const u64* src, size_t words);  // words <= 2N

    // ModDown / rescale constants (level independent)
    const u64* d_phatinv = nullptr;  // [k][2]   (P/p)^{-1} mod p, shoup
    const u64* d_phatmod = nullptr;  // [k][L+1] (P/p) mod q_t
    const u64* d_pinv = nullptr;     // [L+1][2] P^{-1} mod q_t, shoup
    const u64* d_pmod = nullptr;     // [L+1][2] P mod q_t, shoup
    const u64* d_qlinv = nullptr;    // [L+1][L+1][2]  q_l^{-1} mod q_t, shoup   (row l, col t<l)
    const u64* d_qlmod = nullptr;    // [L+1][L+1]     q_l mod q_t
    std::vector<LevelTables> lvl;    // index by ell (1..L+1)
    std::map<u64, const u32*> automorph_maps;  // galois element -> device map [N]

    explicit Context(const Params& p);
    ~Context();
    Context(const Context&) = delete;
    Context& operator=(const Context&) = delete;

    void require_device() const;
    template <class T> T* dalloc(size_t count) { return static_cast<T*>(pool.alloc(count * sizeof(T))); }   // for blocks with an owner of their own
    template <class T> Scratch<T> scratch(size_t count) { return Scratch<T>(pool, count); }
    template <class T> const T* upload_table(const std::vector<T>& v);
    int limb_id_q(int i) const { return i; }
    int limb_id_p(int j) const { return L + 1 + j; }
    int digits_at(int ell) const { return (ell + alpha - 1) / alpha; }
    u64 galois_element(long rot_index) const;      // 5^r mod 2N (r may be negative): a rotation of the PHYSICAL slot vector
    // Interleaved samples (include/fhelin.h "Interleaved samples"): `stride` sample vectors of n logical slots share the n * stride
    // physical slots of a packing, sample i in the slots = i mod stride.  Every rotation index the evaluator, the composites and the
    // C ABI take is LOGICAL and goes through rot_element: a physical rotation by stride * r rotates every sample by r.  Bootstrapping
    // works on the physical packing and is the one caller that bypasses the mapping (PhysicalScope).  stride == 1: nothing changes.
    int stride = 1;
    bool stride_explicit = false;   // set by fhelin_ctx_set_interleave (an evaluation-key set of another stride is then refused)
    bool stride_locked = false;     // a key, plaintext, ciphertext or bootstrap set-up exists: the stride can no longer change
    u64 rot_element(int rot_index) const { return stride == 1 ? galois_element(rot_index) : galois_element((long)stride * rot_index); }
    struct PhysicalScope {          // host-side: indices and slot counts are physical until destruction
        Context& c;
        int was;
        explicit PhysicalScope(Context& ctx) : c(ctx), was(ctx.stride) { c.stride = 1; }
        ~PhysicalScope() { c.stride = was; }
    };
    const u32* automorph_map(u64 galois);          // device map for the NTT-domain permutation
    const u32* automorph_inverse_of(const u32* map);  // the map of the inverse automorphism (built together with `map`)
    std::map<const u32*, const u32*> automorph_inverse;
    u32 automorph_ginv_of(const u32* map) const;      // g^-1 mod 2N of the map's Galois element g (KsShape::ginv)
    std::map<const u32*, u32> automorph_ginv;
    // Row-pass epilogues (kernels.h NttEpilogue): the forward NTT that feeds a rescale, a merged ModDown + rescale or a ModDown
    // finishes it in registers instead of storing the transform for a separate streaming kernel.  Bit-identical either way.
    // FHELIN_FUSE_FINISH=0: the separate kernels (rescale_finish, moddown_rescale_finish, moddown_finish) everywhere (A/B).
    bool fuse_finish = true;
    // FHELIN_FUSE_MODDOWN=1: also the ModDown of a ROTATION (output through the inverse automorphism map: scattered stores)
    // rides in the row pass.  Off: measured slower.
    bool fuse_moddown = false;
    // FHELIN_HOST_ENCODE=1 / fhelin_ctx_set_host_encode: the special FFT of CKKS encoding on the host (the original path, kept
    // as the reference the device encoder is compared with bit for bit); default: on the GPU (kernels_client.hip)
    bool host_encode = false;
    // FHELIN_DEVICE_DECODE=1 / fhelin_ctx_set_device_decode: fhelin_decrypt, _flooded and _interleaved run as batches of one through
    // Client::decrypt_batch (lift, division and forward special FFT on the device, the same doubles bit for bit); default: the host decoder
    bool device_decode = false;
    // Rotations gather at the inner product, so that every ModDown is the identity one that the row pass of NTT(conv) finishes
    // (needs fuse_finish).  A merged rotation sum: launch_ks_inner_multi adds P * sum_r sigma_r(c0) to the
    // accumulator's Q part while it has the maps in hand.  A plain rotation: launch_ks_inner reads digits, own limb and c0 through
    // the map and the key's permuted copy (EvalKey::d_perm), launch_moddown_conv converts with the signs of sigma_g (KsShape::gather).
    // FHELIN_ROT_GATHER=0: both end in moddown_finish_kernel, which gathers (A/B).  Bit-identical either way.
    bool rot_gather = true;
    bool fuse_lift = true;      // rescale: centred lift formed in the NTT's first-pass load (FHELIN_FUSE_LIFT)
    // FHELIN_FUSE_ACCP_ROWS: 1 - the special-limb half of a single-key inner product (relinearisation, plain and per-row
    // rotations; at most 8 digits) is formed in the load stage of the inverse NTT's row pass (kernels_elem.h NttProduct), the inner-product
    // launch covers the Q limbs only and the ModDown starts at the column pass; 2 - the merged rotation sums too (measured slower: their
    // inner product shares key words between row pairs and stages digit tiles in LDS, which the row pass does not); 0 - the separate
    // launches everywhere.  Bit-identical every way.  FHELIN_ACCP_ROWS_MIN_VECS=<n>: only accumulators of at least n special-limb vectors
    int fuse_accp_rows = 1;
    int accp_rows_min_vecs = 0;
    // FHELIN_FUSE_ACCQ_ROWS: 1 - the Q-limb half of the same single-key inner products, where the ModDown ends in the row pass
    // of NTT(conv), is formed by that row pass (launch_ntt_epilogue_product): no inner-product launch, no accQ; only the classes that
    // tools/accq_rows_probe.py shows faster (Evaluator::accq_in_rows); 2 - every single-key class that is built; 0 - launch_ks_inner and the
    // accQ round trip everywhere.  Needs the special-limb half in its row pass (fuse_accp_rows).  Bit-identical every way.
    // FHELIN_ACCQ_ROWS_MIN_VECS=<n>: with 1, only accumulators of at least n Q-limb vectors
    int fuse_accq_rows = 1;
    int accq_rows_min_vecs = 0;
    bool lds_digits = true;     // merged rotate-and-sum: digit tiles staged once in LDS when every rotation keeps tiles in place (FHELIN_LDS_DIGITS)
    struct FftDev {
        const u32* rot = nullptr;     // [slots]      5^j mod 4 slots
        const double* ksi = nullptr;  // [4 slots + 1][2]
    };
    std::map<int, FftDev> fft_dev;    // by slot count
    void sync();
    u64 sync_count = 0;             // host synchronisations so far: counted in sync() and nowhere else (fhelin_debug_sync_count)
    hipEvent_t transport_ev = nullptr;   // stream hand-off of the device transport (capi_transport.cpp); made on first use
    // K1 launch + accounting (active = vectors actually transformed, for tables with skipped entries)
    void ntt(const LimbBatch& b, bool inverse, int active = -1) {
        stats.limb_ntt += (u64)(active >= 0 ? active : b.nvec);
        if (trace_small_ntt && b.nvec <= trace_small_ntt) note_small_ntt(b.nvec);
        launch_ntt(dt, b, inverse, stream);
    }
    // FHELIN_NTT_TRACE=<n>: transforms of at most n limb vectors (launches that cannot fill the GPU) are counted by call stack and the
    // table is printed when the context goes away (a development aid: which caller still issues single-ciphertext launches)
    // FHELIN_HOST_WAITS=1: host time spent blocked inside the library, by site (printed when the context goes away)
    bool trace_waits = false;
    std::map<std::string, std::pair<u64, u64>> wait_sites;   // site -> (calls that waited, nanoseconds)
    void note_wait(const char* site, u64 ns) {
        auto& e = wait_sites[site];
        e.first += 1;
        e.second += ns;
    }
    int trace_small_ntt = 0;
    std::map<std::string, std::pair<u64, u64>> small_ntt_sites;   // call stack -> (launches, limb vectors)
    void note_small_ntt(int nvec);
    int trace_scalar = 0;                                         // FHELIN_SCALAR_TRACE=1: the same table for the launches of ew_scalar_kernel
    std::map<std::string, std::pair<u64, u64>> scalar_sites;
    void note_scalar(int nvec);
    void ntt_epilogue(const LimbBatch& b, const NttEpilogue& ep) {
        stats.limb_ntt += (u64)b.nvec;
        if (trace_small_ntt && b.nvec <= trace_small_ntt) note_small_ntt(b.nvec);
        launch_ntt_epilogue(dt, b, ep, stream);
    }
    void ntt_epilogue_product(const LimbBatch& b, const NttEpilogue& ep, const NttProduct& p) {
        stats.limb_ntt += (u64)b.nvec;
        if (trace_small_ntt && b.nvec <= trace_small_ntt) note_small_ntt(b.nvec);
        launch_ntt_epilogue_product(dt, b, ep, p, stream);
    }
};

}  // namespace fhelin
