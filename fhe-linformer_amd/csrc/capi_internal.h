// Shared plumbing for the extern "C" translation units.
#pragma once
#include <cstring>
#include <exception>
#include <list>
#include <string>
#include <unordered_map>
#include "context.h"
#include "evaluator.h"
#include "client.h"
#include "composite.h"
#include "bootstrap.h"
#include "kernels_keys.h"
#include "wire_header.h"   // get / put: fields of the file and blob formats, at any alignment
#include "deferred.h"   // LazyRows, LazyHeavy and the forcing rules that ct_in and vec_of go through

namespace fhelin {
// Profile-guided level planning (include/fhelin.h fhelin_level_plan_*).
// The drivers are straight-line programs: which ciphertext meets which, and how many limbs each operation consumes, does
// not depend on the data.  A RECORDING pass notes, for every handle the boundary gives out, the handles the producing call
// read and the result's effective limb count (limbs minus a pending rescale).  From that the planner derives, back to
// front, the fewest limbs each value may have without any terminal (a bootstrap input, a decryption, an export) running
// short, and so by how many limbs every SOURCE - a fresh encryption, a bootstrap output - can start lower.  An APPLYING pass
// of the same program then encrypts at that level and raises bootstrap inputs to fewer limbs, so that limbs nobody would
// ever use are not carried through the key switches in between.  Sources are identified by their order in the pass.
struct LevelPlan {
    int mode = 0;  // 0 off, 1 record, 2 apply
    struct Node {
        std::vector<int> in;
        int eff = -1;       // limbs - (deg >= 2): -1 while a deferred row is unevaluated
        int ordinal = -1;   // >= 0: a source
        int need = -1;      // fewest effective limbs any consumer chain requires (-1: reaches no terminal)
    };
    std::vector<Node> nodes;
    int epoch = 0;              // recordings are numbered: a handle's node id only means something in the recording that made it
    int next_ordinal = 0;
    std::vector<int> target;    // the plan, per source ordinal: effective limbs the source should start with (-1: as asked)

    static int eff_of(const Ciphertext& c) { return c.ell - (c.deg >= 2 ? 1 : 0); }
    int add_node(const std::vector<int>& in, int eff) {
        nodes.push_back(Node{in, eff, -1, -1});
        return (int)nodes.size() - 1;
    }
    void terminal(int node, int need) {
        if (mode == 1 && node >= 0) nodes[node].need = std::max(nodes[node].need, need);
    }
    // applying: a terminal that is short of limbs means the pass is not the recorded program
    void check_terminal(const Ciphertext& c, int need) const {
        if (mode == 2 && eff_of(c) < need)
            throw Error(FHELIN_ERR_STATE, "level plan: a value reached a decryption / export with fewer limbs than it needs - this pass does not follow the recorded program");
    }
    // the next source of the pass would start with `ell` limbs: how many of them to leave out (0 unless applying)
    int next_drop(int ell) {
        const int k = next_ordinal++;
        if (mode != 2 || k >= (int)target.size() || target[k] < 1) return 0;
        return std::max(0, ell - target[k]);
    }
    void begin(int m) {
        mode = m;
        next_ordinal = 0;
        nodes.clear();
        ++epoch;
    }
    bool live(int node, int node_epoch) const { return mode == 1 && node >= 0 && node_epoch == epoch && node < (int)nodes.size(); }
    void finish();  // record mode: derive `target` from the recording (capi.cpp)
};
// handles read by the C-ABI call in progress on this thread (node ids of the recording context)
std::vector<int>& plan_inputs();
}  // namespace fhelin

// Plaintexts by CONTENT (fhelin_encode): a model's weights, biases and the drivers' masks are the same slot values in every pass, and a
// server holds one model for every sample.  The cache keeps one Plaintext per (n, slots, level hint, value bytes); every encode gives a
// handle of its own whose Plaintext::shared points at it, so that Plaintext::at takes the device encodings made by the handles of
// earlier passes and launches nothing.  Only an encoding at exactly the asked (limb count, scale) is shared - the bytes the handle would
// have made itself - so every operation reads what it read without the cache.  A hash hit is CONFIRMED against the stored values byte
// for byte (memcmp: -0.0 and NaN payloads stay distinct), as Composite::relarge_src_ does.
// Bounded: whole plaintexts go least recently used first once the encodings held exceed cap_bytes (a handle that still refers to an
// evicted plaintext keeps it alive; the cache only forgets it).  One engine per thread: no lock.  FHELIN_PT_CACHE=0: every encode makes
// a plaintext of its own; FHELIN_PT_CACHE_MB: the cap (default 1024).
namespace fhelin {
struct PtCache {
    struct Entry {
        int n = 0;          // values the caller gave
        uint64_t hash = 0;  // of the bytes of the values that count (the first min(n, slots))
        PtPtr p;            // slots, level hint and the values themselves (no imaginary part: fhelin_encode takes real vectors)
    };
    static constexpr size_t MAX_ENTRIES = 4096;   // plaintexts that were never used hold no encoding: bounded by count
    bool on = true;
    size_t cap_bytes = (size_t)1 << 30;
    std::list<Entry> lru;                         // most recently used first
    std::unordered_multimap<uint64_t, std::list<Entry>::iterator> by_hash;
    PtCache();
    PtPtr encode(Client& cl, int default_slots, const double* vals, int n, int level, int slots);
    size_t bytes_held() const;                    // device bytes of the encodings of the cached plaintexts
    void clear();
private:
    void evict_last();
};
}  // namespace fhelin
// opaque handle behind include/fhelin.h's `fhelin_ctx`
struct fhelin_ctx {
    fhelin::Context ctx;
    fhelin::Evaluator ev;
    fhelin::Client cl;
    fhelin::Composite comp;
    fhelin::Bootstrapper boot;
    bool lazy_rows = true;      // FHELIN_LAZY_ROWS
    bool lazy_heavy = true;     // FHELIN_LAZY_HEAVY
    bool boot_pairs = false;    // FHELIN_BOOT_PAIRS / fhelin_ctx_set_bootstrap_pairing: deferred single bootstraps go through Bootstrapper::bootstrap_pairs
    // deferred operations, per lane: a lane's pending operations are evaluated on that lane's stream (fhelin_ctx_set_lane)
    std::vector<std::shared_ptr<fhelin::LazyHeavy>> pending_heavy[fhelin::DevicePool::MAX_LANES];
    bool any_pending() const {
        for (const auto& v : pending_heavy)
            if (!v.empty()) return true;
        return false;
    }
    int user_lane = 0;          // fhelin_ctx_set_lane: 0 = the context's main stream
    hipEvent_t lane_mark[fhelin::DevicePool::MAX_LANES] = {};   // fhelin_ctx_lane_mark: a point in a lane's stream others can wait for
    bool lane_marked[fhelin::DevicePool::MAX_LANES] = {};
    fhelin::LevelPlan plan;
    fhelin::PtCache pt_cache;   // declared after ctx: gone before the device pool is torn down
    // the unwrap of wrapped inputs (capi_wrapped.cpp): the mask (1 in the slots = 0 mod 128) and the tables of a rescale that drops p_0
    fhelin::PtPtr wrap_mask;
    const fhelin::u64* p0_qlinv = nullptr;   // [n_q][2] p_0^-1 mod q_t, Shoup
    const fhelin::u64* p0_qlmod = nullptr;   // [n_q]    p_0 mod q_t
    explicit fhelin_ctx(const fhelin::Params& p);
};
struct fhelin_ct {
    mutable fhelin::CtPtr p;                          // null while the row is still deferred
    mutable std::shared_ptr<fhelin::LazyRows> lazy;
    mutable std::shared_ptr<fhelin::LazyHeavy> heavy;   // a deferred bootstrap / Chebyshev evaluation
    int lazy_idx = 0;
    fhelin_ctx* owner = nullptr;
    int node = -1;                                    // level-plan recording: this value's node ...
    int node_epoch = -1;                              // ... in this recording (a handle may outlive the pass that made it)
};
struct fhelin_pt {
    fhelin::PtPtr p;
};

#if !defined(__BYTE_ORDER__) || __BYTE_ORDER__ != __ORDER_LITTLE_ENDIAN__
#error "evaluation-key sets and compact ciphertexts are written in host byte order, which must be little-endian"
#endif

namespace fhelin {
int capi_fail(int code, const std::string& msg);
// the per-vector device digests h[n_vec][2] (launch_key_digest_strided: digest, range flag) of one key or one c0 folded into its digest;
// in_range: every residue below its limb's modulus
inline u64 fold_key_digest(const u64* h, size_t n_vec, bool& in_range) {
    u128 acc = 0;
    in_range = true;
    for (size_t j = 0; j < n_vec; ++j) {
        acc += (u128)h[2 * j] * key_weight_vec((u32)j);
        if (!h[2 * j + 1]) in_range = false;
    }
    return (u64)(acc % KEY_DIGEST_P);
}

// level-plan recording: the call in progress reads `h`
inline void note_input(fhelin_ctx* c, const fhelin_ct* h) {
    if (c->plan.live(h->node, h->node_epoch)) plan_inputs().push_back(h->node);
}
// a new handle for a result of the call in progress
inline fhelin_ct* wrap(fhelin_ctx* c, const CtPtr& p) {
    auto* h = new fhelin_ct;
    h->p = p;
    if (c->plan.mode == 1) {
        h->node = c->plan.add_node(plan_inputs(), LevelPlan::eff_of(*p));
        h->node_epoch = c->plan.epoch;
    }
    return h;
}
// The main stream is about to consume `h`: a deferred value is evaluated first (force); if a worker lane is still producing it, order
// the main stream behind the producing op (no host wait) and drop the holds that op needed.
inline const CtPtr& ct_in(fhelin_ctx* c, const fhelin_ct* h) {
    if (h->p && h->p->wrapped())
        throw Error(FHELIN_ERR_ARG, "a wrapped input ciphertext is accepted by fhelin_unwrap_inputs, fhelin_decrypt, fhelin_ct_info, compact "
                                    "export and free only");
    note_input(c, h);
    force(c, h);
    Ciphertext& ct = *h->p;
    if (ct.async_pending) {
        Context& x = c->ctx;
        hip_check(hipStreamWaitEvent(x.main_stream, ct.async_ev, 0), "hipStreamWaitEvent(async result)");
        ct.async_pending = false;
        x.release_holds(ct.async_lane, ct.async_seq);
    }
    return h->p;
}
// `h` is read by a terminal of the level plan (a decryption, an export: `need` effective limbs are all it reads): marked while
// recording, checked while applying, and the value itself as ct_in gives it
inline const CtPtr& terminal_in(fhelin_ctx* c, const fhelin_ct* h, int need = 2) {
    if (c->plan.live(h->node, h->node_epoch)) c->plan.terminal(h->node, need);
    const CtPtr& p = ct_in(c, h);
    c->plan.check_terminal(*p, need);
    return p;
}
// the ciphertexts behind v[0..n): no null handle, everything deferred among them evaluated together (force_many), then ct_in in index order
inline CtVec vec_of(fhelin_ctx* c, const fhelin_ct* const* v, int n) {
    for (int i = 0; i < n; ++i)
        if (!v[i]) throw Error(FHELIN_ERR_ARG, "null ciphertext handle in array");
    force_many(c, v, n);
    CtVec out;
    for (int i = 0; i < n; ++i) out.push_back(ct_in(c, v[i]));
    return out;
}
}  // namespace fhelin

#define FHELIN_TRY try { fhelin::plan_inputs().clear();
#define FHELIN_CATCH                                                          \
    return FHELIN_OK;                                                         \
    }                                                                         \
    catch (const fhelin::Error& e) { return fhelin::capi_fail(e.code, e.what()); }          \
    catch (const std::bad_alloc&) { return fhelin::capi_fail(FHELIN_ERR_INTERNAL, "host out of memory"); } \
    catch (const std::exception& e) { return fhelin::capi_fail(FHELIN_ERR_INTERNAL, e.what()); }
