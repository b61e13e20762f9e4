// extern "C" boundary, level-capped keys (include/fhelin.h "Level-capped keys"): the cap table of a client context, what a key
// holds, and the usage recorder.  The check itself is Evaluator::bind_key (evaluator.cpp); generation is Client::make_switch_key.
#include "../../include/fhelin.h"
#include <set>
#include "capi_internal.h"

using namespace fhelin;

#define NEED(x) if (!(x)) return capi_fail(FHELIN_ERR_ARG, "null argument")

extern "C" {

int fhelin_ctx_set_key_caps(fhelin_ctx* c, const int32_t* kind, const uint64_t* galois, const int32_t* max_ell, int32_t n) {
    NEED(c && n >= 0 && ((kind && galois && max_ell) || n == 0));
    FHELIN_TRY
    Context& x = c->ctx;
    if (c->cl.eval_only()) throw Error(FHELIN_ERR_KEY, "set_key_caps: an evaluation context generates no keys");
    const u64 g_conj = 2ull * x.N - 1;
    const int n_q = x.L + 1;
    std::set<std::pair<int, u64>> seen;
    std::vector<Client::KeyCap> table;
    for (int i = 0; i < n; ++i) {
        const std::string at = "set_key_caps: entry " + std::to_string(i) + ": ";
        // kinds 4 and 5, the keys of sparse-secret bootstrapping, are known to a context with that knob on (as to fhelin_key_info): a
        // recorded table names both.  The to-sparse key is held at two limbs whatever its entry says (Client::gen_sparse_keys)
        if (kind[i] < 1 || kind[i] > (c->boot.sparse_h() ? 5 : 3))
            throw Error(FHELIN_ERR_ARG, at + "kind is 1 (relinearisation), 2 (rotation) or 3 (conjugation); with sparse-secret bootstrapping on "
                                             "also 4 (to-sparse) or 5 (from-sparse)");
        if (max_ell[i] < 1 || max_ell[i] > n_q) throw Error(FHELIN_ERR_ARG, at + "max_ell outside 1 .. n_q");
        const bool g_ok = kind[i] == 1 || kind[i] >= 4 ? galois[i] == 0 : kind[i] == 3 ? galois[i] == g_conj : (galois[i] & 1) && galois[i] > 1 && galois[i] < g_conj;
        if (!g_ok) throw Error(FHELIN_ERR_ARG, at + "the Galois element is 0 for kinds 1, 4 and 5, 2N-1 for kind 3, an odd number in (1, 2N-1) for kind 2");
        if (!seen.insert({kind[i], galois[i]}).second) throw Error(FHELIN_ERR_ARG, at + "a second entry for the same key");
        table.push_back(Client::KeyCap{kind[i], galois[i], max_ell[i]});
    }
    for (const Client::KeyCap& e : table) {
        bool held = false;
        if (e.kind == 1) held = (bool)c->ev.relin_key;
        else if (e.kind == 3) held = (bool)c->ev.conj_key;
        else if (e.kind == 4) held = (bool)c->ev.to_sparse_key;
        else if (e.kind == 5) held = (bool)c->ev.from_sparse_key;
        else {
            auto it = c->ev.rot_keys.find(e.galois);
            held = it != c->ev.rot_keys.end() && it->second;
        }
        if (held)
            throw Error(FHELIN_ERR_STATE, "set_key_caps: the context already holds the " + std::string(e.kind == 1 ? "relinearisation key" : e.kind == 3 ? "conjugation key" : e.kind == 4 ? "to-sparse key" : e.kind == 5 ? "from-sparse key" : "rotation key of Galois element " + std::to_string((unsigned long long)e.galois)) +
                                              " - caps apply to keys generated afterwards");
    }
    c->cl.set_key_caps(table);
    FHELIN_CATCH
}

int fhelin_key_info(fhelin_ctx* c, int32_t kind, int32_t index, int32_t* digits, int32_t* max_ell, int32_t* seeded) {
    NEED(c);
    FHELIN_TRY
    KeyPtr k;
    if (kind == 0) k = c->ev.relin_key;
    else if (kind == 2) k = c->ev.conj_key;
    else if (kind == 1) {
        auto it = c->ev.rot_keys.find(c->ctx.rot_element(index));
        if (it != c->ev.rot_keys.end()) k = it->second;
    } else if ((kind == 3 || kind == 4) && c->boot.sparse_h()) k = kind == 3 ? c->ev.to_sparse_key : c->ev.from_sparse_key;   // known with the knob on
    else throw Error(FHELIN_ERR_ARG, "unknown key kind");
    if (!k) throw Error(FHELIN_ERR_KEY, "key not present");
    if (digits) *digits = k->digits;
    if (max_ell) *max_ell = k->max_ell;
    if (seeded) *seeded = k->seeded ? 1 : 0;
    FHELIN_CATCH
}

int fhelin_key_usage_begin(fhelin_ctx* c) {
    NEED(c);
    FHELIN_TRY
    c->ev.usage.clear();
    c->ev.usage_on = true;
    FHELIN_CATCH
}

int fhelin_key_usage_end(fhelin_ctx* c, int32_t* kind, uint64_t* galois, int32_t* max_ell, int32_t cap, int32_t* n) {
    NEED(c && n && cap >= 0 && ((kind && galois && max_ell) || cap == 0));
    FHELIN_TRY
    if (c->ev.usage_on) {
        // what is still deferred belongs to the pass: evaluated now, on its own lane, while the recorder still listens
        struct Stop {
            Evaluator& ev;
            ~Stop() { ev.usage_on = false; }
        } stop{c->ev};
        if (c->any_pending()) flush_heavy_all(c, true);
    }
    int32_t k = 0;
    for (const auto& kv : c->ev.usage) {   // ordered by (kind, galois)
        if (k < cap) {
            kind[k] = kv.first.first;
            galois[k] = kv.first.second;
            max_ell[k] = kv.second;
        }
        ++k;
    }
    *n = k;
    FHELIN_CATCH
}

}  // extern "C"
