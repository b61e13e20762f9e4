// Deferred evaluation behind the C boundary (deferred.h): deferred rows, deferred heavy operations, forcing, lane hand-over.
#include "../../include/fhelin.h"
#include <algorithm>
#include "capi_internal.h"

namespace fhelin {
void emit_lazy(fhelin_ctx* c, const std::shared_ptr<LazyRows>& g, int n, fhelin_ct** outs) {
    g->done.assign(n, CtPtr());
    for (int i = 0; i < n; ++i) {
        auto* h = new fhelin_ct;
        h->lazy = g;
        h->lazy_idx = i;
        h->owner = c;
        if (c->plan.mode == 1) {
            h->node = c->plan.add_node(plan_inputs(), -1);   // level known once the row is evaluated (force_rows)
            h->node_epoch = g->node_epoch = c->plan.epoch;
            g->node.push_back(h->node);
        }
        outs[i] = h;
    }
}
// Evaluate the listed rows of several deferred groups.  Groups that are the SAME call on different inputs (one driver call per
// sample of a batch: same weights / same row list) are evaluated TOGETHER - their rows share the batched key switches - and every
// row still holds the residues its own group's evaluation gives (rows are independent).
void force_rows_multi(fhelin_ctx* c, LazyGroups& reqs) {
    struct Todo { LazyRows* g; std::vector<int> rows; };
    std::vector<Todo> todo;
    for (auto& e : reqs) {
        Todo t{e.first, {}};
        for (int i : e.second)
            if (!t.g->done[i] && std::find(t.rows.begin(), t.rows.end(), i) == t.rows.end()) t.rows.push_back(i);
        if (!t.rows.empty()) todo.push_back(t);
    }
    std::vector<char> taken(todo.size(), 0);
    for (size_t first = 0; first < todo.size(); ++first) {
        if (taken[first]) continue;
        const LazyRows& f = *todo[first].g;
        std::vector<size_t> grp;
        for (size_t k = first; k < todo.size(); ++k) {
            if (taken[k]) continue;
            const LazyRows& g = *todo[k].g;
            bool same = g.kind == f.kind;
            if (same && g.kind == LazyRows::MatmulPt) same = g.w == f.w && g.bias == f.bias && g.slots == f.slots && g.padding == f.padding;
            if (same && g.kind == LazyRows::RElarge) same = g.weights == f.weights && g.bias == f.bias && g.mask_val == f.mask_val;
            if (same && g.kind == LazyRows::UnwrapExpanded) same = g.n == f.n && todo[k].rows == todo[first].rows;
            if (same) {
                grp.push_back(k);
                taken[k] = 1;
            }
        }
        std::vector<CtVec> res(grp.size());
        if (f.kind == LazyRows::UnwrapExpanded) {
            CtVec srcs;
            for (size_t k : grp) srcs.push_back(todo[k].g->src);
            res = c->comp.unwrapExpanded_rows_multi(srcs, f.n, todo[first].rows);
        } else {
            CtVec sub;
            for (size_t k : grp)
                for (int i : todo[k].rows) sub.push_back(todo[k].g->rows[i]);
            const CtVec r = f.kind == LazyRows::MatmulPt ? c->comp.matmul_pt(sub, f.w, f.bias, f.slots, f.padding)
                                                          : c->comp.matmulRElarge(sub, f.weights, f.bias, f.mask_val);
            size_t p = 0;
            for (size_t j = 0; j < grp.size(); ++j) {
                const size_t cnt = todo[grp[j]].rows.size();
                res[j].assign(r.begin() + p, r.begin() + p + cnt);
                p += cnt;
            }
        }
        for (size_t j = 0; j < grp.size(); ++j) {
            LazyRows& g = *todo[grp[j]].g;
            const std::vector<int>& rows = todo[grp[j]].rows;
            for (size_t k = 0; k < rows.size(); ++k) {
                g.done[rows[k]] = res[j][k];
                if (!g.node.empty() && c->plan.live(g.node[rows[k]], g.node_epoch)) c->plan.nodes[g.node[rows[k]]].eff = LevelPlan::eff_of(*res[j][k]);
            }
            bool all = true;
            for (const CtPtr& d : g.done) all = all && d;
            if (all) {  // nothing left to evaluate: release the inputs
                g.rows.clear();
                g.src.reset();
            }
        }
    }
}
void force_rows(fhelin_ctx* c, LazyRows& g, const std::vector<int>& idx) {
    LazyGroups one{{&g, idx}};
    force_rows_multi(c, one);
}
// A consumer asks for rows `idx` of a deferred group: which rows to evaluate now.  The first partial read evaluates just those rows
// (a driver that uses Q[0] only); a second one means the driver is walking over the rows: everything that is left is evaluated in
// one batched call instead of row by row.
std::vector<int> rows_for_read(LazyRows& g, const std::vector<int>& idx) {
    std::vector<int> rest;
    for (int i = 0; i < (int)g.done.size(); ++i)
        if (!g.done[i]) rest.push_back(i);
    bool wanted = false, partial = false;
    for (int i : idx) wanted |= !g.done[i];
    if (!wanted) return {};
    for (int i : rest) partial |= std::find(idx.begin(), idx.end(), i) == idx.end();
    if (partial && g.partial_reads++ == 0) return idx;
    return rest;
}
void force_group(fhelin_ctx* c, LazyRows& g, const std::vector<int>& idx) { force_rows(c, g, rows_for_read(g, idx)); }

LazyGroups lazy_groups(fhelin_ctx* c, const fhelin_ct* const* v, int n, bool strict_null) {
    LazyGroups groups;
    for (int i = 0; i < n; ++i) {
        const fhelin_ct* h = v[i];
        if (!h && strict_null) throw Error(FHELIN_ERR_ARG, "null ciphertext handle in array");
        if (!h) continue;
        if (!h->p && h->heavy) force(c, h);      // the first one evaluates everything pending
        if (h->p || !h->lazy) continue;
        LazyRows* g = h->lazy.get();
        auto it = std::find_if(groups.begin(), groups.end(), [&](const auto& e) { return e.first == g; });
        if (it == groups.end()) it = groups.insert(groups.end(), {g, {}});
        if (std::find(it->second.begin(), it->second.end(), h->lazy_idx) == it->second.end()) it->second.push_back(h->lazy_idx);
    }
    return groups;
}
void force_many(fhelin_ctx* c, const fhelin_ct* const* v, int n) {
    LazyGroups groups = lazy_groups(c, v, n, false);
    // per group the rows its read pattern asks for (force_group's rule), then ONE merged evaluation over the groups
    for (auto& e : groups) e.second = rows_for_read(*e.first, e.second);
    force_rows_multi(c, groups);
}

// Deferred heavy operations: everything pending, in dependency order; per round the ready operations of one kind, one
// parameter set and one input shape go through ONE batched call.
// A batched call that throws fails ONLY its own group (and, transitively, the operations that read its results); every other ready
// group is still evaluated.  The failure stays with the operation: reading its handle reports it (force), fhelin_sync reports the
// first one of the flush; reading an unrelated result succeeds.
static void finish(LazyHeavy& h) {   // over, with a result or a failure: nothing it read is held any longer
    h.done = true;
    h.in.reset();
    h.in_heavy.reset();
    h.in2.reset();
    h.in2_heavy.reset();
}
static void complete(LazyHeavy& h, const CtPtr& result) {
    h.result = result;
    finish(h);
}
static void fail_op(LazyHeavy& h, int code, const std::string& msg) {
    h.failed = true;
    h.err_code = code;
    h.err_msg = msg;
    finish(h);
}
void flush_heavy(fhelin_ctx* c, bool report) {
    std::vector<std::shared_ptr<LazyHeavy>> pend;
    pend.swap(c->pending_heavy[c->ctx.pool.cur_lane]);
    int first_code = 0;
    std::string first_msg;
    auto note_failure = [&](int code, const std::string& msg) {
        if (!first_code) {
            first_code = code;
            first_msg = msg;
        }
    };
    // run one batched call over `grp` and hand every operation its result; a throw fails exactly these operations
    auto guarded = [&](const std::vector<LazyHeavy*>& grp, auto&& run) {
        try {
            const CtVec out = run();
            for (size_t k = 0; k < grp.size(); ++k) complete(*grp[k], out[k]);
        } catch (const Error& e) {
            for (LazyHeavy* g : grp) fail_op(*g, e.code, e.what());
            note_failure(e.code, e.what());
        } catch (const std::exception& e) {
            for (LazyHeavy* g : grp) fail_op(*g, FHELIN_ERR_INTERNAL, e.what());
            note_failure(FHELIN_ERR_INTERNAL, e.what());
        }
    };
    for (;;) {
        std::vector<LazyHeavy*> ready;
        bool waiting = false;
        for (auto& sp : pend) {
            LazyHeavy& h = *sp;
            if (h.done) continue;
            if (sp.use_count() == 1) {   // every handle to the result is gone and nothing pending reads it: never evaluated
                fail_op(h, FHELIN_ERR_STATE, "never evaluated: no handle to the result was left");
                continue;
            }
            bool dep_failed = false;
            std::string why;
            for (auto* dep : {&h.in_heavy, &h.in2_heavy})
                if (*dep && (*dep)->done) {
                    if ((*dep)->failed || !(*dep)->result) {
                        dep_failed = true;
                        why = (*dep)->err_msg;
                    } else {
                        (dep == &h.in_heavy ? h.in : h.in2) = (*dep)->result;
                        dep->reset();
                    }
                }
            if (dep_failed) {
                fail_op(h, FHELIN_ERR_STATE, "a deferred operation this one reads failed earlier: " + why);
                continue;
            }
            if (h.in && (h.kind != LazyHeavy::Add || h.in2)) ready.push_back(&h);
            else waiting = true;
        }
        if (ready.empty()) {
            if (waiting) {   // cannot happen (an operation only ever reads earlier ones); fail what is left rather than spin
                for (auto& sp : pend)
                    if (!sp->done) fail_op(*sp, FHELIN_ERR_INTERNAL, "deferred heavy operations: dependency cycle");
                note_failure(FHELIN_ERR_INTERNAL, "deferred heavy operations: dependency cycle");
            }
            break;
        }
        std::vector<char> taken(ready.size(), 0);
        {   // every ready addition of the round in ONE batched call (Evaluator::add_batch aligns levels per group of rows); additions whose
            // operands cannot be added (component counts differ) fail on their own, before the batch
            CtVec as, bs;
            std::vector<LazyHeavy*> adds;
            for (size_t k = 0; k < ready.size(); ++k)
                if (ready[k]->kind == LazyHeavy::Add) {
                    taken[k] = 1;
                    if (ready[k]->in->npoly != ready[k]->in2->npoly) {
                        fail_op(*ready[k], FHELIN_ERR_STATE, "add: component count mismatch");
                        note_failure(FHELIN_ERR_STATE, "add: component count mismatch");
                        continue;
                    }
                    adds.push_back(ready[k]);
                    as.push_back(ready[k]->in);
                    bs.push_back(ready[k]->in2);
                }
            if (!adds.empty()) guarded(adds, [&] { return adds.size() == 1 ? CtVec{c->ev.add(as[0], bs[0])} : c->ev.add_batch(as, bs); });
        }
        for (size_t first = 0; first < ready.size(); ++first) {
            if (taken[first]) continue;
            LazyHeavy& f = *ready[first];
            // pairing on: the single bootstraps of one planned drop that are ready together share ONE paired pipeline, in call order,
            // whatever their limbs and degree (the pipeline reads two limbs of each)
            const bool paired = c->boot_pairs && f.kind == LazyHeavy::Boot && f.precision == 0;
            std::vector<LazyHeavy*> grp;
            for (size_t k = first; k < ready.size(); ++k) {
                LazyHeavy& g = *ready[k];
                const bool same = !taken[k] && g.kind == f.kind && (paired || (g.in->ell == f.in->ell && g.in->deg == f.in->deg)) &&
                                  g.in->npoly == f.in->npoly &&
                                  (f.kind == LazyHeavy::Boot ? g.drop == f.drop && g.precision == f.precision : (g.a == f.a && g.b == f.b && g.coeffs == f.coeffs));
                if (same) {
                    grp.push_back(&g);
                    taken[k] = 1;
                }
            }
            guarded(grp, [&] {
                CtVec in;
                for (LazyHeavy* g : grp) in.push_back(g->in);
                return f.kind != LazyHeavy::Boot ? c->ev.eval_chebyshev_many(in, f.coeffs, f.a, f.b)
                       : f.precision > 0         ? c->boot.bootstrap_iter_batch(in, f.precision, f.drop)
                       : paired                  ? c->boot.bootstrap_pairs(in, f.drop)
                                                 : c->boot.bootstrap_batch(in, f.drop);
            });
        }
    }
    if (report && first_code) throw Error(first_code, "a deferred operation failed: " + first_msg);
}
void flush_lane(fhelin_ctx* c, int k, bool report) {
    Context::LaneScope scope(c->ctx, k);
    flush_heavy(c, report);
}
void flush_heavy_all(fhelin_ctx* c, bool report) {
    int code = 0;
    std::string msg;
    for (int k = 0; k < DevicePool::MAX_LANES; ++k) {
        if (c->pending_heavy[k].empty()) continue;
        try {
            flush_lane(c, k, report);
        } catch (const Error& e) {
            if (!code) {
                code = e.code;
                msg = e.what();
            }
        }
    }
    if (code) throw Error(code, msg);
}
void wait_for_lane(fhelin_ctx* c, int lane) {
    Context& x = c->ctx;
    if (lane == x.pool.cur_lane) return;
    hip_check(hipEventRecord(x.fork_event, x.stream_of(lane)), "hipEventRecord(lane hand-over)");
    hip_check(hipStreamWaitEvent(x.stream, x.fork_event, 0), "hipStreamWaitEvent(lane hand-over)");
}
void force(fhelin_ctx* c, const fhelin_ct* h) {
    if (!h->p && h->heavy) {
        LazyHeavy& op = *h->heavy;
        if (!op.done) {
            if (op.lane == c->ctx.pool.cur_lane) {
                flush_heavy(c);
            } else {                 // issued under another lane: evaluated there, then this lane's stream goes behind it
                flush_lane(c, op.lane);
                wait_for_lane(c, op.lane);
            }
        }
        if (op.failed || !op.result)
            throw Error(op.err_code ? op.err_code : FHELIN_ERR_STATE, "deferred operation failed: " + (op.err_msg.empty() ? std::string("no result") : op.err_msg));
        h->p = op.result;
        h->heavy.reset();
        return;
    }
    if (h->p || !h->lazy) return;
    LazyRows& g = *h->lazy;
    if (!g.done[h->lazy_idx]) force_group(c, g, std::vector<int>{h->lazy_idx});
    h->p = g.done[h->lazy_idx];
    h->lazy.reset();
}

bool defer_allowed(fhelin_ctx* c) {
    return c->lazy_heavy && c->plan.mode != 1 && c->ctx.pool.cur_lane == c->user_lane && c->ctx.stream == c->ctx.stream_of(c->user_lane);
}
// one operand of a deferred operation: the unfinished deferred operation that will produce it (a dependency), or the ciphertext itself
static void take_operand(fhelin_ctx* c, const fhelin_ct* h, CtPtr& in, std::shared_ptr<LazyHeavy>& dep) {
    if (!h->p && h->heavy && !h->heavy->done) dep = h->heavy;
    else in = ct_in(c, h);
}
// `op` joins the current lane's pending operations; the handle to its result
static fhelin_ct* pending_handle(fhelin_ctx* c, const std::shared_ptr<LazyHeavy>& op) {
    op->lane = c->ctx.pool.cur_lane;
    c->pending_heavy[op->lane].push_back(op);
    auto* h = new fhelin_ct;
    h->heavy = op;
    h->owner = c;
    return h;
}
fhelin_ct* defer_heavy(fhelin_ctx* c, const fhelin_ct* a, const std::shared_ptr<LazyHeavy>& op) {
    take_operand(c, a, op->in, op->in_heavy);
    if (op->in) {   // what can be checked now is checked now: the offending call reports it, not a later read
        if (op->in->npoly != 2) throw Error(FHELIN_ERR_STATE, "bootstrap / polynomial evaluation: the ciphertext must have 2 components (relinearise first)");
        if (op->kind == LazyHeavy::Cheb && op->in->ell - (op->in->deg >= 2 ? 1 : 0) < 2)
            throw Error(FHELIN_ERR_STATE, "polynomial evaluation: no limb left for a multiplication");
    }
    return pending_handle(c, op);
}
fhelin_ct* defer_add(fhelin_ctx* c, const fhelin_ct* a, const fhelin_ct* b) {
    auto op = std::make_shared<LazyHeavy>();
    op->kind = LazyHeavy::Add;
    take_operand(c, a, op->in, op->in_heavy);
    take_operand(c, b, op->in2, op->in2_heavy);
    if (op->in && op->in2 && op->in->npoly != op->in2->npoly) throw Error(FHELIN_ERR_STATE, "add: component count mismatch");
    return pending_handle(c, op);
}

CtPtr run_heavy(fhelin_ctx* c, const fhelin_ct* in, const std::function<CtPtr(const CtPtr&)>& f) {
    Context& x = c->ctx;
    note_input(c, in);
    force(c, in);               // a deferred input is evaluated on the main stream, before the lane is entered
    if (x.n_lanes < 2 || !x.async_lanes || x.stream != x.main_stream) return f(ct_in(c, in));
    Ciphertext& ci = *in->p;
    const int k = ci.async_pending ? ci.async_lane : 1 + (x.async_rr++ % x.n_lanes);
    // the lane starts behind everything the main stream has been given so far: the op's input, and every earlier
    // consumer of blocks that this lane's pool may hand out again
    hip_check(hipEventRecord(x.fork_event, x.main_stream), "hipEventRecord(async fork)");
    hip_check(hipStreamWaitEvent(x.stream_of(k), x.fork_event, 0), "hipStreamWaitEvent(async fork)");
    CtPtr out;
    {
        Context::LaneScope scope(x, k);
        out = f(in->p);
    }
    const u64 seq = ++x.lane_seq[k];
    if (!out->async_ev) hip_check(hipEventCreateWithFlags(&out->async_ev, hipEventDisableTiming), "hipEventCreate(async)");
    hip_check(hipEventRecord(out->async_ev, x.stream_of(k)), "hipEventRecord(async)");
    out->async_pending = true;
    out->async_lane = k;
    out->async_seq = seq;
    x.lane_hold[k].emplace_back(seq, std::static_pointer_cast<void>(in->p));
    return out;
}
}  // namespace fhelin
