// Deferred evaluation behind the C boundary: rows of batched composites (LazyRows) and heavy single-ciphertext operations and
// additions (LazyHeavy) that are evaluated, batched, when a result is first read; the forcing rules; lane hand-over.
// capi_internal.h includes this header: the translation units of the boundary see both.
#pragma once
#include <functional>
#include <memory>
#include <string>
#include <utility>
#include <vector>
#include "composite.h"

struct fhelin_ctx;
struct fhelin_ct;

// Rows of a batched composite whose evaluation is DEFERRED until a row is consumed (fhelin_fc_matmul_pt,
// fhelin_fc_unwrapExpanded): the reference's drivers compute whole row sets of which later code reads a single row
// (src/main.cpp:183,:196 — all S query projections, only Q[0] used; :416-424 — all S tokens expanded, only output_2[0]
// used).  A row is evaluated the first time a handle to it is read — together with every other
// deferred row of the same call that the consuming operation also takes — and never if nobody reads it.  Rows are
// independent, so a forced row holds exactly the residues eager evaluation gives (bit-exact tests run with deferral
// on).  FHELIN_LAZY_ROWS=0 evaluates eagerly.
// fhelin_fc_matmulRElarge defers its rows too, for another reason: the drivers hand ALL of them to generate_containers next
// (src/main.cpp:341-352), and the two calls together are one shift sum per 32 rows (Composite::relarge_containers) where each alone
// is a tree per row and then the container sum.  generate_containers takes the fused form when every input is a row of
// matmulRElarge that nobody has read (same weights, bias and mask); a row somebody reads first is evaluated as matmulRElarge
// itself would.  The fused form is a different integer function with the same slot values: it is part of the default path the
// residue-level oracle restates (oracle/residue_controller.py).
namespace fhelin {
struct LazyRows {
    enum Kind { MatmulPt, UnwrapExpanded, RElarge } kind = MatmulPt;
    CtVec rows;                 // MatmulPt, RElarge: the input rows (kept alive)
    PtPtr w, bias;
    std::vector<PtPtr> weights; // RElarge: the four weight blocks; mask value
    double mask_val = 1.0;
    int slots = 0, padding = 0;
    CtPtr src;                  // UnwrapExpanded: the wrapped ciphertext
    int n = 0;
    std::vector<CtPtr> done;    // per row: null until evaluated
    int partial_reads = 0;      // reads so far that asked for only some of the rows (force_group)
    std::vector<int> node;      // level-plan recording: the rows' node ids ...
    int node_epoch = -1;        // ... of this recording (LevelPlan::epoch)
};
}
// Heavy single-ciphertext operations (bootstrap, Chebyshev evaluation) whose evaluation is DEFERRED until the result is read:
// the reference's drivers issue them in loops over independent ciphertexts (the GELU containers, src/main.cpp:354-358: eval_gelu
// then bootstrap per container; the two halves of affine-1, :313-314) and read the results only after the loop.  When the first
// result is read, everything pending is evaluated in dependency order with the operations of one kind, one parameter set and
// one input shape BATCHED (Evaluator::eval_chebyshev_many, Bootstrapper::bootstrap_batch): every launch then carries all of
// them and the switching keys / plaintext diagonals are read once.  Each result holds exactly the residues the single call gives.
// EvalAdd(ct, ct) is deferred the same way: the drivers' residual additions are loops of 130 single calls (src/main.cpp:237-239,
// output[i] = add(output[i], inputs[i])), each with a FLEXIBLEAUTO level adjustment of its own; read together they are ONE batched
// adjustment (integer multiply + rescale over all rows) and one batched addition.
// FHELIN_LAZY_HEAVY=0 (or a recording level-plan pass) evaluates at the call, on alternating worker lanes (run_heavy).
namespace fhelin {
struct LazyHeavy {
    enum Kind { Cheb, Boot, Add } kind = Boot;
    CtPtr in;                               // the input, once it exists ...
    std::shared_ptr<LazyHeavy> in_heavy;    // ... or the deferred operation that will produce it
    CtPtr in2;                              // Add: the second operand, likewise
    std::shared_ptr<LazyHeavy> in2_heavy;
    std::vector<double> coeffs;             // Cheb
    double a = 0, b = 0;
    int drop = 0;                           // Boot: limbs left out under a level plan
    int precision = 0;                      // Boot: > 0 = iterative bootstrap with this precision (Bootstrapper::bootstrap_iter)
    CtPtr result;
    bool done = false, failed = false;
    int err_code = 0;                       // failed: what the batched call that evaluated it threw (reported when the handle is read)
    std::string err_msg;
    int lane = 0;                           // the lane (stream) the call was made under: it is evaluated there (fhelin_ctx_set_lane)
};

using LazyGroups = std::vector<std::pair<LazyRows*, std::vector<int>>>;   // (group, rows of it)

// handles to the n rows of a deferred group
void emit_lazy(fhelin_ctx* c, const std::shared_ptr<LazyRows>& g, int n, fhelin_ct** outs);
// the still deferred rows among v[0..n), by group, each row once, in first-seen order; a deferred heavy operation among the handles
// is evaluated on the way (the first one evaluates everything pending).  A null handle is refused (strict_null) or passed over
LazyGroups lazy_groups(fhelin_ctx* c, const fhelin_ct* const* v, int n, bool strict_null);
// evaluate the listed rows of a deferred group in ONE batched call
void force_rows(fhelin_ctx* c, LazyRows& g, const std::vector<int>& idx);
// the same for several groups at once; groups that are the same call on different inputs (one call per sample of a batch) share
// their batched key switches
void force_rows_multi(fhelin_ctx* c, LazyGroups& reqs);
std::vector<int> rows_for_read(LazyRows& g, const std::vector<int>& idx);
// A consumer asks for rows `idx` of a deferred group.  The first partial read evaluates just those rows (a driver that
// uses Q[0] only); a second one means the driver is walking over the rows (for (i...) output[i] = add(output[i],
// inputs[i]), src/main.cpp:237-239): everything that is left is evaluated in one batched call instead of row by row.
void force_group(fhelin_ctx* c, LazyRows& g, const std::vector<int>& idx);
// `h` is about to be read: a deferred heavy operation is evaluated under the lane it was issued under (with everything else pending
// there) and its own failure, if any, is thrown; a deferred row is evaluated by force_group's rule
void force(fhelin_ctx* c, const fhelin_ct* h);
// the deferred rows among v[0..n) are evaluated together, one batched call per group
void force_many(fhelin_ctx* c, const fhelin_ct* const* v, int n);
// evaluate every pending deferred heavy operation, batched
// report: throw the first failure of this flush (fhelin_sync / fhelin_ctx_trim: "evaluate everything pending"); a read of ONE result
// (force) does not - it reports that result's own failure, if any, and leaves the others' to their readers
void flush_heavy(fhelin_ctx* c, bool report = false);          // the CURRENT lane's pending operations
void flush_lane(fhelin_ctx* c, int lane, bool report = false); // lane `lane`'s, under that lane; the current one is back afterwards
void flush_heavy_all(fhelin_ctx* c, bool report = false);      // every lane's, each on its own stream; the first Error is rethrown at the end
// a value produced under lane `lane` is about to be read under the current one: order the current stream behind that lane's work
void wait_for_lane(fhelin_ctx* c, int lane);
// deferral on the context's main stream or on a lane the CALLER selected (fhelin_ctx_set_lane) - not inside the library's own lane scopes
bool defer_allowed(fhelin_ctx* c);
// a handle to the deferred operation `op` (its kind and parameters set by the caller) on `a`, itself possibly deferred
fhelin_ct* defer_heavy(fhelin_ctx* c, const fhelin_ct* a, const std::shared_ptr<LazyHeavy>& op);
// a handle to the deferred sum a + b (either operand possibly deferred itself)
fhelin_ct* defer_add(fhelin_ctx* c, const fhelin_ct* a, const fhelin_ct* b);
// Run a heavy single-ciphertext op (bootstrap, polynomial evaluation) on a worker lane without joining it.  Ops issued
// back to back on independent ciphertexts (the reference's per-container loops, src/main.cpp:354-358, :313-314)
// then overlap on the GPU; a chain on the same ciphertext stays on its lane.  Falls back to the main stream when
// lanes are off.
CtPtr run_heavy(fhelin_ctx* c, const fhelin_ct* in, const std::function<CtPtr(const CtPtr&)>& f);
}  // namespace fhelin
