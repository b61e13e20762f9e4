#!/usr/bin/env python3
"""Interleaved samples (include/fhelin.h "Interleaved samples") measured against single passes:
    tools/interleave_probe.py [--log-n 16|17] [--stride 2|4] [--steps 5] [--out FILE]
At the headline chain (N = 2^16: 28+7 limbs; --log-n 17: 30+7) the `main` driver runs on the same `stride` synthetic samples twice per
step: as `stride` single passes on a stride-1 engine (A) and as ONE pass on an engine with that slot stride (B), A and B alternating
step by step.  Both run under a level plan recorded on their own first pass.  Times are device events around the server side of a
pass (forward_encrypted up to the result's last launch).  One JSON line: ms per pass and per sample for both, ms per bootstrap at
the sparse and at the fuller packing, limb-NTTs and key switches per sample, pool bytes in use, and per lane the maximum logits
error against oracle/circuit_sim.py and the decrypted error of the first bootstrap."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-n", type=int, default=16, choices=[16, 17])
    ap.add_argument("--stride", type=int, default=2, choices=[2, 4])
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--tokens", type=int, default=129)
    ap.add_argument("--out", default=None, help="also write the line to this file")
    args = ap.parse_args()
    if (16384 * args.stride) > (1 << (args.log_n - 1)):
        ap.error("16384 slots x stride exceed N/2 at this ring")

    import fhe_linformer_amd as fa
    from fhe_linformer_amd import linformer as lf
    from oracle import plain_forward as pf, circuit_sim as cs

    s, S = args.stride, args.tokens
    preset, n_q = ("bench", 28) if args.log_n == 16 else ("deep", 30)
    w = pf.synthetic_model(1234)
    xs = [pf.synthetic_tokens(S, 4321 + i) for i in range(s)]
    ref_logits, ref_affine = [], []
    for x in xs:
        st = {}
        ref_logits.append(lf.logits_from_slots(lf.forward(cs.SlotSimController(), w, *pf.client_inputs(w, x), st, "main")))
        ref_affine.append(np.asarray(st["affine1_0"]))

    def engine(stride):
        e = fa.Engine(preset, seed=11, n_q=n_q, n_p=-1, interleave=stride)
        e.keygen()
        e.gen_relin_key()
        e.gen_rotation_keys(fa.circuit_rotation_indices())
        e.bootstrap_setup(3, 3, 16384)
        return e

    def one_pass(e, ctl, sample, mode, trace=None):
        """client side, then the timed server side; sample: one embedding (stride 1) or the list of the group's"""
        if mode:
            e.level_plan_begin(mode)
        enc = lf.ingest_sample(ctl, w, sample)
        e.sync()
        e.timer_start()
        out = lf.forward_encrypted(ctl, w, enc, trace, "main")
        ms = e.timer_stop()
        if mode:
            e.level_plan_end()
        return out, ms

    eA, eB = engine(1), engine(s)
    cA, cB = lf.GpuController(eA), lf.GpuController(eB)
    res = {"tool": "interleave_probe", "log_n": args.log_n, "limbs": f"{eA.n_q}+{eA.n_p}", "stride": s, "tokens": S, "steps": args.steps}
    try:
        # first pass of each: masks and model plaintexts are encoded once, the level plan is recorded
        one_pass(eA, cA, xs[0], "record")
        one_pass(eB, cB, xs, "record")
        a_ms, b_ms = [], []
        for step in range(args.steps):                    # A and B alternate: neither has the warmer device
            eA.stats(reset=True)
            tot, outs = 0.0, []
            for x in xs:
                o, ms = one_pass(eA, cA, x, "apply")
                tot += ms
                outs.append(o)
            stA = eA.stats()
            a_ms.append(tot)
            eB.stats(reset=True)
            outB, ms = one_pass(eB, cB, xs, "apply")
            stB = eB.stats()
            b_ms.append(ms)
        med = statistics.median
        res["single"] = {"ms_per_pass": med(a_ms) / s, "ms_per_sample": med(a_ms) / s, "ms_all_steps": [round(v / s, 3) for v in a_ms],
                         "limb_ntt_per_sample": stA["limb_ntt"] / s, "keyswitch_per_sample": stA["keyswitch"] / s,
                         "pool_live_bytes": eA.cache_stats()["pool_live_bytes"], "pool_live_peak_bytes": stA["pool_live_peak_bytes"]}
        res["interleaved"] = {"ms_per_pass": med(b_ms), "ms_per_sample": med(b_ms) / s, "ms_all_steps": [round(v, 3) for v in b_ms],
                              "limb_ntt_per_sample": stB["limb_ntt"] / s, "keyswitch_per_sample": stB["keyswitch"] / s,
                              "pool_live_bytes": eB.cache_stats()["pool_live_bytes"], "pool_live_peak_bytes": stB["pool_live_peak_bytes"]}
        res["per_sample_ratio"] = res["interleaved"]["ms_per_sample"] / res["single"]["ms_per_sample"]
        res["single"]["logits_err"] = [float(np.max(np.abs(lf.logits_from_slots(eA.decrypt(o, 16384)) - r))) for o, r in zip(outs, ref_logits)]
        lanes = cB.decrypt_lanes(outB)
        res["interleaved"]["logits_err"] = [float(np.max(np.abs(lf.logits_from_slots(lanes[i]) - ref_logits[i]))) for i in range(s)]
        res["argmax_equal"] = [int(np.argmax(lf.logits_from_slots(lanes[i]))) == int(np.argmax(ref_logits[i])) for i in range(s)]

        # the first bootstrap of the pass (its input: affine1_0): time and decrypted error, sparse against the fuller packing
        def boot(e, ctl, sample, lanes_of):
            tr = {}
            one_pass(e, ctl, sample, None, tr)
            x = tr["affine1_0"]
            before = lanes_of(x)
            t = []
            for _ in range(3):
                e.sync()
                e.timer_start()
                y = e.bootstrap(x)
                y.info()                                   # deferred: evaluated here
                t.append(e.timer_stop())
            after = lanes_of(y)
            return med(t), before, after
        msA, b0, a0 = boot(eA, cA, xs[0], lambda c: eA.decrypt(c, 16384)[None])
        msB, b1, a1 = boot(eB, cB, xs, lambda c: eB.decrypt_interleaved(c, 16384))
        res["single"]["ms_per_bootstrap"] = msA
        res["interleaved"]["ms_per_bootstrap"] = msB
        res["single"]["first_bootstrap_err"] = [float(np.max(np.abs(a0[0] - b0[0])))]
        res["interleaved"]["first_bootstrap_err"] = [float(np.max(np.abs(a1[i] - b1[i]))) for i in range(s)]
        res["interleaved"]["affine1_err_vs_oracle"] = [float(np.max(np.abs(b1[i] - ref_affine[i]))) for i in range(s)]
    finally:
        eA.close()
        eB.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
