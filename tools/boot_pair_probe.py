#!/usr/bin/env python3
"""Paired bootstrapping (include/fhelin.h "Paired bootstrapping") measured against the plain batched pipeline:
    tools/boot_pair_probe.py [--steps 3] [--no-driver] [--out FILE]
At the headline chain (N = 2^16, 28+7 limbs, 16384 slots):
  1. bootstrap_batch against bootstrap_paired_batch for n = 2, 5, 8 ciphertexts at the GELU bootstraps' planned drop of 4 limbs,
     alternating call by call, device events around each call; the maximum decryption error of each.
  2. the `main` driver with the pairing knob off and on, alternating pass by pass, at 1 and at 4 samples per pass (GpuController /
     BatchedController under a level plan recorded once): ms per sample, pipelines per sample (the `bootstrap` counter of fhelin_stats)
     and the maximum logits error against oracle/circuit_sim.py over the bench's samples (seeds 4321 + i).
One JSON line."""
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
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--tokens", type=int, default=129)
    ap.add_argument("--drop", type=int, default=4)
    ap.add_argument("--no-driver", action="store_true", help="part 1 only")
    ap.add_argument("--out", default=None, help="also write the line to this file")
    args = ap.parse_args()

    import fhe_linformer_amd as fa
    from fhe_linformer_amd import linformer as lf
    from oracle import plain_forward as pf, circuit_sim as cs

    med = statistics.median
    note = lambda *a: print(*a, file=sys.stderr, flush=True)     # progress; the result is the one line on stdout
    e = fa.Engine("bench", seed=11, n_q=28, n_p=-1)
    res = {"tool": "boot_pair_probe", "log_n": 16, "limbs": f"{e.n_q}+{e.n_p}", "slots": 16384, "steps": args.steps, "drop": args.drop}
    try:
        e.keygen()
        e.gen_relin_key()
        if not args.no_driver:
            e.gen_rotation_keys(fa.circuit_rotation_indices())
        e.bootstrap_setup(3, 3, 16384)
        n = 16384

        # ---- 1. the pipelines alone
        def timed(f):
            e.sync()
            e.timer_start()
            out = f()
            return out, e.timer_stop()

        res["batch"] = {}
        for B in (2, 5, 8):
            ms = [np.random.default_rng(10 + i).uniform(-1, 1, n) for i in range(B)]
            cts = [e.encrypt(v, level=e.n_q - 2) for v in ms]
            plan = [e.n_q - 15 - args.drop] * B
            t_plain, t_pair = [], []
            for it in range(args.steps + 1):            # the first round warms both up
                for which, call, ts in (("plain", e.bootstrap_batch, t_plain), ("paired", e.bootstrap_paired_batch, t_pair)):
                    e.set_level_plan(plan)
                    e.level_plan_begin("apply")
                    before = e.stats()["bootstrap"]
                    outs, t = timed(lambda: call(cts))
                    e.level_plan_begin("off")
                    if it:
                        ts.append(t)
                    if which == "plain":
                        plain_outs, plain_pipes = outs, e.stats()["bootstrap"] - before
                    else:
                        pair_outs, pair_pipes = outs, e.stats()["bootstrap"] - before
            err = lambda outs: float(max(np.max(np.abs(e.decrypt(o) - v)) for o, v in zip(outs, ms)))
            res["batch"][str(B)] = {"plain_ms": med(t_plain), "paired_ms": med(t_pair), "ratio": med(t_pair) / med(t_plain),
                                    "plain_pipelines": plain_pipes, "paired_pipelines": pair_pipes, "out_ell": plain_outs[0].info()["ell"],
                                    "plain_max_err": err(plain_outs), "paired_max_err": err(pair_outs),
                                    "plain_ms_all": [round(t, 3) for t in t_plain], "paired_ms_all": [round(t, 3) for t in t_pair]}
            note("batch", B, res["batch"][str(B)])
            del cts, plain_outs, pair_outs

        # ---- 2. the driver
        if not args.no_driver:
            S, W = args.tokens, 4
            w = pf.synthetic_model(1234)
            xs = [pf.synthetic_tokens(S, 4321 + i) for i in range(W)]
            ref = [lf.logits_from_slots(lf.forward(cs.SlotSimController(), w, *pf.client_inputs(w, x), None, "main")) for x in xs]
            ctl = lf.GpuController(e)
            e.level_plan_begin("record")
            enc_rec = lf.encrypt_inputs(ctl, *pf.client_inputs(w, pf.synthetic_tokens(S, 999)))
            n_client = sum(len(v) for v in enc_rec.values())
            e.decrypt(lf.forward_encrypted(ctl, w, enc_rec, None, "main"))
            plan = e.level_plan_end()
            del enc_rec
            bplan = lf.batched_level_plan(plan, W, n_client)
            bctl = lf.BatchedController(e, W)

            def ingest(x):
                e.set_level_plan(plan)
                e.level_plan_begin("apply")
                enc = lf.ingest_sample(ctl, w, x)
                e.level_plan_begin("off")
                return enc
            encs = [ingest(x) for x in xs]

            def run(width, on):
                """one pass at `width` samples: (ms, pipelines, per-sample logits errors)"""
                e.set_bootstrap_pairing(on)
                e.set_level_plan(plan if width == 1 else bplan)
                e.level_plan_begin("apply", first_source=n_client * width)
                before = e.stats()["bootstrap"]
                e.sync()
                e.timer_start()
                if width == 1:
                    outs = [lf.forward_encrypted(ctl, w, encs[0], None, "main")]
                else:
                    outs = list(lf.forward_encrypted(bctl, w, lf.batch_inputs(encs), None, "main"))
                for o in outs:
                    o.info()                            # deferred results are evaluated here
                t = e.timer_stop()
                e.level_plan_begin("off")
                pipes = e.stats()["bootstrap"] - before
                errs = [float(np.max(np.abs(lf.logits_from_slots(e.decrypt(o, 16384)) - r))) for o, r in zip(outs, ref)]
                e.set_bootstrap_pairing(False)
                return t, pipes, errs

            res["driver"] = {}
            for width in (1, W):
                t_off, t_on = [], []
                for it in range(args.steps + 1):
                    a = run(width, False)
                    b = run(width, True)
                    note("driver", width, "off", a, "on", b)
                    if it:
                        t_off.append(a[0])
                        t_on.append(b[0])
                res["driver"][str(width)] = {
                    "off_ms_per_sample": med(t_off) / width, "on_ms_per_sample": med(t_on) / width, "ratio": med(t_on) / med(t_off),
                    "off_pipelines_per_sample": a[1] / width, "on_pipelines_per_sample": b[1] / width,
                    "off_logits_err": a[2], "on_logits_err": b[2],
                    "off_ms_all": [round(t / width, 3) for t in t_off], "on_ms_all": [round(t / width, 3) for t in t_on]}
    finally:
        e.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
