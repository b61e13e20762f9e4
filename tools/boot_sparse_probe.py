#!/usr/bin/env python3
"""Sparse-secret bootstrapping (include/fhelin.h "Sparse-secret bootstrapping") measured against the default path of the same
build:
    tools/boot_sparse_probe.py [--steps 3] [--hamming 32] [--no-driver] [--out profiles/boot_sparse_n16.json]
At the headline chain (N = 2^16, 28+7 limbs, 16384 slots), two contexts in one process - the knob off and on (it binds at
bootstrap_setup) - alternating call by call, device events around each call:
  1. ms per bootstrap, single and in a batch of 5, at drop 0 and at the GELU bootstraps' planned drop of 4; limbs out; the maximum
     decryption error; limb-NTTs and key switches per bootstrap from fhelin_stats;
  2. ms per phase (ModRaise + SubSum with the two switches, CoeffsToSlots, EvalMod, SlotsToCoeffs) as differences of
     bootstrap_partial(ct, 1 / 2 / 3) and the whole bootstrap;
  3. bytes of the two new keys as held (the to-sparse key at two limbs, the from-sparse key whole) against two uncapped keys;
  4. the `main` driver at 1 and 4 samples per pass with the knob off and on: ms per sample, bootstraps per pass and the maximum logits
     error against oracle/circuit_sim.py (the bench's samples, seeds 4321 + i).  One sample per pass alternates pass by pass; at four the
     two contexts' memory pools do not fit the device side by side, so each context runs its rounds in a row.
One JSON line.  Without a GPU it prints "not measured" and exits 0: nothing is estimated on the host."""
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
    ap.add_argument("--hamming", type=int, default=32, help="Hamming weight of the ephemeral secret")
    ap.add_argument("--no-driver", action="store_true", help="parts 1-3 only")
    ap.add_argument("--out", default=None, help="also write the line to this file")
    args = ap.parse_args()
    try:
        import torch
        if not torch.cuda.is_available():
            raise RuntimeError
    except Exception:
        print(json.dumps({"boot_sparse_probe": "not measured: no GPU"}))
        return 0

    import fhe_linformer_amd as fa
    from fhe_linformer_amd import linformer as lf

    med = statistics.median
    note = lambda *a: print(*a, file=sys.stderr, flush=True)     # progress; the result is the one line on stdout
    n = 16384
    engines = {}
    res = {"tool": "boot_sparse_probe", "log_n": 16, "slots": n, "steps": args.steps, "hamming": args.hamming}
    try:
        for which in ("off", "on"):
            e = fa.Engine("bench", seed=11, n_q=28, n_p=-1)
            e.keygen()
            e.gen_relin_key()
            if not args.no_driver:
                e.gen_rotation_keys(fa.circuit_rotation_indices())
            if which == "on":
                e.set_bootstrap_sparse_secret(args.hamming)
            e.bootstrap_setup(3, 3, n)
            engines[which] = e
        e0 = engines["off"]
        res["limbs"] = f"{e0.n_q}+{e0.n_p}"
        desc = {k: e.bootstrap_describe() for k, e in engines.items()}
        res["config"] = {k: {f: d[f] for f in ("K", "R", "cheb_degree", "depth", "sparse_h")} for k, d in desc.items()}

        def timed(e, f):
            e.sync()
            e.timer_start()
            out = f()
            for o in (out if isinstance(out, list) else [out]):
                o.info()
            return out, e.timer_stop()

        # ---- 1. whole bootstraps
        res["bootstrap"] = {}
        for drop in (0, 4):
            for B in (1, 5):
                ms = [np.random.default_rng(10 + i).uniform(-1, 1, n) for i in range(B)]
                t, err, st, ell = {"off": [], "on": []}, {}, {}, {}
                cts = {k: [e.encrypt(v, level=e.n_q - 2) for v in ms] for k, e in engines.items()}
                for it in range(args.steps + 1):            # the first round warms both up
                    for k, e in engines.items():
                        e.set_level_plan([e.n_q - desc[k]["depth"] - drop] * B)
                        e.level_plan_begin("apply")
                        before = e.stats()
                        outs, dt = timed(e, (lambda: e.bootstrap_batch(cts[k])) if B > 1 else (lambda: [e.bootstrap(cts[k][0])]))
                        after = e.stats()
                        e.level_plan_begin("off")
                        if it:
                            t[k].append(dt / B)
                        st[k] = {s: (after[s] - before[s]) / B for s in ("limb_ntt", "keyswitch", "ct_pt_mult")}
                        ell[k] = outs[0].info()["ell"]
                        err[k] = float(max(np.max(np.abs(e.decrypt(o) - v)) for o, v in zip(outs, ms)))
                        del outs
                res["bootstrap"][f"drop{drop}_batch{B}"] = {
                    "off_ms": med(t["off"]), "on_ms": med(t["on"]), "ratio": med(t["on"]) / med(t["off"]),
                    "off_spread_ms": max(t["off"]) - min(t["off"]), "off_limbs_out": ell["off"], "on_limbs_out": ell["on"],
                    "off_max_err": err["off"], "on_max_err": err["on"], "off_stats": st["off"], "on_stats": st["on"],
                    "off_ms_all": [round(x, 3) for x in t["off"]], "on_ms_all": [round(x, 3) for x in t["on"]]}
                note("bootstrap", drop, B, res["bootstrap"][f"drop{drop}_batch{B}"])
                del cts

        # ---- 2. phases, by difference of the partial bootstraps (drop 0, one ciphertext)
        m = np.random.default_rng(3).uniform(-1, 1, n)
        ph = {"off": {s: [] for s in (1, 2, 3, 0)}, "on": {s: [] for s in (1, 2, 3, 0)}}
        cts = {k: e.encrypt(m, level=e.n_q - 2) for k, e in engines.items()}
        for it in range(args.steps + 1):
            for k, e in engines.items():
                for s in (1, 2, 3, 0):
                    _, dt = timed(e, (lambda: e.bootstrap_partial(cts[k], s)) if s else (lambda: e.bootstrap_drop(cts[k], 0)))
                    if it:
                        ph[k][s].append(dt)
        res["phase_ms"] = {}
        for k in engines:
            a, b, c, d = (med(ph[k][s]) for s in (1, 2, 3, 0))
            res["phase_ms"][k] = {"modraise_subsum": a, "coeffs_to_slots": b - a, "eval_mod": c - b, "slots_to_coeffs": d - c, "bootstrap": d}
        note("phases", res["phase_ms"])

        # ---- 3. the two new keys: present rows as held, against two uncapped keys
        e1 = engines["on"]
        i3, i4 = e1.key_info(3), e1.key_info(4)
        row = e1.N * 8
        held = lambda i: i["digits"] * 2 * (min(i["max_ell"], e1.n_q) + e1.n_p) * row
        res["keys"] = {"to_sparse": dict(i3, present_bytes=held(i3)), "from_sparse": dict(i4, present_bytes=held(i4)),
                       "uncapped_bytes_each": e1.dnum_digits * 2 * e1.n_limbs * row}
        note("keys", res["keys"])

        # ---- 4. the driver
        if not args.no_driver:
            from oracle import plain_forward as pf, circuit_sim as cs
            S, W = args.tokens, 4
            w = pf.synthetic_model(1234)
            xs = [pf.synthetic_tokens(S, 4321 + i) for i in range(W)]
            ref = [lf.logits_from_slots(lf.forward(cs.SlotSimController(), w, *pf.client_inputs(w, x), None, "main")) for x in xs]
            drv = {}
            for k, e in engines.items():
                ctl = lf.GpuController(e)
                e.level_plan_begin("record")
                enc_rec = lf.encrypt_inputs(ctl, *pf.client_inputs(w, pf.synthetic_tokens(S, 999)))
                n_client = sum(len(v) for v in enc_rec.values())
                e.decrypt(lf.forward_encrypted(ctl, w, enc_rec, None, "main"))
                plan = e.level_plan_end()
                del enc_rec
                bplan = lf.batched_level_plan(plan, W, n_client)
                encs = []
                for x in xs:
                    e.set_level_plan(plan)
                    e.level_plan_begin("apply")
                    encs.append(lf.ingest_sample(ctl, w, x))
                    e.level_plan_begin("off")
                drv[k] = dict(ctl=ctl, bctl=lf.BatchedController(e, W), plan=plan, bplan=bplan, n_client=n_client, encs=encs)

            def run(k, width):
                e, d = engines[k], drv[k]
                e.set_level_plan(d["plan"] if width == 1 else d["bplan"])
                e.level_plan_begin("apply", first_source=d["n_client"] * width)
                before = e.stats()["bootstrap"]
                e.sync()
                e.timer_start()
                if width == 1:
                    outs = [lf.forward_encrypted(d["ctl"], w, d["encs"][0], None, "main")]
                else:
                    outs = list(lf.forward_encrypted(d["bctl"], w, lf.batch_inputs(d["encs"]), None, "main"))
                for o in outs:
                    o.info()                            # deferred results are evaluated here
                t = e.timer_stop()
                boots = int(e.stats()["bootstrap"] - before)
                e.level_plan_begin("off")
                errs = [float(np.max(np.abs(lf.logits_from_slots(e.decrypt(o, 16384)) - r))) for o, r in zip(outs, ref)]
                return t, errs, boots

            res["driver"] = {}
            for width in (1, W):
                t, last = {"off": [], "on": []}, {}
                order = [(it, k) for it in range(args.steps + 1) for k in engines] if width == 1 else \
                        [(it, k) for k in engines for it in range(args.steps + 1)]
                for it, k in order:
                    last[k] = run(k, width)
                    if it:
                        t[k].append(last[k][0])
                    note("driver", width, k, last[k])
                    if width > 1 and it == args.steps:
                        engines[k].trim()
                res["driver"][str(width)] = {
                    "alternating": width == 1,
                    "off_ms_per_sample": med(t["off"]) / width, "on_ms_per_sample": med(t["on"]) / width, "ratio": med(t["on"]) / med(t["off"]),
                    "off_logits_err": last["off"][1], "on_logits_err": last["on"][1],
                    "off_bootstraps_per_pass": last["off"][2], "on_bootstraps_per_pass": last["on"][2],
                    "off_ms_all": [round(x / width, 3) for x in t["off"]], "on_ms_all": [round(x / width, 3) for x in t["on"]]}
    finally:
        for e in engines.values():
            e.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
