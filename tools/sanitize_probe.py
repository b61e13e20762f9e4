#!/usr/bin/env python3
"""Sanitised replies (include/fhelin.h "Sanitised replies") at the driver's ring (the `bench` preset, N=2^16, 28 + 7 limbs) on the
driver's own result ciphertext (S = 129 tokens, main driver).  Prints one JSON object with
  - reply bytes before (the ciphertext the circuit ends with) and after sanitisation (keep the 20 logit slots, out_ell = 2);
  - ms per reply at batch 1 and batch 4 (one call for the batch), device events, warm, median of --reps, per flood_bits;
  - the logits' error against the circuit oracle without sanitisation and with flood_bits 0 / 20 / 30, and the largest magnitude any
    other slot of the reply decrypts to (before: what the raw result leaks there).
Without a GPU it prints "not measured" and exits 0: nothing is estimated on the host.
  python tools/sanitize_probe.py [--reps 5] [--json out.json]"""
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
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    try:
        import torch
        if not torch.cuda.is_available():
            raise RuntimeError
    except Exception:
        print(json.dumps({"sanitize_probe": "not measured: no GPU"}))
        return 0
    import fhe_linformer_amd as fa
    from fhe_linformer_amd import linformer as lf
    from oracle import plain_forward as pf, circuit_sim as cs
    S, variant = 129, "main"
    w = pf.synthetic_model(1234)
    eng = fa.Engine("bench", seed=11, n_q=28, n_p=-1)
    res = {"preset": "bench", "N": eng.N, "n_q": eng.n_q, "n_p": eng.n_p, "S": S, "reps": a.reps, "keep_slots": len(lf.LOGIT_SLOTS), "out_ell": 2}
    try:
        eng.keygen()
        eng.gen_relin_key()
        eng.gen_rotation_keys(fa.circuit_rotation_indices())
        eng.bootstrap_setup(3, 3, 16384)
        ctl = lf.GpuController(eng)
        xs = [pf.synthetic_tokens(S, 4321 + k) for k in range(4)]
        refs = [lf.logits_from_slots(lf.forward(cs.SlotSimController(), w, *pf.client_inputs(w, x), None, variant)) for x in xs]
        raws = [lf.forward_encrypted(ctl, w, lf.ingest_sample(ctl, w, x), None, variant) for x in xs]
        eng.force(raws)
        others = np.ones(16384, dtype=bool)
        others[list(lf.LOGIT_SLOTS)] = False
        inf = raws[0].info()
        res["raw"] = dict(limbs=inf["ell"], deg=inf["deg"], npoly=inf["npoly"], bytes=inf["npoly"] * inf["ell"] * eng.N * 8)
        dec = [eng.decrypt(r) for r in raws]
        res["raw"]["logits_err_max"] = max(float(np.max(np.abs(lf.logits_from_slots(d) - ref))) for d, ref in zip(dec, refs))
        res["raw"]["other_slots_max"] = max(float(np.max(np.abs(d[others]))) for d in dec)
        mask = eng.encode(lf._keep_mask(lf.LOGIT_SLOTS))
        for bits in (0, 20, 30):
            r = res[f"flood_bits_{bits}"] = {}
            replies = eng.sanitize(raws, mask, bits, 2)                      # also the warm-up of every path timed below
            ri = replies[0].info()
            r["limbs"], r["bytes"] = ri["ell"], ri["npoly"] * ri["ell"] * eng.N * 8
            dec = [eng.decrypt(c) for c in replies]
            r["logits_err_max"] = max(float(np.max(np.abs(lf.logits_from_slots(d) - ref))) for d, ref in zip(dec, refs))
            r["other_slots_max"] = max(float(np.max(np.abs(d[others]))) for d in dec)
            hi, lo = replies[0].scale_parts()
            r["predicted_slot_sigma"] = float(np.sqrt(16384.0) * np.sqrt(4.0 ** bits / 3 + 3.19 ** 2 * (2 * eng.N / 3 + 193)) / (hi + lo))
            del replies
            for B in (1, 4):
                t = []
                for _ in range(a.reps):
                    eng.sync()
                    eng.timer_start()
                    out = eng.sanitize(raws[:B], mask, bits, 2)
                    t.append(eng.timer_stop() / B)
                    del out
                r[f"ms_per_reply_B{B}"] = statistics.median(t)
            # re-randomisation and level drop alone (no mask): the fused launch and its sampling
            one = eng.rescale(raws[0]) if inf["deg"] > 1 else raws[0]
            t = []
            for _ in range(a.reps):
                eng.sync()
                eng.timer_start()
                out = eng.sanitize(one, None, bits, 2)
                t.append(eng.timer_stop())
                del out
            r["ms_rerandomise_only_B1"] = statistics.median(t)
    finally:
        eng.close()
    print(json.dumps(res, indent=1))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
