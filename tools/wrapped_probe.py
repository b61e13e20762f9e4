#!/usr/bin/env python3
"""Wrapped inputs (include/fhelin.h "Wrapped inputs") at the driver's ring (the `bench` preset, N=2^16) on the driver's sample
(S = 129 tokens, 194 inputs), without and with the level plan.  Prints one JSON object with
  - bytes per sample: full ciphertexts, compact blobs (seeded encryption), wrapped compact blobs;
  - fhelin_client_ingest (seeded) against fhelin_client_ingest_wrapped (warm, device-synchronised, median of --reps);
  - the unwrap: ms per sample at B = 1 and B = 4 (one call for the B samples), its key switches and limb-NTTs per sample;
  - the server's pass per sample: the regular pass against unwrap + pass, the two interleaved in one session (median of --reps);
  - the logits' error against the circuit oracle for both paths, and the largest input error after unwrapping.
--stride s (default 1: the figures above, unchanged) runs the same measurements on an engine with interleaved samples
(include/fhelin.h "Interleaved samples"): the unit of every call is then a GROUP of s samples - fhelin_client_ingest_interleaved
against fhelin_client_ingest_wrapped_interleaved, one unwrap per group - and every "per sample" figure is the group's divided by s
(the *_per_group keys hold the group's); the logits' and the unwrapped inputs' errors are reported per lane.
Without a GPU it prints "not measured" and exits 0: nothing is estimated on the host.
  python tools/wrapped_probe.py [--reps 5] [--stride 1] [--modes off,plan] [--json out.json]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(eng, fn):
    eng.sync()
    t0 = time.perf_counter()
    r = fn()
    eng.sync()
    return 1e3 * (time.perf_counter() - t0), r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--stride", type=int, default=1, help="samples per ciphertext (slot stride)")
    ap.add_argument("--modes", default="off,plan", help="off (no level plan), plan, or both")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    try:
        import torch
        if not torch.cuda.is_available():
            raise RuntimeError
    except Exception:
        print(json.dumps({"wrapped_probe": "not measured: no GPU"}))
        return 0
    import fhe_linformer_amd as fa
    from fhe_linformer_amd import linformer as lf
    from oracle import plain_forward as pf, circuit_sim as cs
    S, variant = 129, "main"
    w = pf.synthetic_model(1234)
    s = a.stride
    eng = fa.Engine("bench", seed=11, n_q=28, n_p=-1, interleave=s)
    res = {"preset": "bench", "N": eng.N, "n_q": eng.n_q, "S": S, "inputs": 64 + S + 1, "reps": a.reps, "stride": s}
    try:
        eng.keygen()
        eng.gen_relin_key()
        eng.gen_rotation_keys(fa.circuit_rotation_indices())
        eng.bootstrap_setup(3, 3, 16384)
        eng.set_seeded_encryption(True)
        ctl = lf.GpuController(eng)
        args = (w["cls_token"], w["posEmb"], w["E_w"], w["E_b"], w["F_w"], w["F_b"])
        smp = [pf.synthetic_tokens(S, 4321 + k) for k in range(4 * s)]
        sref = [lf.logits_from_slots(lf.forward(cs.SlotSimController(), w, *pf.client_inputs(w, x), None, variant)) for x in smp]
        if s == 1:   # the unit of a call: a sample, or the group of s samples that share every ciphertext
            ing = lambda x: eng.client_ingest(*args, emb=x)
            ingw = lambda x: eng.client_ingest_wrapped(*args, emb=x)
            xs, refs = smp, [[r] for r in sref]
            lanes = lambda c: eng.decrypt(c, 16384)[None]
        else:
            ing = lambda x: eng.client_ingest_interleaved(*args, embs=x)
            ingw = lambda x: eng.client_ingest_wrapped_interleaved(*args, embs=x)
            xs, refs = [smp[s * k:s * k + s] for k in range(4)], [sref[s * k:s * k + s] for k in range(4)]
            lanes = lambda c: eng.decrypt_interleaved(c, 16384)
        logit_err = lambda out, k: [float(np.max(np.abs(lf.logits_from_slots(v) - r))) for v, r in zip(lanes(out), refs[k])]
        # the plan, recorded once with the regular ingest
        eng.level_plan_begin("record")
        lanes(lf.forward_encrypted(ctl, w, lf.ingest_sample(ctl, w, xs[0]), None, variant))
        plan = eng.level_plan_end()
        for mode in a.modes.split(","):
            r = res[mode] = {}
            begin = (lambda: eng.level_plan_begin("apply")) if mode == "plan" else (lambda: None)
            end = (lambda: eng.level_plan_end()) if mode == "plan" else (lambda: None)
            # bytes per sample
            begin()
            regular = ing(xs[0])
            end()
            flat = regular["inputs_E"] + regular["inputs_F"] + regular["inputs"]
            r["bytes_full"] = sum(2 * c.info()["ell"] * eng.N * 8 for c in flat)
            r["bytes_compact"] = sum(len(c.export_compact()) for c in flat)
            begin()
            ws = ingw(xs[0])
            end()
            r["wrapped_ciphertexts"] = [dict(count=h.wrapped_info()["count"], limbs=h.info()["ell"]) for h in ws]
            r["bytes_wrapped_compact"] = sum(len(h.export_compact()) for h in ws)
            if s > 1:   # the three figures above are the group's
                for k in ("bytes_full", "bytes_compact", "bytes_wrapped_compact"):
                    r[k + "_per_group"], r[k] = r[k], r[k] / s
            del regular, flat
            # client time
            ci, cw = [], []
            for _ in range(a.reps):
                begin()
                ci.append(timed(eng, lambda: ing(xs[1]))[0])
                end()
                begin()
                cw.append(timed(eng, lambda: ingw(xs[1]))[0])
                end()
            r["client_ingest_ms"], r["client_ingest_wrapped_ms"] = statistics.median(ci), statistics.median(cw)
            # unwrap alone: B = 1 and B = 4, with its operation counts
            for B in (1, 4):
                if mode == "plan":   # B samples' sources, sample-major (linformer.batched_level_plan)
                    eng.set_level_plan(lf.batched_level_plan(plan, B, 64 + S + 1))
                t = []
                for _ in range(a.reps):
                    begin()
                    wsb = [h for x in xs[:B] for h in ingw(x)]
                    eng.stats(reset=True)
                    ms, outs = timed(eng, lambda: eng.unwrap_inputs(wsb))
                    st = eng.stats()
                    end()
                    t.append(ms / B)
                    del outs, wsb
                if s > 1:
                    r[f"unwrap_ms_per_group_B{B}"], r[f"unwrap_ms_per_group_all_B{B}"] = statistics.median(t), t
                r[f"unwrap_ms_per_sample_B{B}"] = statistics.median(t) / s
                r[f"unwrap_ms_per_sample_all_B{B}"] = [v / s for v in t]
                r[f"unwrap_keyswitch_per_sample_B{B}"] = st["keyswitch"] / B / s
                r[f"unwrap_limb_ntt_per_sample_B{B}"] = st["limb_ntt"] / B / s
            if mode == "plan":
                eng.set_level_plan(plan)
            # the server's pass, regular and wrapped interleaved; logits against the oracle
            tr, tw, er, ew, kr, kw = [], [], [], [], [], []
            worst_in = [0.0] * s
            for k in range(a.reps):
                x = xs[k % 4]
                begin()
                enc = ing(x)
                eng.stats(reset=True)
                ms, out = timed(eng, lambda: lf.forward_encrypted(ctl, w, enc, None, variant))
                kr.append(eng.stats()["keyswitch"])
                er.append(logit_err(out, k % 4))
                end()
                tr.append(ms)
                del enc, out
                begin()
                ws = ingw(x)
                eng.stats(reset=True)

                def server():
                    outs = eng.unwrap_inputs(ws)
                    e = {"inputs_E": outs[:32], "inputs_F": outs[32:64], "inputs": outs[64:]}
                    return outs, lf.forward_encrypted(ctl, w, e, None, variant)

                ms, (outs, out) = timed(eng, server)
                kw.append(eng.stats()["keyswitch"])
                ew.append(logit_err(out, k % 4))
                end()
                tw.append(ms)
                if k == 0:
                    rows = []
                    for one in (x if s > 1 else [x]):
                        x_in, X_E, X_F = pf.client_inputs(w, one)
                        rows.append(list(X_E) + list(X_F) + list(x_in))
                    for v, c in enumerate(outs):
                        for i, got in enumerate(lanes(c)):
                            err = np.max(np.abs(got - np.repeat(rows[i][v], 128)))
                            worst_in[i] = max(worst_in[i], float(err / max(1.0, np.max(np.abs(rows[i][v])))))
                del ws, outs, out
            if s > 1:
                r["pass_regular_ms_per_group"], r["pass_wrapped_with_unwrap_ms_per_group"] = statistics.median(tr), statistics.median(tw)
            r["pass_regular_ms"] = statistics.median(tr) / s
            r["pass_wrapped_with_unwrap_ms"] = statistics.median(tw) / s
            r["pass_keyswitch_regular"], r["pass_keyswitch_wrapped"] = kr[0], kw[0]
            r["logits_err_regular_max"], r["logits_err_wrapped_max"] = max(max(e) for e in er), max(max(e) for e in ew)
            r["input_err_after_unwrap_rel_max"] = max(worst_in)
            if s > 1:
                r["logits_err_wrapped_per_lane"] = [max(e[i] for e in ew) for i in range(s)]
                r["input_err_after_unwrap_rel_per_lane"] = worst_in
    finally:
        eng.close()
    print(json.dumps(res, indent=1))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
