#!/usr/bin/env python3
"""Linear transforms (include/fhelin.h "Linear transforms") at the driver's ring: N = 2^16, 28 + 7 limbs, one ciphertext at 13 limbs,
32 and 128 dense diagonals, each at the planner's split and at n1 = 8.  Per case, alternating, warm, device events, median of --reps:
  - `lt_apply`: fhelin_lt_apply;
  - `composition`: the bootstrap-style form through existing entry points - rotate_many over the baby steps, one mult_plain / add sum
    per group, rotate_each_sum over the groups;
  - `hoisted` (n1 <= 8 only): fhelin_hoisted_dot per group, then rotate_each_sum;
with limb-NTTs and key switches per call (fhelin_stats) and the device bytes the plan's full-basis encodings hold against the folded
key copies fhelin_hoisted_dot would need for the same terms.  Prints one JSON object.  Without a GPU it prints "not measured" and
exits 0: nothing is estimated on the host.
  python tools/lt_probe.py [--reps 9] [--json out.json]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ELL = 13


def timed(eng, fn):
    eng.timer_start()
    out = fn()
    ms = eng.timer_stop()
    return ms, out


def counted(eng, fn):
    eng.stats(reset=True)
    fn()
    eng.sync()
    s = eng.stats()
    return {"limb_ntt": s["limb_ntt"], "keyswitch": s["keyswitch"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    try:
        import torch
        if not torch.cuda.is_available():
            raise RuntimeError
    except Exception:
        print(json.dumps({"lt_probe": "not measured: no GPU"}))
        return 0
    import fhe_linformer_amd as fa
    eng = fa.Engine("bench", seed=17, n_q=28, n_p=-1)
    ns = 1 << eng.params.log_slots
    res = {"preset": "bench", "N": eng.N, "n_q": eng.n_q, "n_p": eng.n_p, "limbs": ELL, "slots": ns, "reps": a.reps, "cases": {}}
    try:
        eng.keygen()
        rng = np.random.default_rng(3)
        xv = rng.uniform(-1, 1, ns)
        x = eng.encrypt(xv, level=eng.n_q - ELL)
        key_bytes = eng.dnum_digits * 2 * eng.n_limbs * eng.N * 8
        for n_diag in (32, 128):
            diags = rng.uniform(-1, 1, (n_diag, ns))
            idx = list(range(n_diag))
            want = sum(d * np.roll(xv, -i) for d, i in zip(diags, idx))
            for n1_arg in (0, 8):
                lt = eng.lt_create(diags, idx, n1=n1_arg)
                inf = lt.info()
                n1, n2 = inf["n1"], inf["n2"]
                baby, giant = list(range(n1)), [g * n1 for g in range(n2)]
                eng.gen_rotation_keys(lt.rotations())
                pts = [[eng.encode(np.roll(diags[g + b], g)) if g + b < n_diag else None for b in baby] for g in giant]

                def new_path():
                    return eng.lt_apply(lt, [x])[0]

                def composition():
                    rot = [x] + eng.rotate_many(x, baby[1:])
                    inner = []
                    for row in pts:
                        acc = None
                        for c, p in zip(rot, row):
                            if p is not None:
                                t = eng.mult(c, p)
                                acc = t if acc is None else eng.add(acc, t)
                        inner.append(acc)
                    return eng.rotate_each_sum(inner, giant)

                def hoisted():
                    return eng.rotate_each_sum([eng.hoisted_dot([x], row, baby[1:])[0] for row in pts], giant)

                paths = {"lt_apply": new_path, "composition": composition}
                if n1 <= 8 and all(p is not None for row in pts for p in row):
                    paths["hoisted"] = hoisted
                r = {"n1": n1, "n2": n2, "n_terms": inf["n_terms"], "rotation_keys": len(lt.rotations())}
                for name, fn in paths.items():       # warm-up: encodings, permuted / folded keys; and the value each path decrypts to
                    r["max_error_" + name] = float(np.max(np.abs(eng.decrypt(fn())[:ns] - want)))
                    r["per_call_" + name] = counted(eng, fn)
                ms = {name: [] for name in paths}
                for _ in range(a.reps):              # alternating: drift hits every path alike
                    for name, fn in paths.items():
                        ms[name].append(timed(eng, fn)[0])
                for name in paths:
                    r["ms_" + name] = statistics.median(ms[name])
                    r["ms_spread_" + name] = [min(ms[name]), max(ms[name])]
                n_rot_terms = sum(1 for row in pts for b, p in enumerate(row) if p is not None and b > 0)
                r["plan_encoding_bytes"] = inf["n_terms"] * eng.n_limbs * eng.N * 8       # [n_q + n_p][N] per term
                r["folded_key_bytes_same_terms"] = n_rot_terms * key_bytes                 # one key copy per rotated term
                res["cases"]["%d_diagonals_n1_%s" % (n_diag, "planner" if n1_arg == 0 else "8")] = r
                del pts, lt
                eng.trim()
    finally:
        eng.close()
    print(json.dumps(res, indent=1))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
