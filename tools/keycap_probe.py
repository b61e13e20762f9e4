#!/usr/bin/env python3
"""Level-capped keys at driver scale (include/fhelin.h "Level-capped keys"): the `main` driver at N=2^16 with 28+7 limbs under its
recorded level plan, seeded keys, the full key list (relinearisation, the circuit's rotations, the bootstrap set-up for 16384 slots).
  1. an uncapped client records the level plan, then one applied pass under the usage recorder gives the cap of every key;
  2. capped against uncapped, alternating, --reps times each from a fresh context with the same seed: key generation, the bytes and
     the save time of the full and of the compact set, the load time of each into a fresh evaluation context (warm page cache), all
     device-synchronised;
  3. the applied pass on both (first repetition): logits and final residues compared bit for bit, and the device bytes in use after
     the pass (keys plus their permuted and folded copies, plaintext encodings, whatever the pass left live).
One JSON record; --json writes it (profiles/keycaps_*.json).  Without a GPU it prints "not measured" and exits 0.
  python tools/keycap_probe.py [--preset bench] [--n-q 28] [--n-p 7] [--S 129] [--variant main] [--reps 2] [--dir DIR] [--json out.json]"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def warm(path):
    with open(path, "rb") as f:
        while f.read(64 << 20):
            pass


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--preset", default="bench")
    ap.add_argument("--n-q", type=int, default=28)
    ap.add_argument("--n-p", type=int, default=7)
    ap.add_argument("--S", type=int, default=129)
    ap.add_argument("--variant", default="main")
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--dir", default="")
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    import fhe_linformer_amd as fa
    from fhe_linformer_amd import linformer as lf
    from oracle import plain_forward as pf
    kw = dict(n_q=a.n_q, n_p=a.n_p)
    try:
        probe = fa.Engine(a.preset, seed=1, **kw)
        has_dev = probe.has_device
        probe.close()
    except fa.FhelinError as ex:
        has_dev = False
        print(f"no device: {ex}")
    if not has_dev:
        print("not measured: no GPU")
        return 0
    rots = fa.circuit_rotation_indices()
    w = pf.synthetic_model(1234)
    ins = pf.client_inputs(w, pf.synthetic_tokens(a.S, 300))

    def client(caps):
        t0 = time.perf_counter()
        e = fa.Engine(a.preset, seed=41, **kw)
        e.set_seeded_keys(True)
        if caps is not None:
            e.set_key_caps(caps)
        e.keygen()
        e.gen_relin_key()
        e.gen_rotation_keys(rots)
        e.bootstrap_setup(3, 3, 16384)
        e.sync()
        return e, time.perf_counter() - t0

    def applied_pass(e, plan):
        """the driver under the applied plan, inputs encrypted inside the pass: (caps recorded, logits, final residues, live bytes)"""
        ctl = lf.GpuController(e)
        caps, out = lf.record_key_caps(ctl, w, lambda: lf.encrypt_inputs(ctl, *ins), variant=a.variant, plan=plan)
        res = out.export()
        logits = lf.logits_from_slots(e.decrypt(out))
        e.sync()
        return caps, logits, res, e.cache_stats()["pool_live_bytes"]

    # 1. plan and caps, from an uncapped client (a warm-up of code objects and pools as well)
    e, _ = client(None)
    ctl = lf.GpuController(e)
    e.level_plan_begin("record")
    out = lf.forward_encrypted(ctl, w, lf.encrypt_inputs(ctl, *ins), variant=a.variant)
    e.decrypt(out)
    plan = e.level_plan_end()
    caps = applied_pass(e, plan)[0]
    n_q = e.n_q
    e.close()
    res = {"preset": a.preset, "N": 1 << fa.PRESETS[a.preset]["log_n"], "n_q": a.n_q, "n_p": a.n_p, "S": a.S, "variant": a.variant,
           "rotation_indices": len(rots), "caps": [list(c) for c in caps]}
    hist = {}
    for _, _, m in caps:
        hist[m] = hist.get(m, 0) + 1
    res["cap_histogram"] = {str(k): hist[k] for k in sorted(hist)}
    print(f"{len(caps)} keys used by one {a.variant} pass under its plan; caps (limbs: keys): {res['cap_histogram']}; "
          f"{sum(1 for c in caps if c[2] < n_q)} below n_q = {n_q}")

    # 2. + 3. capped against uncapped, alternating
    series = {"uncapped": [], "capped": []}
    first = {}
    tmp = tempfile.mkdtemp(dir=a.dir or None)
    try:
        for rep in range(a.reps):
            for name, table in (("uncapped", None), ("capped", caps)):
                e, t_gen = client(table)
                rec = {"gen_s": t_gen, "keys_bytes_live": e.cache_stats()["pool_live_bytes"]}
                if rep == 0:
                    _, logits, resid, live = applied_pass(e, plan)
                    first[name] = (logits, resid)
                    rec["live_bytes_after_pass"] = live
                for compact in (False, True):
                    form = "compact" if compact else "full"
                    path = os.path.join(tmp, f"{name}.{form}")
                    e.sync()
                    t0 = time.perf_counter()
                    e.save_eval_keys(path, compact=compact)
                    rec[f"{form}_save_s"] = time.perf_counter() - t0
                    rec[f"{form}_bytes"] = os.path.getsize(path)
                    warm(path)
                    ev = fa.Engine(fa.Engine.eval_keys_params(path)[0], seed=5)
                    try:
                        ev.sync()
                        t0 = time.perf_counter()
                        ev.load_eval_keys(path)
                        ev.sync()
                        rec[f"{form}_load_s"] = time.perf_counter() - t0
                    finally:
                        ev.close()
                    os.remove(path)
                e.close()
                series[name].append(rec)
                print(f"  rep {rep} {name:8s}: gen {rec['gen_s']:.2f} s, keys {rec['keys_bytes_live'] / 1e9:.2f} GB on the device; "
                      f"full {rec['full_bytes'] / 1e9:.3f} GB save {rec['full_save_s']:.2f} s load {rec['full_load_s']:.3f} s; "
                      f"compact {rec['compact_bytes'] / 1e9:.3f} GB save {rec['compact_save_s']:.2f} s load {rec['compact_load_s']:.3f} s"
                      + (f"; live after one pass {rec['live_bytes_after_pass'] / 1e9:.2f} GB" if rep == 0 else ""))
    finally:
        for f in os.listdir(tmp):
            os.remove(os.path.join(tmp, f))
        os.rmdir(tmp)
    res["series"] = series
    res["logits_equal"] = bool(np.array_equal(first["uncapped"][0], first["capped"][0]))
    res["residues_equal"] = bool(np.array_equal(first["uncapped"][1], first["capped"][1]))
    print(f"capped pass against uncapped pass: logits equal {res['logits_equal']}, final residues equal {res['residues_equal']}")
    u, c = series["uncapped"][0], series["capped"][0]
    print(f"bytes capped / uncapped: full {c['full_bytes'] / u['full_bytes']:.4f}, compact {c['compact_bytes'] / u['compact_bytes']:.4f}")
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps({k: v for k, v in res.items() if k != "caps"}))
    return 0 if res["logits_equal"] and res["residues_equal"] else 1


if __name__ == "__main__":
    sys.exit(main())
