#!/usr/bin/env python3
"""Full against compact (seeded) evaluation-key sets at one preset, with the driver's full key list (keygen, relinearisation, the
circuit's rotations, the bootstrap set-up for 16384 slots).  Prints
  - the regenerate path (context + keygen + relinearisation + rotations + bootstrap set-up, device-synchronised) in default and in
    seeded-key mode;
  - the bytes of the full and of the compact set, and the time to save each;
  - the time to load each into a fresh context, from a warm page cache (each file is read once first), best of --reps.
Without a GPU it prints "not measured" and exits 0: nothing is estimated on the host.
  python tools/evalkeys_probe.py [--preset bench] [--n-q 28] [--n-p 7] [--reps 2] [--dir DIR] [--json out.json]"""
import argparse
import json
import os
import sys
import tempfile
import time

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
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--dir", default="", help="where the sets are written (default: a temporary directory)")
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    import fhe_linformer_amd as fa
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

    def regenerate(seeded):
        t0 = time.perf_counter()
        e = fa.Engine(a.preset, seed=41, **kw)
        if seeded:
            e.set_seeded_keys(True)
        e.keygen()
        e.gen_relin_key()
        e.gen_rotation_keys(rots)
        e.bootstrap_setup(3, 3, 16384)
        e.sync()
        return e, time.perf_counter() - t0

    res = {"preset": a.preset, "n_q": a.n_q, "n_p": a.n_p, "rotation_indices": len(rots)}
    e, _ = regenerate(False)            # warm-up: code objects, pools
    e.close()
    e, t_def = regenerate(False)
    e.close()
    cl, t_seed = regenerate(True)
    res.update(N=cl.N, regen_default_s=t_def, regen_seeded_s=t_seed)
    print(f"{a.preset} N={cl.N} {a.n_q}+{a.n_p} limbs: regenerate (keygen + relin + {len(rots)} rotations + bootstrap set-up): "
          f"default {t_def:.2f} s, seeded {t_seed:.2f} s ({t_seed / t_def:.2f}x)")
    tmp = tempfile.mkdtemp(dir=a.dir or None)
    try:
        for compact in (False, True):
            name = "compact" if compact else "full"
            path = os.path.join(tmp, "set." + name)
            cl.sync()
            t0 = time.perf_counter()
            cl.save_eval_keys(path, compact=compact)
            t_save = time.perf_counter() - t0
            size = os.path.getsize(path)
            n_keys = fa.Engine.eval_keys_params(path)[2]
            warm(path)
            loads = []
            for _ in range(a.reps):
                cfg = fa.Engine.eval_keys_params(path)[0]
                ev = fa.Engine(cfg, seed=5)
                try:
                    ev.sync()
                    t0 = time.perf_counter()
                    ev.load_eval_keys(path)
                    ev.sync()
                    loads.append(time.perf_counter() - t0)
                finally:
                    ev.close()
            os.remove(path)
            res.update({f"{name}_bytes": size, f"{name}_save_s": t_save, f"{name}_load_s": min(loads), "keys": n_keys})
            print(f"  {name:7s} set: {size / 1e9:.3f} GB ({n_keys} keys), save {t_save:.2f} s, load {min(loads):.3f} s "
                  f"(best of {a.reps}, warm cache)")
        print(f"  compact / full bytes: {res['compact_bytes'] / res['full_bytes']:.4f}")
    finally:
        cl.close()
        for f in os.listdir(tmp):
            os.remove(os.path.join(tmp, f))
        os.rmdir(tmp)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
