"""Per-shape A/B of FHELIN_FUSE_ACCP_ROWS: the key-switch callers at the headline ring (N = 2^16, 28 + 7 limbs, alpha 7), timed
with the engine's device timer on two contexts of ONE process that differ in the knob only - the separate launches (ks_inner over Q and P,
the inverse row pass of accP, its column pass) against the Q-only inner product plus ntt_rows_product_kernel.  One ciphertext and batches,
ell = 24 and 12 (ks_probe.py's levels), the three operand forms: relinearisation (identity), a gathered rotation, merged sums of 3 and 7
rotations.  Prints one JSON line per shape: accP vectors of the launch (batch * 2 * k), ms per call either way, the difference.
    python tools/accp_rows_probe.py [reps]"""
import json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import fhe_linformer_amd as fa

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
ROT3, ROT7 = [128, 256, 384], [1, 2, 3, 4, 5, 6, 7]


def engine(on):
    os.environ["FHELIN_FUSE_ACCP_ROWS"] = "2" if on else "0"   # 2: the merged sums too
    os.environ["FHELIN_ACCP_ROWS_MIN_VECS"] = "0"
    e = fa.Engine("bench", seed=5, n_q=28, n_p=7)
    e.keygen()
    e.gen_relin_key()
    e.gen_rotation_keys(sorted(set(ROT3 + ROT7)))
    return e


es = {"separate": engine(False), "fused": engine(True)}
ns = 1 << es["fused"].params.log_slots
rng = np.random.default_rng(1)


def timed(e, fn):
    for _ in range(2):
        fn()
    e.sync()
    e.timer_start()
    for _ in range(reps):
        fn()
    return e.timer_stop() / reps


for ell in (24, 12):
    for B in (1, 2, 4, 8, 16):
        ms = {}
        for name, e in es.items():
            xs = e.encrypt_batch(rng.uniform(-1, 1, (B, ns)), level=e.n_q - ell)
            ms[name] = {"relin": timed(e, lambda: e.mult_batch(xs, xs)),
                        "rotate": timed(e, lambda: e.rotate_batch(xs, 128)),
                        "sum3": timed(e, lambda: e.rotate_sum(xs, ROT3)),
                        "sum7": timed(e, lambda: e.rotate_sum(xs, ROT7))}
            del xs
        for op in ("relin", "rotate", "sum3", "sum7"):
            a, b = ms["separate"][op], ms["fused"][op]
            print(json.dumps({"ell": ell, "batch": B, "accp_vectors": B * 2 * es["fused"].n_p, "op": op, "ms_separate": round(a, 4),
                              "ms_fused": round(b, 4), "diff_us": round(1000 * (b - a), 1)}), flush=True)
