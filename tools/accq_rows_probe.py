"""Per-shape A/B of FHELIN_FUSE_ACCQ_ROWS: the single-key key-switch callers at the headline ring (N = 2^16, 28 + 7 limbs,
alpha 7), timed with the engine's device timer on two contexts of ONE process that differ in the knob only - ks_inner over the Q limbs plus
the epilogue row pass that reads accQ back, against the epilogue row pass that forms the Q-limb sums itself (ntt_rows_epilogue_product_kernel).
One ciphertext and batches, ell = 24 and 12, the operand forms: relinearisation (identity), a gathered rotation, rows with their own keys
(rotate_many over 3 and 7 indices, the inputs one after the other).  Prints one JSON line per shape: accQ vectors of the launch
(rows * 2 * ell), ms per call either way, the difference.
    python tools/accq_rows_probe.py [reps]"""
import json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import fhe_linformer_amd as fa

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
ROT3, ROT7 = [128, 256, 384], [1, 2, 3, 4, 5, 6, 7]


def engine(on):
    os.environ["FHELIN_FUSE_ACCQ_ROWS"] = "2" if on else "0"
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
                        "many3": timed(e, lambda: [e.rotate_many(x, ROT3) for x in xs]),
                        "many7": timed(e, lambda: [e.rotate_many(x, ROT7) for x in xs])}
            del xs
        for op, rows in (("relin", 1), ("rotate", 1), ("many3", 3), ("many7", 7)):
            a, b = ms["separate"][op], ms["fused"][op]
            print(json.dumps({"ell": ell, "batch": B, "accq_vectors_per_launch": (B if rows == 1 else rows) * 2 * ell, "op": op,
                              "ms_separate": round(a, 4), "ms_fused": round(b, 4), "diff_us": round(1000 * (b - a), 1)}), flush=True)
