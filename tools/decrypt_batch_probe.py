#!/usr/bin/env python3
"""Batched decryption (include/fhelin.h "Batched decryption") at the driver's ring (the `bench` preset, N=2^16, 28 + 7 limbs): B = 1, 4 and 8
fresh ciphertexts at 3 limbs, 16384 slots.  Prints one JSON object with, per B,
  - wall ms of the `decrypt` loop (B downloads, B stream drains, B host decodes) against ONE `decrypt_batch`, alternating, warm, median of
    --reps, and of the same batch with idx = the 20 logit slots;
  - bytes downloaded by each;
  - device-event ms of one `decrypt_batch` (phase, inverse NTT, lift, forward FFT, gather and the copy);
  - whether the batch equalled the loop bit for bit (it must).
Without a GPU it prints "not measured" and exits 0: nothing is estimated on the host.
  python tools/decrypt_batch_probe.py [--reps 9] [--json out.json]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


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
        print(json.dumps({"decrypt_batch_probe": "not measured: no GPU"}))
        return 0
    import fhe_linformer_amd as fa
    from fhe_linformer_amd import linformer as lf
    slots, ell = 16384, 3
    idx = sorted(lf.LOGIT_SLOTS)
    eng = fa.Engine("bench", seed=11, n_q=28, n_p=-1)
    res = {"preset": "bench", "N": eng.N, "n_q": eng.n_q, "n_p": eng.n_p, "slots": slots, "limbs": ell, "reps": a.reps, "n_idx": len(idx)}
    try:
        eng.keygen()
        rng = np.random.default_rng(3)
        cts = eng.encrypt_batch(rng.uniform(-1, 1, (8, slots)), eng.n_q - ell, slots)
        for B in (1, 4, 8):
            part = cts[:B]
            loop = np.stack([eng.decrypt(c, slots) for c in part])          # also the warm-up of every path timed below
            batch = eng.decrypt_batch(part, slots)
            some = eng.decrypt_batch(part, slots, idx=idx)
            r = res["B%d" % B] = {"bit_identical": bool(np.array_equal(loop.view(np.uint64), batch.view(np.uint64))
                                                          and np.array_equal(loop[:, idx].view(np.uint64), some.view(np.uint64)))}
            t_loop, t_batch, t_idx, t_dev = [], [], [], []
            for _ in range(a.reps):                                         # alternating: drift hits all three alike
                eng.sync()
                t0 = time.perf_counter()
                for c in part:
                    eng.decrypt(c, slots)
                t1 = time.perf_counter()
                eng.decrypt_batch(part, slots)
                t2 = time.perf_counter()
                eng.decrypt_batch(part, slots, idx=idx)
                t3 = time.perf_counter()
                t_loop.append((t1 - t0) * 1e3)
                t_batch.append((t2 - t1) * 1e3)
                t_idx.append((t3 - t2) * 1e3)
                eng.timer_start()
                eng.decrypt_batch(part, slots)
                t_dev.append(eng.timer_stop())
            r["wall_ms_decrypt_loop"] = statistics.median(t_loop)
            r["wall_ms_decrypt_batch"] = statistics.median(t_batch)
            r["wall_ms_decrypt_batch_idx"] = statistics.median(t_idx)
            r["wall_ms_spread_loop"] = [min(t_loop), max(t_loop)]
            r["wall_ms_spread_batch"] = [min(t_batch), max(t_batch)]
            r["device_ms_decrypt_batch"] = statistics.median(t_dev)
            r["bytes_loop"] = B * 2 * eng.N * 8                              # two limbs of N words per ciphertext
            r["bytes_batch"] = B * slots * 8
            r["bytes_batch_idx"] = B * len(idx) * 8
    finally:
        eng.close()
    print(json.dumps(res, indent=1))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
