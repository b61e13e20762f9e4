#!/usr/bin/env python3
"""Compact ciphertexts at the driver's ring (the `bench` preset, N=2^16) on one sample of the driver: 194 inputs (S = 129 tokens,
fhelin_client_ingest).  Prints
  - bytes per sample: full ciphertexts against compact blobs;
  - fhelin_client_ingest in public-key mode against seeded mode (warm, device-synchronised, median of --reps);
  - import_compact of the 194 blobs, and a plain host->device copy of the same bytes from the same pageable memory beside it;
  - the expansion kernel alone for the import's shape (device events), as lane-ops/s and bytes/s against the MI355X peaks.
Without a GPU it prints "not measured" and exits 0: nothing is estimated on the host.
  python tools/compact_probe.py [--reps 10] [--json out.json]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# VALU instructions per thread of seeded_expand_kernel = per ChaCha20 block (four residues): the gfx950 ISA of kernels_seeded.hip
# counted with tools/isa_count.py (20 rounds ~ 970 add / xor / alignbit, the rest the four 128-bit Barrett reductions and addressing)
VALU_PER_BLOCK = 1294
# MI355X peaks (MI355X_MICROARCH.md): 256 CUs x 4 SIMD-32 x 64 lanes per 2 cycles at 2.4 GHz; HBM 8.0 TB/s spec, 6.29 measured
PEAK_LANE_OPS = 256 * 4 * 32 * 2.4e9
PEAK_HBM_SPEC, PEAK_HBM_MEAS = 8.0e12, 6.29e12


def median_ms(eng, fn, reps):
    out = []
    for _ in range(reps):
        eng.sync()
        t0 = time.perf_counter()
        r = fn()
        eng.sync()
        out.append(1e3 * (time.perf_counter() - t0))
        del r
    return statistics.median(out)


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    import numpy as np
    import fhe_linformer_amd as fa
    from fhe_linformer_amd import linformer as lf
    from oracle import plain_forward as pf
    try:
        eng = fa.Engine("bench", seed=21)
        has_dev = eng.has_device
    except fa.FhelinError as ex:
        eng, has_dev = None, False
        print(f"no device: {ex}")
    if not has_dev:
        print("not measured: no GPU")
        return 0
    res = {"preset": "bench", "N": eng.N, "n_q": eng.n_q}
    try:
        eng.keygen()
        ctl = lf.GpuController(eng)
        w = pf.synthetic_model(1234)
        x_emb = pf.synthetic_tokens(129, 4321)

        def ingest():
            enc = lf.ingest_sample(ctl, w, x_emb)
            return enc["inputs_E"] + enc["inputs_F"] + enc["inputs"]

        # bytes per sample
        eng.set_seeded_encryption(True)
        cts = ingest()
        blobs = [c.export_compact() for c in cts]
        full = sum(2 * c.info()["ell"] * eng.N * 8 for c in cts)
        compact = sum(map(len, blobs))
        res.update(inputs=len(cts), full_bytes=full, compact_bytes=compact, ratio=compact / full)
        print(f"bytes per sample ({len(cts)} inputs): full {full / 1e9:.3f} GB, compact {compact / 1e9:.3f} GB ({compact / full:.4f})")
        del cts

        # ingest, public-key against seeded (warm: one of each first; alternating)
        t = {True: [], False: []}
        for mode in (False, True):
            eng.set_seeded_encryption(mode)
            ingest()
        for _ in range(a.reps):
            for mode in (False, True):
                eng.set_seeded_encryption(mode)
                t[mode].append(median_ms(eng, ingest, 1))
        pk, sk = statistics.median(t[False]), statistics.median(t[True])
        res.update(ingest_pk_ms=pk, ingest_seeded_ms=sk)
        print(f"client_ingest (194 outputs), median of {a.reps}: public-key {pk:.2f} ms, seeded {sk:.2f} ms ({sk / pk:.3f}x)")

        # import_compact, and a host->device copy of the same bytes from pageable memory
        eng.import_compact(blobs)
        imp = median_ms(eng, lambda: eng.import_compact(blobs), a.reps)
        host = np.frombuffer(b"".join(blobs), dtype=np.uint8)
        buf = eng.buf(host.nbytes)
        try:
            buf.upload(host)
            h2d = median_ms(eng, lambda: buf.upload(host), a.reps)
        finally:
            buf.free()
        res.update(import_ms=imp, h2d_same_bytes_ms=h2d)
        print(f"import_compact ({len(blobs)} blobs, one call), median of {a.reps}: {imp:.2f} ms; host->device copy of the same "
              f"{host.nbytes / 1e9:.3f} GB alone {h2d:.2f} ms ({host.nbytes / h2d / 1e6:.1f} GB/s); the rest (header checks, "
              f"digest, expansion, allocation) {imp - h2d:.2f} ms")

        # the expansion kernel alone, the import's shape: 194 ciphertexts of n_q limbs
        ells = [fa.compact_info(b)["ell"] for b in blobs]
        ell, n_ct = max(ells), len(blobs)
        _, kms = eng.debug_seeded_expand(bytes(range(32)), 0, ell, n_ct, reps=20, download=False)
        blocks = n_ct * ell * eng.N // 4
        wbytes = blocks * 32
        lane_ops = blocks * VALU_PER_BLOCK   # one thread per block: lane-ops = threads x VALU instructions per thread
        t_valu, t_hbm = lane_ops / PEAK_LANE_OPS, wbytes / PEAK_HBM_MEAS
        res.update(expand_ms=kms, expand_lane_ops=lane_ops, expand_bytes=wbytes, expand_ops_rate=lane_ops / (kms * 1e-3),
                   expand_bytes_rate=wbytes / (kms * 1e-3), floor_valu_ms=1e3 * t_valu, floor_hbm_ms=1e3 * t_hbm)
        print(f"seeded_expand ({n_ct} x {ell} limbs, mean of 20 launches): {kms:.3f} ms; {lane_ops:.3e} lane-ops -> "
              f"{lane_ops / (kms * 1e-3) / 1e12:.1f} T lane-ops/s ({100 * t_valu * 1e3 / kms:.0f} % of the {PEAK_LANE_OPS / 1e12:.1f} T VALU peak); "
              f"{wbytes / 1e9:.3f} GB written -> {wbytes / (kms * 1e-3) / 1e12:.2f} TB/s ({100 * t_hbm * 1e3 / kms:.0f} % of the measured "
              f"{PEAK_HBM_MEAS / 1e12:.2f} TB/s); floors: VALU {1e3 * t_valu:.3f} ms, HBM {1e3 * t_hbm:.3f} ms -> "
              f"{'VALU' if t_valu > t_hbm else 'HBM'}-bound")
    finally:
        eng.close()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
