#!/usr/bin/env python3
"""Packed formats at driver scale (include/fhelin.h "Packed formats"): N=2^16 with 28+7 limbs, the `main` driver's key list (seeded
keys, relinearisation, the circuit's rotations, the bootstrap set-up for 16384 slots) under the caps profiles/keycaps_n16.json recorded.
  1. bytes: the capped key set written full, compact, packed full and packed compact (file sizes), the uncapped sets by the formula;
     one sample's wrapped inputs compact against packed; the two-limb sanitised reply plain against packed;
  2. kernel rate: pack and unpack of one switching key's payload and of a batch of 16 ciphertexts, from device events, in unpacked
     GB/s, against a device-to-device copy of the same unpacked bytes timed in the same run, alternating with the kernels;
  3. save and load of the compact capped set, packed against unpacked, alternating, --reps times, a fresh evaluation context for every
     load (warm page cache), all device-synchronised.
It prints what it measures; --json writes the record.  Without a GPU it prints "not measured" and exits 0.
  python tools/packed_probe.py [--reps 5] [--json profiles/packed_probe_n16.json] [--caps profiles/keycaps_n16.json] [--dir DIR]"""
import argparse
import json
import os
import statistics
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
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--json", default="")
    ap.add_argument("--caps", default=os.path.join(ROOT, "profiles", "keycaps_n16.json"))
    ap.add_argument("--dir", default="")
    a = ap.parse_args()
    import fhe_linformer_amd as fa
    from oracle import plain_forward as pf
    kw = dict(n_q=28, n_p=7)
    try:
        probe = fa.Engine("bench", seed=1, **kw)
        has_dev = probe.has_device
        probe.close()
    except fa.FhelinError as ex:
        has_dev = False
        print(f"no device: {ex}")
    if not has_dev:
        print("not measured: no GPU")
        return 0
    caps = [tuple(c) for c in json.load(open(a.caps))["caps"]]
    rots = fa.circuit_rotation_indices()

    def client():
        e = fa.Engine("bench", seed=41, **kw)
        e.set_seeded_keys(True)
        e.set_key_caps(caps)
        e.keygen()
        e.gen_relin_key()
        e.gen_rotation_keys(rots)
        e.bootstrap_setup(3, 3, 16384)
        e.sync()
        return e

    e = client()
    N, n_q, n_p, alpha = e.N, e.n_q, e.n_p, e.alpha
    w = [int(m).bit_length() for m in e.moduli]
    res = {"N": N, "n_q": n_q, "n_p": n_p, "reps": a.reps, "widths": w,
           "bits_per_residue": {"ciphertext_28": sum(w[:n_q]) / n_q, "switching_key_28p7": sum(w) / len(w)}}
    print(f"widths {w}: {res['bits_per_residue']['ciphertext_28']:.2f} bits per ciphertext residue, "
          f"{res['bits_per_residue']['switching_key_28p7']:.2f} per key residue")
    tmp = tempfile.mkdtemp(dir=a.dir or None)
    try:
        # 1. bytes
        sizes = {}
        for name, fn in (("capped_full", lambda p: e.save_eval_keys(p)), ("capped_compact", lambda p: e.save_eval_keys(p, compact=True)),
                         ("capped_packed_full", lambda p: e.save_evalkeys_packed(p)),
                         ("capped_packed_compact", lambda p: e.save_evalkeys_packed(p, compact=True))):
            path = os.path.join(tmp, name)
            fn(path)
            sizes[name] = os.path.getsize(path)
            if name == "capped_compact":
                n_keys = fa.Engine.eval_keys_params(path)[2]
            os.remove(path)
        # uncapped, by the formula: the public key and n_keys - 1 switching keys of dnum digits (4096 bytes of header and table)
        digits, sw = -(-n_q // alpha), n_keys - 1
        sizes["uncapped_full_formula"] = 4096 + 8 * N * (2 * n_q + sw * digits * 2 * (n_q + n_p))
        sizes["uncapped_compact_formula"] = 4096 + 8 * N * (n_q + sw * digits * (n_q + n_p))
        sizes["uncapped_packed_compact_formula"] = 4096 + N // 8 * (sum(w[:n_q]) + sw * digits * sum(w))
        res["key_set_bytes"] = sizes
        print("key sets (bytes):", sizes)
        wm = pf.synthetic_model(1234)
        args = (wm["cls_token"], wm["posEmb"], wm["E_w"], wm["E_b"], wm["F_w"], wm["F_b"])
        ws = e.client_ingest_wrapped(*args, emb=pf.synthetic_tokens(129, 4321))
        res["wrapped_inputs_bytes"] = {"handles": len(ws), "compact": sum(x.compact_bytes() for x in ws),
                                       "packed": sum(x.packed_bytes(seeded=True) for x in ws)}
        reply = e.sanitize(e.encrypt(np.zeros(16384), level=n_q - 3), flood_bits=24, out_ell=2)
        res["reply_bytes"] = {"plain_words": 8 * 2 * 2 * N, "packed": reply.packed_bytes()}
        print("one sample's wrapped inputs:", res["wrapped_inputs_bytes"], " two-limb reply:", res["reply_bytes"])
        del ws, reply

        # 2. kernel rates
        rates = {}
        for name, widths in (("switching_key", (w * 2) * digits), ("ciphertexts_16", (w[:n_q] * 2) * 16)):
            ms = e.debug_pack_rate(widths, reps=a.reps)
            gb = 8e-9 * len(widths) * N
            med = [float(statistics.median(ms[:, k])) for k in range(4)]
            copy = (med[1] + med[3]) / 2
            rates[name] = {"unpacked_bytes": 8 * len(widths) * N, "ms_all": ms.tolist(), "pack_ms": med[0], "unpack_ms": med[2], "copy_ms": copy,
                           "pack_GBps": gb / med[0] * 1e3, "unpack_GBps": gb / med[2] * 1e3, "copy_GBps": gb / copy * 1e3}
            r = rates[name]
            print(f"{name}: {gb:.3f} GB unpacked; pack {r['pack_GBps']:.0f} GB/s, unpack {r['unpack_GBps']:.0f} GB/s, "
                  f"device-to-device copy {r['copy_GBps']:.0f} GB/s (unpacked bytes per second; medians of {a.reps})")
        res["kernel_rate"] = rates

        # 3. save and load, compact capped set, packed against unpacked, alternating
        series = {"unpacked": [], "packed": []}
        for rep in range(a.reps):
            for name in ("unpacked", "packed"):
                path = os.path.join(tmp, name)
                e.sync()
                t0 = time.perf_counter()
                if name == "packed":
                    e.save_evalkeys_packed(path, compact=True)
                else:
                    e.save_eval_keys(path, compact=True)
                rec = {"save_s": time.perf_counter() - t0, "bytes": os.path.getsize(path)}
                warm(path)
                ev = fa.Engine(fa.Engine.eval_keys_params(path)[0], seed=5)
                try:
                    ev.sync()
                    t0 = time.perf_counter()
                    ev.load_eval_keys(path)
                    ev.sync()
                    rec["load_s"] = time.perf_counter() - t0
                finally:
                    ev.close()
                os.remove(path)
                series[name].append(rec)
                print(f"  rep {rep} {name:8s}: {rec['bytes'] / 1e9:.3f} GB, save {rec['save_s']:.3f} s, load {rec['load_s']:.3f} s")
        res["save_load"] = series
    finally:
        e.close()
        for f in os.listdir(tmp):
            os.remove(os.path.join(tmp, f))
        os.rmdir(tmp)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps({k: v for k, v in res.items() if k != "kernel_rate"}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
