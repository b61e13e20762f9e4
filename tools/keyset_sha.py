#!/usr/bin/env python3
"""sha256 of every on-disk form of an evaluation-key set (include/fhelin.h "Evaluation-key sets", "Seeded evaluation keys",
"Level-capped keys", "Packed formats"), from fixed seeds at the `toy` preset (N = 2^12, 6+2 limbs, dnum 3): seeded keys, the
relinearisation key, the conjugation key and rotations 1, 5 and 9.
  full, compact                        "FHELINEK" / "FHELINEC" version 1 (no key capped)
  full_capped, compact_capped          version 2: the relinearisation key capped at 3, rotation 1 at 5 (no multiple of the digit width 2),
                                       rotation 5 at 1
  packed_full, packed_compact          "FHELINEP" of the capped keys
  compact_stride2                      the uncapped compact set of a context at log_slots 10, interleave stride 2 (header word 88)
Two commits that print the same lines write the same files.  --dir keeps the files (for loading one commit's files in another).
Without a GPU it prints "not measured" and exits 0.
  python tools/keyset_sha.py [--dir DIR]"""
import argparse
import hashlib
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROTATIONS = [1, 5, 9]
RELIN_CAP, ROT_CAPS = 3, {1: 5, 5: 1}


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--dir", default="", help="keep the files here")
    a = ap.parse_args()
    import fhe_linformer_amd as fa
    try:
        probe = fa.Engine("toy", seed=1)
        has_dev = probe.has_device
        probe.close()
    except fa.FhelinError as ex:
        has_dev = False
        print(f"no device: {ex}")
    if not has_dev:
        print("not measured: no GPU")
        return 0

    def client(capped, **kw):
        e = fa.Engine("toy", seed=77, **kw)
        e.set_seeded_keys(True)
        if capped:
            g = lambda r: pow(5, r, 2 * e.N)
            e.set_key_caps([(1, 0, RELIN_CAP)] + [(2, g(r), c) for r, c in ROT_CAPS.items()])
        e.keygen()
        e.gen_relin_key()
        e.gen_rotation_keys(ROTATIONS)
        e.gen_conj_key()
        return e

    out = a.dir or tempfile.mkdtemp()
    os.makedirs(out, exist_ok=True)
    sets = []
    e = client(False)
    sets += [("full", e, lambda e, p: e.save_eval_keys(p)), ("compact", e, lambda e, p: e.save_eval_keys(p, compact=True))]
    c = client(True)
    sets += [("full_capped", c, lambda e, p: e.save_eval_keys(p)), ("compact_capped", c, lambda e, p: e.save_eval_keys(p, compact=True)),
             ("packed_full", c, lambda e, p: e.save_evalkeys_packed(p)), ("packed_compact", c, lambda e, p: e.save_evalkeys_packed(p, compact=True))]
    s = client(False, log_slots=10, interleave=2)
    sets += [("compact_stride2", s, lambda e, p: e.save_eval_keys(p, compact=True))]
    try:
        for name, eng, save in sets:
            path = os.path.join(out, name + ".evk")
            save(eng, path)
            data = open(path, "rb").read()
            print(f"{name:16s} {len(data):9d} bytes  sha256 {hashlib.sha256(data).hexdigest()}")
            if not a.dir:
                os.remove(path)
    finally:
        for eng in (e, c, s):
            eng.close()
        if not a.dir:
            os.rmdir(out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
