"""Evaluation-key sets on the host: the header reader (fhelin_evalkeys_params / _info) on files built here from the format
documented in include/fhelin.h, and its refusals (bad magic, bad version, moduli that do not match the parameters, truncated
key table or payload).  No device needed.  The digest is restated here independently of the library."""
import struct

import numpy as np
import pytest

P61 = (1 << 61) - 1
ERR_ARG = 1


def mix32(x):
    """lowbias32 on uint32 (numpy, wrap-around)"""
    x = np.asarray(x, dtype=np.uint64) & 0xFFFFFFFF
    x ^= x >> 16
    x = (x * 0x7FEB352D) & 0xFFFFFFFF
    x ^= x >> 15
    x = (x * 0x846CA68B) & 0xFFFFFFFF
    x ^= x >> 16
    return x


def limb_digest(v):
    v = np.asarray(v, dtype=np.uint64)
    k = mix32(np.arange(v.size, dtype=np.uint64) ^ 0x9E3779B9)
    return int(((v % np.uint64(P61)).astype(object) * k.astype(object)).sum() % P61)


def key_digest(words, N):
    vecs = np.asarray(words, dtype=np.uint64).reshape(-1, N)
    w = mix32(np.arange(vecs.shape[0], dtype=np.uint64) | 0x80000000)
    return sum(limb_digest(v) * int(wj) for v, wj in zip(vecs, w)) % P61


PRM_FIELDS = ("log_n", "n_q", "first_bits", "scale_bits", "n_p", "special_bits", "dnum", "log_slots", "hamming")


def build_set(cfg, moduli, keys, boot=(0,) * 7, magic=b"FHELINEK", version=1):
    """keys: list of (kind, digits, galois, payload uint64 array)"""
    nm = len(moduli)
    table_end = 96 + 8 * nm + 40 * len(keys)
    data_offset = -(-table_end // 4096) * 4096
    head = magic + struct.pack("<II", version, len(keys)) + struct.pack("<9i", *[cfg[f] for f in PRM_FIELDS])
    head += struct.pack("<7i", *boot) + struct.pack("<QQ", data_offset, 0)
    head += np.asarray(moduli, dtype=np.uint64).tobytes()
    at, payload = data_offset, b""
    for kind, digits, g, arr in keys:
        arr = np.ascontiguousarray(arr, dtype=np.uint64)
        head += struct.pack("<IIQQQQ", kind, digits, g, at, arr.size, key_digest(arr, 1 << cfg["log_n"]))
        at += arr.nbytes
        payload += arr.tobytes()
    return head + b"\0" * (data_offset - len(head)) + payload


def _toy_set(fa):
    cfg = dict(fa.PRESETS["toy"])
    e = fa.Engine("toy", device=-1)
    try:
        moduli = [int(m) for m in e.moduli]
    finally:
        e.close()
    N = 1 << cfg["log_n"]
    rng = np.random.default_rng(5)
    pk = np.stack([np.stack([rng.integers(0, q, N, dtype=np.uint64) for q in moduli[: cfg["n_q"]]]) for _ in range(2)])
    return cfg, moduli, [(0, 0, 0, pk)]


def _code(fa, path):
    with pytest.raises(fa.FhelinError) as ei:
        fa.Engine.eval_keys_params(str(path))
    return ei.value.code


def test_params_round_trip_from_documented_format(fa, tmp_path):
    cfg, moduli, keys = _toy_set(fa)
    p = tmp_path / "toy.evk"
    p.write_bytes(build_set(cfg, moduli, keys, boot=(3, 3, 1024, 28, 3, 47, 10)))
    got, boot, n = fa.Engine.eval_keys_params(str(p))
    assert got == cfg
    assert boot == dict(budget_enc=3, budget_dec=3, slots=1024, K=28, R=3, cheb_degree=47, correction=10)
    assert n == 1
    p.write_bytes(build_set(cfg, moduli, keys))
    assert fa.Engine.eval_keys_params(str(p))[1] is None


def test_refuses_bad_magic_version_moduli_and_truncation(fa, tmp_path):
    cfg, moduli, keys = _toy_set(fa)
    p = tmp_path / "bad.evk"
    p.write_bytes(build_set(cfg, moduli, keys, magic=b"FHELINEX"))
    assert _code(fa, p) == ERR_ARG
    p.write_bytes(build_set(cfg, moduli, keys, version=2))
    assert _code(fa, p) == ERR_ARG
    wrong = list(moduli)
    wrong[2] = moduli[3]
    p.write_bytes(build_set(cfg, wrong, keys))
    assert _code(fa, p) == ERR_ARG
    good = build_set(cfg, moduli, keys)
    nm = len(moduli)
    p.write_bytes(good[: 96 + 8 * nm + 20])          # cut inside the key table
    assert _code(fa, p) == ERR_ARG
    p.write_bytes(good[:-8])                          # cut inside the payload
    assert _code(fa, p) == ERR_ARG
    p.write_bytes(good + b"\0" * 8)                   # trailing bytes
    assert _code(fa, p) == ERR_ARG
    p.write_bytes(good)
    assert fa.Engine.eval_keys_params(str(p))[0] == cfg


def test_load_needs_a_device(fa, tmp_path):
    cfg, moduli, keys = _toy_set(fa)
    p = tmp_path / "toy.evk"
    p.write_bytes(build_set(cfg, moduli, keys))
    e = fa.Engine("toy", device=-1)
    try:
        with pytest.raises(fa.FhelinError) as ei:
            e.load_eval_keys(str(p))
        assert ei.value.code == 2      # FHELIN_ERR_NO_DEVICE
    finally:
        e.close()
