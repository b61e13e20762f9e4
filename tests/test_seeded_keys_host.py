"""Compact (seeded) evaluation-key sets on the host: the header reader (fhelin_evalkeys_params / _info) on "FHELINEC" files built
here from the layout documented in include/fhelin.h ("Seeded evaluation keys"), and its refusals (bad magic or version, payloads
sized like full keys, moduli that differ from the chain, truncation, trailing bytes).  No device needed."""
import struct

import numpy as np
import pytest

ERR_ARG = 1
PRM_FIELDS = ("log_n", "n_q", "first_bits", "scale_bits", "n_p", "special_bits", "dnum", "log_slots", "hamming")
SEED = bytes(range(7, 39))


def build_compact(cfg, moduli, keys, seed=SEED, boot=(0,) * 7, magic=b"FHELINEC", version=1, digest=12345):
    """keys: list of (kind, digits, galois, stored uint64 array); the digest field is not checked by the header reader"""
    nm = len(moduli)
    table_end = 128 + 8 * nm + 40 * len(keys)
    data_offset = -(-table_end // 4096) * 4096
    head = magic + struct.pack("<II", version, len(keys)) + struct.pack("<9i", *[cfg[f] for f in PRM_FIELDS])
    head += struct.pack("<7i", *boot) + struct.pack("<QQ", data_offset, 0) + bytes(seed)
    assert len(head) == 128
    head += np.asarray(moduli, dtype=np.uint64).tobytes()
    at, payload = data_offset, b""
    for kind, digits, g, arr in keys:
        arr = np.ascontiguousarray(arr, dtype=np.uint64)
        head += struct.pack("<IIQQQQ", kind, digits, g, at, arr.size, digest)
        at += arr.nbytes
        payload += arr.tobytes()
    return head + b"\0" * (data_offset - len(head)) + payload


def _toy(fa):
    cfg = dict(fa.PRESETS["toy"])
    e = fa.Engine("toy", device=-1)
    try:
        moduli = [int(m) for m in e.moduli]
        digits = e.dnum_digits
    finally:
        e.close()
    return cfg, moduli, digits


def _b_halves(cfg, moduli, digits, rng):
    """the stored parts of a public key and of a relinearisation / rotation / conjugation key"""
    N, n_q = 1 << cfg["log_n"], cfg["n_q"]
    pk = np.stack([rng.integers(0, q, N, dtype=np.uint64) for q in moduli[:n_q]])
    sw = lambda: np.stack([np.stack([rng.integers(0, q, N, dtype=np.uint64) for q in moduli]) for _ in range(digits)])
    two_n = 2 * N
    return [(0, 0, 0, pk), (1, digits, 0, sw()), (3, digits, two_n - 1, sw()), (2, digits, 5, sw()), (2, digits, 25, sw())]


def _code(fa, path):
    with pytest.raises(fa.FhelinError) as ei:
        fa.Engine.eval_keys_params(str(path))
    return ei.value.code


def test_compact_params_round_trip_from_documented_layout(fa, tmp_path):
    cfg, moduli, digits = _toy(fa)
    keys = _b_halves(cfg, moduli, digits, np.random.default_rng(3))
    p = tmp_path / "toy.evc"
    data = build_compact(cfg, moduli, keys, boot=(3, 3, 1024, 28, 3, 47, 10))
    p.write_bytes(data)
    got, boot, n = fa.Engine.eval_keys_params(str(p))
    assert got == cfg
    assert boot == dict(budget_enc=3, budget_dec=3, slots=1024, K=28, R=3, cheb_degree=47, correction=10)
    assert n == len(keys)
    # exactly half the payload of the full set of the same keys
    N, nm = 1 << cfg["log_n"], len(moduli)
    stored = sum(a.size for *_, a in keys)
    assert stored == cfg["n_q"] * N + 4 * digits * nm * N


@pytest.mark.parametrize("magic,version", [(b"FHELINEX", 1), (b"FHELINEC", 2), (b"FHELINEC", 0), (b"FHELINEK", 1)])
def test_bad_magic_or_version_is_refused(fa, tmp_path, magic, version):
    """FHELINEK version 1 with the compact layout is malformed as a full set too (its payload offset and sizes do not fit)"""
    cfg, moduli, digits = _toy(fa)
    p = tmp_path / "bad.evc"
    p.write_bytes(build_compact(cfg, moduli, _b_halves(cfg, moduli, digits, np.random.default_rng(4)), magic=magic, version=version))
    assert _code(fa, p) == ERR_ARG


@pytest.mark.parametrize("which", [0, 1, 3])
def test_full_size_payload_is_refused(fa, tmp_path, which):
    cfg, moduli, digits = _toy(fa)
    rng = np.random.default_rng(5)
    keys = _b_halves(cfg, moduli, digits, rng)
    kind, d, g, arr = keys[which]
    keys[which] = (kind, d, g, np.concatenate([arr, arr], axis=0))     # sized like a v1 key: b and a
    p = tmp_path / "full.evc"
    p.write_bytes(build_compact(cfg, moduli, keys))
    assert _code(fa, p) == ERR_ARG
    # a digit count other than the stored size's
    keys = _b_halves(cfg, moduli, digits, rng)
    kind, d, g, arr = keys[1]
    keys[1] = (kind, d + 1, g, arr)
    p.write_bytes(build_compact(cfg, moduli, keys))
    assert _code(fa, p) == ERR_ARG


def test_moduli_that_differ_from_the_chain_are_refused(fa, tmp_path):
    cfg, moduli, digits = _toy(fa)
    keys = _b_halves(cfg, moduli, digits, np.random.default_rng(6))
    bad = list(moduli)
    bad[-1] += 2
    p = tmp_path / "mod.evc"
    p.write_bytes(build_compact(cfg, bad, keys))
    assert _code(fa, p) == ERR_ARG


def test_truncated_or_trailing_bytes_are_refused(fa, tmp_path):
    cfg, moduli, digits = _toy(fa)
    data = build_compact(cfg, moduli, _b_halves(cfg, moduli, digits, np.random.default_rng(7)))
    p = tmp_path / "t.evc"
    for blob in (data[:-8], data[:-1], data + b"\0" * 8, data[:100], data[:127], data[:128 + 8 * len(moduli) + 20]):
        p.write_bytes(blob)
        assert _code(fa, p) == ERR_ARG
    p.write_bytes(data)
    fa.Engine.eval_keys_params(str(p))
