"""Level-capped keys on the host (include/fhelin.h "Level-capped keys"): the argument and state errors of fhelin_ctx_set_key_caps,
the version 2 key table through fhelin_evalkeys_params / _info on sets built here from the documented format, and the reader's
refusals of malformed version 2 tables.  No device needed."""
import struct

import numpy as np
import pytest

from test_evalkeys_host import PRM_FIELDS, key_digest

ERR_ARG, ERR_STATE, ERR_KEY = 1, 4, 5


def _code(fa, fn, *a):
    with pytest.raises(fa.FhelinError) as ei:
        fn(*a)
    return ei.value.code


def test_set_key_caps_argument_errors(fa):
    e = fa.Engine("toy", device=-1)
    try:
        two_n, n_q = 2 * e.N, e.n_q
        g3 = e.galois_of(3)
        assert g3 == pow(5, 3, two_n)
        assert e.galois_of(-1) == pow(5, e.N // 2 - 1, two_n)
        ok = [(1, 0, 2), (2, g3, 3), (3, two_n - 1, 5)]
        e.set_key_caps(ok)
        e.set_key_caps([(2, g3, n_q)])       # a second call replaces the table; max_ell = n_q is "uncapped"
        e.set_key_caps([])                   # and an empty one clears it
        for bad in ([(0, 0, 2)], [(4, 0, 2)],                         # kind
                    [(1, 0, 0)], [(1, 0, n_q + 1)], [(2, g3, -1)],    # max_ell
                    [(1, 5, 2)], [(3, g3, 2)], [(2, 4, 2)], [(2, two_n - 1, 2)], [(2, two_n + 1, 2)], [(2, 1, 2)],   # galois
                    [(2, g3, 2), (1, 0, 2), (2, g3, 3)]):             # duplicate
            assert _code(fa, e.set_key_caps, bad) == ERR_ARG, bad
        # a refused table changes nothing: the one before it is still in force - visible only through generation (GPU tests);
        # here: the call after a refusal still succeeds
        e.set_key_caps(ok)
    finally:
        e.close()


def test_key_info_and_usage_without_keys(fa):
    e = fa.Engine("toy", device=-1)
    try:
        for kind in (0, 1, 2):
            assert _code(fa, e.key_info, kind, 1) == ERR_KEY
        assert _code(fa, e.key_info, 3, 0) == ERR_ARG
        with e.key_usage() as u:
            pass
        assert u.table == []
    finally:
        e.close()


def test_caps_from_usage(fa):
    t = [(1, 0, 3), (2, 25, 6), (3, 8191, 2)]
    assert fa.caps_from_usage(t, 6) == t
    assert fa.caps_from_usage(t, 6, margin=1) == [(1, 0, 4), (2, 25, 6), (3, 8191, 3)]


# ---- version 2 headers built from the documented format

def build_set_v2(cfg, moduli, keys, magic=b"FHELINEK", version=2, reserved=0):
    """keys: list of (kind, digits, galois, max_ell, payload uint64 array); 48-byte entries"""
    nm = len(moduli)
    head_len = 128 if magic == b"FHELINEC" else 96
    table_end = head_len + 8 * nm + 48 * len(keys)
    data_offset = -(-table_end // 4096) * 4096
    head = magic + struct.pack("<II", version, len(keys)) + struct.pack("<9i", *[cfg[f] for f in PRM_FIELDS])
    head += struct.pack("<7i", *([0] * 7)) + struct.pack("<QQ", data_offset, 0)
    if head_len == 128:
        head += bytes(range(32))
    head += np.asarray(moduli, dtype=np.uint64).tobytes()
    at, payload = data_offset, b""
    for kind, digits, g, max_ell, arr in keys:
        arr = np.ascontiguousarray(arr, dtype=np.uint64)
        head += struct.pack("<IIQQQQII", kind, digits, g, at, arr.size, key_digest(arr, 1 << cfg["log_n"]), max_ell, reserved)
        at += arr.nbytes
        payload += arr.tobytes()
    return head + b"\0" * (data_offset - len(head)) + payload


def _toy(fa):
    cfg = dict(fa.PRESETS["toy"])
    e = fa.Engine("toy", device=-1)
    try:
        moduli = [int(m) for m in e.moduli]
        alpha = e.alpha
    finally:
        e.close()
    return cfg, moduli, alpha


def _keys(cfg, moduli, alpha, caps, halves=2, digits_of=None):
    """a public key and one rotation key per cap (Galois elements 5, 25, ...), payloads of the version 2 size"""
    N, n_q, n_p = 1 << cfg["log_n"], cfg["n_q"], cfg["n_p"]
    rng = np.random.default_rng(11)
    keys = [(0, 0, 0, n_q, rng.integers(0, 1 << 40, (halves, n_q, N), dtype=np.uint64))]
    for i, cap in enumerate(caps):
        digits = digits_of(cap) if digits_of else -(-cap // alpha)
        keys.append((2, digits, pow(5, i + 1, 2 * N), cap, rng.integers(0, 1 << 40, (digits, halves, cap + n_p, N), dtype=np.uint64)))
    return keys


def _params_code(fa, path):
    return _code(fa, fa.Engine.eval_keys_params, str(path))


@pytest.mark.parametrize("magic,halves", [(b"FHELINEK", 2), (b"FHELINEC", 1)])
def test_version2_header_is_read(fa, tmp_path, magic, halves):
    cfg, moduli, alpha = _toy(fa)
    assert alpha == 2
    p = tmp_path / "caps.evk"
    # caps 1, 2, 3, 5 -> 1, 1, 2, 3 digits (a partial and a full last digit); n_q: an uncapped key in a version 2 table
    keys = _keys(cfg, moduli, alpha, (1, 2, 3, 5, cfg["n_q"]), halves)
    assert [k[1] for k in keys[1:]] == [1, 1, 2, 3, 3]
    p.write_bytes(build_set_v2(cfg, moduli, keys, magic=magic))
    got, boot, n = fa.Engine.eval_keys_params(str(p))
    assert got == cfg and boot is None and n == len(keys)


def test_version2_refusals(fa, tmp_path):
    cfg, moduli, alpha = _toy(fa)
    n_q, n_p, N = cfg["n_q"], cfg["n_p"], 1 << cfg["log_n"]
    p = tmp_path / "bad.evk"
    good = _keys(cfg, moduli, alpha, (3,))
    p.write_bytes(build_set_v2(cfg, moduli, good))
    assert fa.Engine.eval_keys_params(str(p))[2] == 2
    # a non-zero reserved word
    p.write_bytes(build_set_v2(cfg, moduli, good, reserved=1))
    assert _params_code(fa, p) == ERR_ARG
    # max_ell outside 1 .. n_q (the payload sized for the claimed cap, so only max_ell is wrong)
    for cap in (0, n_q + 1):
        kind, digits, g, _, _ = good[1]
        arr = np.zeros((max(1, -(-cap // alpha)), 2, cap + n_p, N), dtype=np.uint64)
        p.write_bytes(build_set_v2(cfg, moduli, [good[0], (kind, arr.shape[0], g, cap, arr)]))
        assert _params_code(fa, p) == ERR_ARG, cap
    # the public key must carry n_q
    pk = good[0]
    p.write_bytes(build_set_v2(cfg, moduli, [(pk[0], pk[1], pk[2], n_q - 1, pk[4]), good[1]]))
    assert _params_code(fa, p) == ERR_ARG
    # digits != digits_at(max_ell): cap 3 is two digits; one and three are refused (payload sized for the claimed digits)
    for digits in (1, 3):
        bad = _keys(cfg, moduli, alpha, (3,), digits_of=lambda cap: digits)
        p.write_bytes(build_set_v2(cfg, moduli, bad))
        assert _params_code(fa, p) == ERR_ARG, digits
    # words that do not match: the version 1 size (full rows) under a cap
    kind, digits, g, cap, _ = good[1]
    p.write_bytes(build_set_v2(cfg, moduli, [good[0], (kind, digits, g, cap, np.zeros((digits, 2, n_q + n_p, N), dtype=np.uint64))]))
    assert _params_code(fa, p) == ERR_ARG
    # a version the reader does not know
    p.write_bytes(build_set_v2(cfg, moduli, good, version=3))
    assert _params_code(fa, p) == ERR_ARG
    p.write_bytes(build_set_v2(cfg, moduli, good))
    assert fa.Engine.eval_keys_params(str(p))[0] == cfg
