"""Sparse-secret bootstrapping on the host (include/fhelin.h "Sparse-secret bootstrapping"): the knob's range and getter, what it
writes into the bootstrap configuration, the environment knob, the cap table's and fhelin_key_info's view of the two new kinds, and the
key-set reader on tables with the two new entry kinds, built here from the documented format.  No device needed."""
import struct

import numpy as np
import pytest

from test_keycaps_host import _toy, build_set_v2

ERR_ARG, ERR_STATE, ERR_KEY = 1, 4, 5
H = 32


def _code(fa, fn, *a):
    with pytest.raises(fa.FhelinError) as ei:
        fn(*a)
    return ei.value.code


def _host(fa, monkeypatch, env=None):
    if env is None:
        monkeypatch.delenv("FHELIN_BOOT_SPARSE_H", raising=False)
    else:
        monkeypatch.setenv("FHELIN_BOOT_SPARSE_H", env)
    return fa.Engine("boot12", device=-1)


def test_range_getter_and_default(fa, monkeypatch):
    e = _host(fa, monkeypatch)
    try:
        assert e.bootstrap_sparse_secret() == 0                      # off is the default
        for bad in (7, -1, 1, e.N + 1):
            assert _code(fa, e.set_bootstrap_sparse_secret, bad) == ERR_ARG, bad
            assert e.bootstrap_sparse_secret() == 0
        for ok in (8, H, 192, e.N):
            e.set_bootstrap_sparse_secret(ok)
            assert e.bootstrap_sparse_secret() == ok
        e.set_bootstrap_sparse_secret(0)
        assert e.bootstrap_sparse_secret() == 0
    finally:
        e.close()


def test_environment_knob(fa, monkeypatch):
    e = _host(fa, monkeypatch, str(H))
    try:
        assert e.bootstrap_sparse_secret() == H
    finally:
        e.close()
    for ignored in ("7", "0", "junk", str(1 << 20)):
        e = _host(fa, monkeypatch, ignored)
        try:
            assert e.bootstrap_sparse_secret() == 0, ignored
        finally:
            e.close()


def test_no_device_refusals_and_describe(fa, monkeypatch):
    e = _host(fa, monkeypatch)
    try:
        e.set_bootstrap_sparse_secret(H)
        # nothing is set up on a context without a device: describe has no trailer to show, the hook no secret
        assert _code(fa, e.bootstrap_describe) == ERR_STATE
        assert _code(fa, e.boot_sparse_secret) == ERR_STATE
        assert _code(fa, e.bootstrap_setup, 3, 3, 1024) != 0
        e.set_bootstrap_sparse_secret(64)                            # the set-up did not happen: the knob is still free
        assert e.bootstrap_sparse_secret() == 64
    finally:
        e.close()


def test_key_kinds_without_keys(fa, monkeypatch):
    e = _host(fa, monkeypatch)
    try:
        for kind in (3, 4):
            assert _code(fa, e.key_info, kind, 0) == ERR_ARG         # the knob's kinds: unknown without it
        e.set_bootstrap_sparse_secret(H)
        for kind in (3, 4):
            assert _code(fa, e.key_info, kind, 0) == ERR_KEY         # known, not made
        assert _code(fa, e.key_info, 5, 0) == ERR_ARG
        # the cap table takes both kinds as the usage recorder reports them (the to-sparse entry is accepted and that key still held at two limbs)
        e.set_key_caps([(4, 0, 2), (5, 0, 9)])
        e.set_key_caps([(1, 0, 3), (4, 0, e.n_q), (5, 0, e.n_q)])
        for bad in ([(5, 1, 9)], [(4, 2 * e.N - 1, 2)], [(6, 0, 9)], [(5, 0, 0)], [(4, 0, e.n_q + 1)], [(5, 0, 3), (5, 0, 4)]):
            assert _code(fa, e.set_key_caps, bad) == ERR_ARG, bad
        e.set_bootstrap_sparse_secret(0)                             # ... and neither with the knob off, as before
        for bad in ([(4, 0, 2)], [(5, 0, 9)]):
            assert _code(fa, e.set_key_caps, bad) == ERR_ARG, bad
    finally:
        e.close()


# ---- the depth the bootstrap counts for its cosine fit ---------------------------------------------------------------------------
def test_cheb_depth_is_what_the_evaluation_spends(fa, orc):
    """Evaluator::cheb_depth (fhelin_debug_cheb_depth) against the limbs oracle/residue_eval.py's eval_chebyshev - the residue-exact mirror
    of the library's evaluator - really leaves behind, at the degrees on both sides of every step: 28 is the largest degree in five levels
    (29 and 31 take six), 60 the largest in six, 120 in seven"""
    from oracle.residue_eval import RCt
    from test_boot_residue_gpu import _rev, _uniform_ct, _uniform_key
    e = fa.Engine("boot12", seed=9, device=-1)
    try:
        rev = _rev(e, {"relin": _uniform_key(orc, e, 31)})
        ell = 10
        x = _uniform_ct(orc, e, 40, ell)
        for degree, want in ((5, 3), (13, 4), (14, 4), (15, 5), (27, 5), (28, 5), (29, 6), (31, 6), (47, 6), (59, 6), (60, 6),
                             (61, 7), (119, 7), (120, 7)):
            n, j = degree + 1, np.arange(degree + 1)
            fx = np.cos(3 * np.cos(np.pi * (j + 0.5) / n) + 0.3)                       # no vanishing coefficient
            coeffs = [float(2.0 / n * np.sum(fx * np.cos(np.pi * k * (j + 0.5) / n))) for k in range(n)]
            out = rev.eval_chebyshev(RCt(x, 1, rev.sf[e.n_q - ell]), coeffs, -1.0, 1.0)
            spent = ell - (out.ell - (1 if out.deg >= 2 else 0))
            assert fa.cheb_depth(degree) == spent == want, (degree, fa.cheb_depth(degree), spent, want)
        with pytest.raises(fa.FhelinError) as ei:
            fa.cheb_depth(0)
        assert ei.value.code == ERR_ARG
    finally:
        e.close()


# ---- the key-set reader on the two new entry kinds ----------------------------------------------------------------------------------
def _keys(cfg, alpha, rng, sparse=True, cap_to=2):
    """(kind, digits, galois, max_ell, payload) as build_set_v2 takes them, in storage order: public, relinearisation, conjugation, the
    two sparse-secret keys, one rotation"""
    N, n_q, n_p = 1 << cfg["log_n"], cfg["n_q"], cfg["n_p"]

    def key(kind, g, max_ell):
        digits = -(-max_ell // alpha)
        return (kind, digits, g, max_ell, rng.integers(0, 1 << 40, (digits, 2, max_ell + n_p, N), dtype=np.uint64))

    keys = [(0, 0, 0, n_q, rng.integers(0, 1 << 40, (2, n_q, N), dtype=np.uint64)), key(1, 0, n_q), key(3, 2 * N - 1, n_q)]
    if sparse:
        keys += [key(4, 0, cap_to), key(5, 0, n_q)]
    return keys + [key(2, 5, n_q)]


def _patch_last_word(data, cfg, moduli, kinds, value):
    """the 48-byte entries' last word set on the entries of the given kinds"""
    b = bytearray(data)
    table = 96 + 8 * len(moduli)
    n_keys = struct.unpack_from("<I", b, 12)[0]
    for k in range(n_keys):
        if struct.unpack_from("<I", b, table + 48 * k)[0] in kinds:
            struct.pack_into("<I", b, table + 48 * k + 44, value)
    return bytes(b)


def test_reader_accepts_and_refuses_sparse_entries(fa, tmp_path):
    cfg, moduli, alpha = _toy(fa)
    rng = np.random.default_rng(5)
    N = 1 << cfg["log_n"]
    p = tmp_path / "sparse.evk"
    good = _patch_last_word(build_set_v2(cfg, moduli, _keys(cfg, alpha, rng)), cfg, moduli, (4, 5), H)
    p.write_bytes(good)
    got, boot, n = fa.Engine.eval_keys_params(str(p))
    assert got == cfg and boot is None and n == 6

    def refused(data):
        p.write_bytes(data)
        with pytest.raises(fa.FhelinError) as ei:
            fa.Engine.eval_keys_params(str(p))
        return ei.value.code == ERR_ARG

    plain = build_set_v2(cfg, moduli, _keys(cfg, alpha, rng))
    assert refused(plain)                                                                  # no Hamming weight on the two entries
    assert refused(_patch_last_word(plain, cfg, moduli, (4, 5), 7))                        # below 8
    assert refused(_patch_last_word(plain, cfg, moduli, (4, 5), N + 1))                    # above N
    assert refused(_patch_last_word(_patch_last_word(plain, cfg, moduli, (4,), H), cfg, moduli, (5,), H + 1))   # two weights
    assert refused(_patch_last_word(good, cfg, moduli, (1,), H))                           # the word stays zero on every other kind
    one = [k for k in _keys(cfg, alpha, rng) if k[0] != 5]
    assert refused(_patch_last_word(build_set_v2(cfg, moduli, one), cfg, moduli, (4,), H))                      # one key without the other
    wide = _keys(cfg, alpha, rng, cap_to=3)
    assert refused(_patch_last_word(build_set_v2(cfg, moduli, wide), cfg, moduli, (4, 5), H))                   # the to-sparse key at three limbs
    # a set without the two kinds reads as it always did
    p.write_bytes(build_set_v2(cfg, moduli, _keys(cfg, alpha, rng, sparse=False)))
    assert fa.Engine.eval_keys_params(str(p))[2] == 4
