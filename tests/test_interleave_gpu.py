"""Interleaved samples (include/fhelin.h "Interleaved samples"), bit for bit against the engine's own stride-1 path, which the
oracle already checks.  A TWIN of an engine with n logical slots and stride s is a stride-1 engine with n * s slots, the same seed
and the same calls in the same order (so: the same secret, keys and sampler draws); a logical rotation index r of the first is the
index s * r of the twin.  Exported residues, (npoly, ell, deg) and the 80-bit scale must be EQUAL; only the slot count the
handles report differs (logical n against n * s)."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
LD = np.longdouble
ERR_STATE = 4


def _same(a, b, s, what=""):
    ia, ib = a.info(), b.info()
    assert (ia["npoly"], ia["ell"], ia["deg"]) == (ib["npoly"], ib["ell"], ib["deg"]), (what, ia, ib)
    assert ia["slots"] * s == ib["slots"], (what, "slots are logical", ia["slots"], ib["slots"])
    ha, la = a.scale_parts()
    hb, lb = b.scale_parts()
    assert LD(ha) + LD(la) == LD(hb) + LD(lb), (what, "scale")
    assert np.array_equal(a.export(), b.export()), what


def _code(fa, fn, *a, **kw):
    with pytest.raises(fa.FhelinError) as ei:
        fn(*a, **kw)
    return ei.value.code


def _move(ct, dst, slots=None):
    """a ciphertext into another context of the same parameters, residues and 80-bit scale as they are"""
    inf = ct.info()
    hi, lo = ct.scale_parts()
    buf = dst.upload(ct.export())
    try:
        out = dst.ct_import_device(buf.ptr.value, inf["npoly"], inf["ell"], inf["deg"], hi, lo, inf["slots"] if slots is None else slots)
        dst.sync()
    finally:
        buf.free()
    return out


def _rot_indices(n):
    """logical indices of the rotation tests; n/2 + 1, n - 1 and n + 5 tell a reduction modulo the wrong slot count"""
    single = [1, 3, -1, n // 2 + 1, n - 1, n + 5]
    sums = [2, 4, 6]                                   # {r, 2r, 3r} with r = 2
    tree = [16, 32, 48, 64, -16, -32, -48, -64]        # rotsum / repeat over 8 values, padding 16: steps 16, 32 (+48 merged), 64
    return single, sums, tree


@pytest.fixture(scope="module", params=[("toy", 10, 2), ("toy13", 10, 4)], ids=["toy-s2", "toy13-s4"])
def pair(fa, request):
    preset, log_slots, s = request.param
    A = fa.Engine(preset, seed=4242, log_slots=log_slots, interleave=s)
    B = fa.Engine(preset, seed=4242, log_slots=log_slots + (s.bit_length() - 1))
    n = 1 << log_slots
    single, sums, tree = _rot_indices(n)
    idx = single + sums + tree
    for e, k in ((A, 1), (B, s)):
        e.keygen()
        e.gen_relin_key()
        e.gen_rotation_keys([k * r for r in idx])
    yield A, B, s, n
    A.close()
    B.close()


@pytest.fixture(scope="module")
def cts(fa, pair):
    """one interleaved ciphertext of s different samples on A; the twin encrypts the interleaved vector with the same draws"""
    A, B, s, n = pair
    z = np.random.default_rng(11).uniform(-1, 1, (s, n))
    ca = A.encrypt_interleaved_batch(z[None])[0]
    cb = B.encrypt_batch(fa.interleave(z)[None])[0]
    return z, ca, cb


def test_engine_reports_stride_and_logical_slots(pair, cts):
    A, B, s, n = pair
    _, ca, cb = cts
    assert A.interleave == s and B.interleave == 1
    assert ca.slots == n and cb.slots == n * s
    _same(ca, cb, s, "fresh interleaved encryption: the interleaving draws nothing")
    _same(ca, _move(ca, B, n * s), s, "export / import")


def test_encode_replicates(pair):
    A, B, s, n = pair
    v = np.random.default_rng(5).uniform(-1, 1, n)
    pa, pb = A.encode(v), B.encode(np.repeat(v, s))
    for ell in (A.n_q, 1):
        assert np.array_equal(A.pt_export(pa, ell), B.pt_export(pb, ell)), ell
    full = A.n_q + A.n_p                               # over the full key basis, at an explicit scale
    sc = LD(A.scaling_factors[0])
    assert np.array_equal(A.pt_export(pa, full, sc), B.pt_export(pb, full, sc))
    short = np.array([0.5, -0.25, 0.125])              # fewer values than slots: zero padding, then replicated
    assert np.array_equal(A.pt_export(A.encode(short), 2), B.pt_export(B.encode(np.repeat(short, s)), 2))


def test_encode_on_the_host_encoder(pair):
    A, B, s, n = pair
    v = np.random.default_rng(6).uniform(-1, 1, n)
    A.set_host_encode(True)
    B.set_host_encode(True)
    try:
        assert np.array_equal(A.pt_export(A.encode(v), 2), B.pt_export(B.encode(np.repeat(v, s)), 2))
    finally:
        A.set_host_encode(False)
        B.set_host_encode(False)
    assert np.array_equal(A.pt_export(A.encode(v), 2), B.pt_export(B.encode(np.repeat(v, s)), 2))


def test_rotations(pair, cts):
    A, B, s, n = pair
    _, ca, cb = cts
    single, sums, _ = _rot_indices(n)
    for r in single:
        _same(A.rotate(ca, r), B.rotate(cb, s * r), s, ("rotate", r))
        _same(A.raw_rotate(ca, r), B.raw_rotate(cb, s * r), s, ("raw_rotate", r))
    for x, y in zip(A.rotate_many(ca, single), B.rotate_many(cb, [s * r for r in single])):
        _same(x, y, s, "rotate_many")
    _same(A.rotate_sum([ca], sums)[0], B.rotate_sum([cb], [s * r for r in sums])[0], s, "rotate_sum")
    ra = [A.rotate(ca, r) for r in (1, 3)] + [ca]
    rb = [B.rotate(cb, s * r) for r in (1, 3)] + [cb]
    _same(A.rotate_each_sum(ra, [3, -1, 0]), B.rotate_each_sum(rb, [3 * s, -s, 0]), s, "rotate_each_sum")
    for x, y in zip(A.rotate_each(ra[:2], [-1, 1]), B.rotate_each(rb[:2], [-s, s])):
        _same(x, y, s, "rotate_each")


def test_hoisted_dot(pair, cts):
    A, B, s, n = pair
    _, ca, cb = cts
    rng = np.random.default_rng(8)
    vs = [rng.uniform(-1, 1, n) for _ in range(3)]
    for rescale in (False, True):
        ya = A.hoisted_dot([ca], [A.encode(v) for v in vs], [1, 3], rescale)[0]
        yb = B.hoisted_dot([cb], [B.encode(np.repeat(v, s)) for v in vs], [s, 3 * s], rescale)[0]
        _same(ya, yb, s, ("hoisted_dot", rescale))


def test_rotsum_and_repeat(pair, cts):
    A, B, s, n = pair
    _, ca, cb = cts
    _same(A.rotsum(ca, 8, 16), B.rotsum(cb, 8, 16 * s), s, "fc_rotsum")
    _same(A.repeat(ca, 8, 16), B.repeat(cb, 8, 16 * s), s, "fc_repeat")


def test_every_lane_rotates_by_the_logical_index(pair, cts):
    A, _, s, n = pair
    z, ca, _ = cts
    for r in (3, n + 5):
        got = A.decrypt_interleaved(A.rotate(ca, r))
        assert got.shape == (s, n)
        for i in range(s):
            assert np.max(np.abs(got[i] - np.roll(z[i], -r))) < 1e-7, (r, i)     # tests/test_scheme_gpu.py test_rotation_semantics


def test_round_trip(fa, pair, cts):
    A, B, s, n = pair
    z, ca, cb = cts
    for level in (0, 2, A.n_q - 2, A.n_q - 1):                                      # tests/test_scheme_gpu.py test_encrypt_decrypt_roundtrip
        c = A.encrypt_interleaved_batch(z[None], level=level)[0]
        assert c.level == level
        got = A.decrypt_interleaved(c)
        for i in range(s):
            assert np.max(np.abs(got[i] - z[i])) < 1e-8, (level, i)
    assert np.max(np.abs(B.decrypt(cb, n * s) - fa.interleave(z))) < 1e-8          # the twin sees the interleaved vector
    assert np.max(np.abs(B.decrypt(_move(ca, B, n * s), n * s) - fa.interleave(z))) < 1e-8
    assert np.max(np.abs(A.decrypt(ca) - z[0])) < 1e-8                              # decrypt is lane 0
    assert np.array_equal(A.decrypt(ca), A.decrypt_interleaved(ca)[0])
    assert np.max(np.abs(A.decrypt_flooded(ca, 20) - z[0])) < 1e-6                  # 2^20 / Delta = 2^-32
    # the replicating entry points: every lane gets the values
    v = np.random.default_rng(3).uniform(-1, 1, n)
    for c in (A.encrypt(v), A.encrypt_batch(v[None])[0]):
        got = A.decrypt_interleaved(c)
        for i in range(s):
            assert np.max(np.abs(got[i] - v)) < 1e-8
    # slot-wise operations act lane by lane
    prod = A.decrypt_interleaved(A.mult(ca, A.encode(v)))
    sq = A.decrypt_interleaved(A.mult(ca, ca))
    for i in range(s):
        assert np.max(np.abs(prod[i] - z[i] * v)) < 1e-7                            # tests/test_scheme_gpu.py test_mult_plain_and_cipher
        assert np.max(np.abs(sq[i] - z[i] * z[i])) < 1e-7


def test_refusals(fa, pair):
    A, _, s, n = pair
    assert _code(fa, A.set_interleave, 1) == ERR_STATE                              # after keygen
    assert A.interleave == s
    w = np.zeros((4, 128))
    assert _code(fa, A.client_ingest_wrapped, np.zeros(128), w, np.zeros((32, 8)), np.zeros(32), np.zeros((32, 8)), np.zeros(32),
                 emb=w) == ERR_STATE


# ---- bootstrapping: stride 2 on 1024 logical slots against the twin at 2048 slots, which is full packing (two EvalMods) -----------
@pytest.fixture(scope="module")
def boot_pair(fa):
    A = fa.Engine("boot12", seed=77, log_slots=10, interleave=2)
    B = fa.Engine("boot12", seed=77, log_slots=11)
    for e in (A, B):
        e.keygen()
        e.gen_relin_key()
    A.bootstrap_setup(3, 3, 1024)                      # logical slots: set up for 2048 physical ones
    B.bootstrap_setup(3, 3, 2048)
    yield A, B
    A.close()
    B.close()


def test_bootstrap_set_up_is_the_physical_one(boot_pair):
    A, B = boot_pair
    da, db = A.bootstrap_describe(), B.bootstrap_describe()
    assert da["slots"] == db["slots"] == 2048 and not da["packed"]
    for which in ("c2s", "s2c"):
        assert [[(g, b) for g, b, _ in st["terms"]] for st in da[which]] == [[(g, b) for g, b, _ in st["terms"]] for st in db[which]]
        assert [st["slots"] for st in da[which]] == [st["slots"] for st in db[which]]


def test_bootstrap(fa, boot_pair):
    A, B = boot_pair
    s, n = 2, 1024
    z = np.random.default_rng(21).uniform(-0.5, 0.5, (3, s, n))
    ca = A.encrypt_interleaved_batch(z, level=A.n_q - 3)
    cb = B.encrypt_batch(np.stack([fa.interleave(v) for v in z]), level=B.n_q - 3)
    for x, y in zip(ca, cb):
        _same(x, y, s, "bootstrap input")
    ya, yb = A.bootstrap(ca[0]), B.bootstrap(cb[0])
    _same(ya, yb, s, "bootstrap")
    assert ya.slots == n
    got = A.decrypt_interleaved(ya)
    err = [float(np.max(np.abs(got[i] - z[0, i]))) for i in range(s)]
    print("bootstrap error per lane (N = 2^12, 2048 physical slots):", err)
    for x, y in zip(A.bootstrap_batch(ca[1:]), B.bootstrap_batch(cb[1:])):
        _same(x, y, s, "bootstrap_batch")
    _same(A.bootstrap_iter(ca[0], 8), B.bootstrap_iter(cb[0], 8), s, "bootstrap_iter")


# ---- evaluation-key sets ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("compact", [False, True], ids=["full", "compact"])
def test_key_set_carries_the_stride(fa, tmp_path, compact):
    import struct
    A = fa.Engine("boot12", seed=31, log_slots=10, interleave=2)
    ev = one = None
    try:
        A.set_seeded_keys(compact)
        A.keygen()
        A.gen_relin_key()
        A.gen_rotation_keys([1, -3])
        A.bootstrap_setup(3, 3, 1024)
        path = str(tmp_path / "s2.evk")
        A.save_eval_keys(path, compact=compact)
        head = open(path, "rb").read(96)
        assert struct.unpack_from("<Q", head, 88)[0] == 2
        assert struct.unpack_from("<9i", head, 16)[7] == 10 and struct.unpack_from("<7i", head, 52)[2] == 1024     # both logical
        assert fa.Engine.eval_keys_interleave(path) == 2
        ev = fa.Engine.from_eval_keys(path, seed=5)
        assert ev.interleave == 2
        z = np.random.default_rng(2).uniform(-0.5, 0.5, (1, 2, 1024))
        ct = A.encrypt_interleaved_batch(z, level=A.n_q - 3)[0]
        sv = _move(ct, ev)
        for r in (1, -3):
            _same(A.rotate(ct, r), ev.rotate(sv, r), 1, ("rotate on the loaded set", r))
        _same(A.bootstrap(ct), ev.bootstrap(sv), 1, "bootstrap on the loaded set")
        # a context that was told another stride refuses the file
        one = fa.Engine("boot12", seed=6, log_slots=10)
        one.set_interleave(1)
        assert _code(fa, one.load_eval_keys, path) == ERR_STATE
        assert one.interleave == 1
        os.remove(path)
    finally:
        for e in (A, ev, one):
            if e is not None:
                e.close()


def test_stride_one_key_set_keeps_zero_at_88(fa, tmp_path):
    import struct
    e = fa.Engine("toy", seed=9)
    try:
        e.keygen()
        e.gen_rotation_keys([1])
        path = str(tmp_path / "s1.evk")
        e.save_eval_keys(path)
        assert struct.unpack_from("<Q", open(path, "rb").read(96), 88)[0] == 0
        assert fa.Engine.eval_keys_interleave(path) == 1
        os.remove(path)
    finally:
        e.close()
