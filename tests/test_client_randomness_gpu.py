"""Client-side randomness pinned term by term (include/fhelin.h "Sampler streams"): everything that draws randomness on the GPU is a
deterministic function of a ChaCha20 key, a stream number and a position, and fhelin_debug_sampler_peek tells which keys and which
counter a call is about to use.  So every term is compared EXACTLY with tests/sampler_model.py, which is written against the header's
text: the small sampler's polynomials; u, e0 and e1 of public-key encryptions (single, and a batch that crosses the chunk of 32);
u, e0 + f and e1 of sanitised replies (0 / 1 / 24 / 52 flood bits, mixed limb counts, a second chunk, under a mask, on an evaluation
context); the flood polynomial of a flooded decryption; the noise of seeded encryptions, of the seeded public key and of seeded
switching keys.  Every comparison is np.array_equal on residues (exact doubles for the decryption); every Gaussian comparison asserts
that no coefficient of the model lies in its rounding guard band."""
import numpy as np
import pytest

import sampler_model as sm
from sampler_model import chacha20_words
from test_compact_gpu import _noise, header
from test_seeded_keys_gpu import _small, key_noise, payload, read_table

pytestmark = pytest.mark.gpu


def _public_key(eng, path):
    """[2][n_q][N] from a saved evaluation-key set (its first payload), as tests/test_seeded_keys_gpu.py reads it"""
    eng.save_eval_keys(path)
    data = open(path, "rb").read()
    ent = read_table(data)[0]
    assert ent["kind"] == 0 and ent["words"] == 2 * eng.n_q * eng.N
    return payload(data, ent).reshape(2, eng.n_q, eng.N).copy()


def _import_exact(eng, limbs, like):
    """limbs as a handle with `like`'s degree, slots and exact (80-bit) scale"""
    inf = like.info()
    hi, lo = like.scale_parts()
    limbs = np.ascontiguousarray(limbs, dtype=np.uint64)
    buf = eng.upload(limbs)
    try:
        out = eng.ct_import_device(buf.ptr.value, limbs.shape[0], limbs.shape[1], inf["deg"], hi, lo, inf["slots"])
        eng.sync()
    finally:
        buf.free()
    return out


def _after(eng, calls, key):
    """the counter reads `calls` and the next key draw is `key`: the call drew exactly the keys the text lists"""
    k, c = eng.debug_sampler_peek(1)
    assert c == calls and np.array_equal(k[0], key)


@pytest.fixture(scope="module")
def toy(fa, tmp_path_factory):
    """one keyed toy client (N = 2^12, 6 + 2 limbs, non-zero seed), its public key and the file it was read from"""
    eng = fa.Engine("toy", seed=31)
    eng.keygen()
    path = str(tmp_path_factory.mktemp("rand") / "toy.evk")
    pk = _public_key(eng, path)
    yield eng, pk, path
    eng.close()


@pytest.fixture(scope="module")
def bench(fa, tmp_path_factory):
    eng = fa.Engine("bench", seed=32)
    eng.keygen()
    pk = _public_key(eng, str(tmp_path_factory.mktemp("rand") / "bench.evk"))
    yield eng, pk
    eng.close()


# ---------------------------------------------------------------------------------------------------------------- the small sampler
@pytest.mark.parametrize("preset", ["toy", "bench"])      # bench: N = 2^16, 32 workgroups, block counters above 255
def test_small_sampler_equals_the_model(fa, preset):
    eng = fa.Engine(preset, seed=17)
    try:
        for kind in (1, 0):
            keys, calls = eng.debug_sampler_peek(2)
            got = eng.debug_sample(kind, 3)
            for p in range(3):
                if kind == 1:
                    want = sm.ternary(keys[0], sm.stream_of(calls, p), eng.N)
                else:
                    want, banded = sm.gaussian(keys[0], sm.stream_of(calls, p), eng.N)
                    assert banded == 0
                assert np.array_equal(got[p], want), (kind, p)
            _after(eng, calls + 1, keys[1])
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------------------ public-key encryption
def _fresh_zero(orc, eng, pk, keys, calls, n, ell):
    """the encryptions of zero of one public-key encryption call of n vectors at counter `calls`: keys[0] for u, keys[1] for e0 | e1"""
    q, psi = eng.q[:ell], eng.psi_q[:ell]
    out = []
    for b in range(n):
        u = sm.ternary(keys[0], sm.stream_of(calls, b), eng.N)
        e0, b0 = sm.gaussian(keys[1], sm.stream_of(calls + 1, b), eng.N)
        e1, b1 = sm.gaussian(keys[1], sm.stream_of(calls + 1, n + b), eng.N)
        assert b0 == 0 and b1 == 0
        out.append(sm.enc_zero(orc, pk, u, e0, e1, q, psi))
    return out


def _with_message(zero, m, q):
    c = zero.copy()
    qq = np.asarray(q, dtype=np.uint64)[:, None]
    c[0] = (c[0] + np.asarray(m, dtype=np.uint64)) % qq          # residues below 2^60: the sum cannot wrap
    return c


def test_encrypt_single_equals_the_model(toy, orc):
    eng, pk, _ = toy
    ell = 4
    z = np.random.default_rng(1).uniform(-1, 1, 1 << eng.params.log_slots)
    pt = eng.encode(z, eng.n_q - ell)
    keys, calls = eng.debug_sampler_peek(3)
    ct = eng.encrypt(pt)
    assert ct.info()["ell"] == ell
    (zero,) = _fresh_zero(orc, eng, pk, keys, calls, 1, ell)
    assert np.array_equal(ct.export(), _with_message(zero, eng.pt_export(pt, ell), eng.q[:ell]))
    _after(eng, calls + 2, keys[2])


def test_encrypt_batch_of_33_draws_fresh_keys_for_its_second_chunk(toy, orc):
    eng, pk, _ = toy
    ell, n = 2, 33
    rows = np.random.default_rng(2).uniform(-1, 1, (n, 200))
    keys, calls = eng.debug_sampler_peek(5)
    cts = eng.encrypt_batch(rows, level=eng.n_q - ell)
    assert len(cts) == n
    zeros = _fresh_zero(orc, eng, pk, keys[0:2], calls, 32, ell) + _fresh_zero(orc, eng, pk, keys[2:4], calls + 2, 1, ell)
    for b in range(n):
        m = eng.pt_export(eng.encode(rows[b], eng.n_q - ell), ell)
        assert np.array_equal(cts[b].export(), _with_message(zeros[b], m, eng.q[:ell])), b
    _after(eng, calls + 4, keys[4])


def test_encrypt_single_at_bench_equals_the_model(bench, orc):
    eng, pk = bench
    ell = 2
    z = np.random.default_rng(3).uniform(-1, 1, 1 << eng.params.log_slots)
    pt = eng.encode(z, eng.n_q - ell)
    keys, calls = eng.debug_sampler_peek(3)
    ct = eng.encrypt(pt)
    (zero,) = _fresh_zero(orc, eng, pk, keys, calls, 1, ell)
    assert np.array_equal(ct.export(), _with_message(zero, eng.pt_export(pt, ell), eng.q[:ell]))
    _after(eng, calls + 2, keys[2])


# ----------------------------------------------------------------------------------------------------------------- sanitised replies
def _rerand_zero(orc, eng, pk, keys, calls, n, out_ell, bits):
    """(the n terms (pk_b u + NTT(e0 + f), pk_a u + NTT(e1)) of one chunk of a sanitize call at counter `calls`, the counter after it):
    keys[0] u, keys[1] e0 (and f), keys[2] e1"""
    q, psi = eng.q[:out_ell], eng.psi_q[:out_ell]
    c_e0 = calls + 1 if bits == 0 else calls + 2
    c_e1 = c_e0 + 1
    out = []
    for b in range(n):
        u = sm.ternary(keys[0], sm.stream_of(calls, b), eng.N)
        e0, b0 = sm.gaussian(keys[1], sm.stream_of(c_e0, b), eng.N)
        e1, b1 = sm.gaussian(keys[2], sm.stream_of(c_e1, b), eng.N)
        assert b0 == 0 and b1 == 0
        w = e0 + sm.flood(keys[1], sm.stream_of(calls + 1, b), bits, eng.N) if bits else e0
        out.append(sm.enc_zero(orc, pk, u, w, e1, q, psi))
    return out, c_e1 + 1


def _plus(pre, zero, q):
    """the first limbs of `pre` [2][>= out_ell][N] plus `zero` [2][out_ell][N]"""
    nl = zero.shape[1]
    qq = np.asarray(q[:nl], dtype=np.uint64)[:, None]
    return (np.ascontiguousarray(pre[:, :nl]) + zero) % qq


@pytest.mark.parametrize("bits", [0, 1, 24, 52])          # 1: the Gaussian decides the result - the int8 packing of gauss = 1 is visible
def test_sanitize_equals_input_plus_the_restated_encryption_of_zero(toy, orc, bits):
    eng, pk, _ = toy
    z = np.random.default_rng(4).uniform(-1, 1, 1 << eng.params.log_slots)
    ct = eng.encrypt(z, level=eng.n_q - 4)
    keys, calls = eng.debug_sampler_peek(4)
    out = eng.sanitize(ct, flood_bits=bits, out_ell=2)
    (zero,), after = _rerand_zero(orc, eng, pk, keys, calls, 1, 2, bits)
    assert after == calls + (4 if bits else 3)
    assert np.array_equal(out.export(), _plus(ct.export(), zero, eng.q))
    _after(eng, after, keys[3])


def test_sanitize_mixed_limb_counts_in_one_launch(toy, orc):
    eng, pk, _ = toy
    rng = np.random.default_rng(5)
    n = 1 << eng.params.log_slots
    cts = [eng.encrypt(rng.uniform(-1, 1, n), level=eng.n_q - ell) for ell in (4, 5, 3)]
    keys, calls = eng.debug_sampler_peek(4)
    outs = eng.sanitize(cts, flood_bits=24, out_ell=2)
    zeros, after = _rerand_zero(orc, eng, pk, keys, calls, 3, 2, 24)
    for b in range(3):
        assert np.array_equal(outs[b].export(), _plus(cts[b].export(), zeros[b], eng.q)), b
    _after(eng, after, keys[3])


def test_sanitize_batch_of_33_runs_a_second_chunk(toy, orc):
    eng, pk, _ = toy
    cts = eng.encrypt_batch(np.random.default_rng(6).uniform(-1, 1, (33, 64)), level=eng.n_q - 2)
    keys, calls = eng.debug_sampler_peek(7)
    outs = eng.sanitize(cts, flood_bits=24, out_ell=1)
    first, mid = _rerand_zero(orc, eng, pk, keys[0:3], calls, 32, 1, 24)
    second, after = _rerand_zero(orc, eng, pk, keys[3:6], mid, 1, 1, 24)
    assert (mid, after) == (calls + 4, calls + 8)
    for b, zero in enumerate(first + second):
        assert outs[b].info()["ell"] == 1
        assert np.array_equal(outs[b].export(), _plus(cts[b].export(), zero, eng.q)), b
    _after(eng, after, keys[6])


def test_sanitize_under_a_mask(toy, orc):
    """the pre-image is the engine's own mult_plain_batch + rescale_batch result, which other tests pin; they draw nothing"""
    eng, pk, _ = toy
    n = 1 << eng.params.log_slots
    ct = eng.encrypt(np.random.default_rng(7).uniform(0.5, 1, n), level=eng.n_q - 4)
    m = np.zeros(n)
    m[[0, 128, 256]] = 1.0
    mask = eng.encode(m)
    keys, calls = eng.debug_sampler_peek(4)
    (pre,) = eng.rescale_batch(eng.mult_plain_batch([ct], mask))
    _after(eng, calls, keys[0])
    assert pre.info()["ell"] == 3 and pre.info()["deg"] == 1
    out = eng.sanitize(ct, mask=mask, flood_bits=1, out_ell=2)
    (zero,), after = _rerand_zero(orc, eng, pk, keys, calls, 1, 2, 1)
    assert np.array_equal(out.export(), _plus(pre.export(), zero, eng.q))
    assert out.scale_parts() == pre.scale_parts()
    _after(eng, after, keys[3])


def test_sanitize_on_an_evaluation_context(fa, toy, orc):
    cl, pk, path = toy
    z = np.random.default_rng(8).uniform(-1, 1, 1 << cl.params.log_slots)
    sent = cl.encrypt(z, level=cl.n_q - 4)
    sv = fa.Engine.from_eval_keys(path, seed=123)
    try:
        at_server = _import_exact(sv, sent.export(), sent)
        keys, calls = sv.debug_sampler_peek(4)             # the server's own generator
        assert not np.array_equal(keys, cl.debug_sampler_peek(4)[0])
        reply = sv.sanitize(at_server, flood_bits=24, out_ell=2)
        (zero,), after = _rerand_zero(orc, sv, pk, keys, calls, 1, 2, 24)
        assert np.array_equal(reply.export(), _plus(sent.export(), zero, sv.q))
        _after(sv, after, keys[3])
    finally:
        sv.close()


# ---------------------------------------------------------------------------------------------------------------- flooded decryption
@pytest.mark.parametrize("ell", [4, 1])                   # two limbs read, and one
def test_decrypt_flooded_adds_the_restated_flood_polynomial(toy, orc, ell):
    eng, _, _ = toy
    bits = 30
    z = np.random.default_rng(9).uniform(-1, 1, 1 << eng.params.log_slots)
    ct = eng.encrypt(z, level=eng.n_q - ell)
    keys, calls = eng.debug_sampler_peek(2)
    got = eng.decrypt_flooded(ct, bits)
    f = sm.flood(keys[0], sm.stream_of(calls, 0), bits, eng.N)
    limbs = ct.export()
    q = eng.q[:ell]
    limbs[0] = (limbs[0] + sm.ntt_of(orc, f, q, eng.psi_q[:ell])) % np.asarray(q, dtype=np.uint64)[:, None]
    want = eng.decrypt(_import_exact(eng, limbs, ct))
    assert np.array_equal(got, want)                       # exact doubles
    assert not np.array_equal(got, eng.decrypt(ct))
    _after(eng, calls + 2, keys[1])                        # the Gaussian stream range is skipped, not used


# --------------------------------------------------------------------------------------------------------------------- seeded paths
def test_seeded_encryption_noise_is_the_restated_gaussian(fa):
    eng = fa.Engine("toy", seed=33)
    try:
        eng.keygen()
        eng.set_seeded_encryption(True)
        rng = np.random.default_rng(10)
        n = 1 << eng.params.log_slots
        # one vector at 4 limbs: the call's public seed is drawn first, then the sampler key
        pt = eng.encode(rng.uniform(-1, 1, n), eng.n_q - 4)
        keys, calls = eng.debug_sampler_peek(3)
        ct = eng.encrypt(pt)
        assert header(ct.export_compact())["seed"] == sm.key_bytes(keys[0])
        want, banded = sm.gaussian(keys[1], sm.stream_of(calls, 0), eng.N)
        assert banded == 0
        z = _noise(eng, pt, ct, 4)
        assert all(np.array_equal(z[l], want) for l in range(4))
        _after(eng, calls + 1, keys[2])
        # 33 rows at 2 limbs: one seed for the call, one sampler key per chunk of 32
        rows = rng.uniform(-1, 1, (33, 100))
        keys, calls = eng.debug_sampler_peek(4)
        cts = eng.encrypt_batch(rows, level=eng.n_q - 2)
        for b, ct in enumerate(cts):
            assert header(ct.export_compact())["seed"] == sm.key_bytes(keys[0])
            key, c, p = (keys[1], calls, b) if b < 32 else (keys[2], calls + 1, b - 32)
            want, banded = sm.gaussian(key, sm.stream_of(c, p), eng.N)
            assert banded == 0
            z = _noise(eng, eng.encode(rows[b], eng.n_q - 2), ct, 2)
            assert np.array_equal(z[0], want) and np.array_equal(z[1], want), b
        _after(eng, calls + 2, keys[3])
    finally:
        eng.close()


def _key_words(G4):
    """four generator words -> the eight key words of one key draw"""
    G4 = np.asarray(G4, dtype=np.uint64)
    return np.stack([G4 & np.uint64(0xFFFFFFFF), G4 >> np.uint64(32)], axis=1).astype(np.uint32).reshape(8)


def test_seeded_key_noise_is_the_restated_gaussian(fa, orc, tmp_path):
    """the seeded public key, the relinearisation key and one rotation key over all Q and P limbs (the noise is isolated as
    tests/test_seeded_keys_gpu.py::test_keys_are_valid_keys_of_the_secret does)"""
    cl = fa.Engine("toy", seed=77)
    try:
        cl.set_seeded_keys(True)
        assert cl.debug_sampler_peek(0)[1] == 0
        cl.keygen()
        N, m, nl, n_q, alpha = cl.N, [int(x) for x in cl.moduli], cl.n_limbs, cl.n_q, cl.alpha
        roots = [int(x) for x in cl.roots]
        s = cl.secret_export()
        # keygen: the secret's draws, then the key-set seed = four words of the generator, then one key draw for the public key's e
        G = chacha20_words(cl.secret_seed(), np.arange(512, dtype=np.uint64), 0).reshape(-1)
        ks = np.frombuffer(cl.key_set_seed(), dtype="<u8")
        at = [j for j in range(G.size - 12) if np.array_equal(G[j:j + 4], ks)]
        assert len(at) == 1 and at[0] >= 2 * cl.params.hamming       # one position and one sign word per secret coefficient at least
        j = at[0]
        _after(cl, 1, _key_words(G[j + 8:j + 12]))
        want, banded = sm.gaussian(_key_words(G[j + 4:j + 8]), sm.stream_of(0, 0), N)
        assert banded == 0
        pk = _public_key(cl, str(tmp_path / "seeded.evk"))
        e = _small(fa, orc.add(pk[0], orc.mul(pk[1], s[:n_q], m[:n_q]), m[:n_q]), m[:n_q], roots[:n_q])
        assert np.array_equal(e, want)
        # switching keys: one key draw per key, digit j's e at stream (C << 32) + j
        P = 1
        for p in m[n_q:]:
            P *= p
        gi = pow(5, -1, 2 * N)                                   # rotation by 1: Galois element 5
        for name in ("relin", "rotation"):
            keys, calls = cl.debug_sampler_peek(2)
            if name == "relin":
                cl.gen_relin_key()
                key, s_from, s_to = cl.key_export(0, 0), orc.mul(s, s, m), s
            else:
                cl.gen_rotation_keys([1])
                key, s_from, s_to = cl.key_export(1, 1), s, np.stack([orc.automorph_ntt(s[l], gi) for l in range(nl)])
            noise = key_noise(fa, key, s_from, s_to, m, roots, n_q, alpha, P)     # one integer polynomial per digit on all Q and P limbs
            assert len(noise) == cl.dnum_digits
            for d, e in enumerate(noise):
                want, banded = sm.gaussian(keys[0], sm.stream_of(calls, d), N)
                assert banded == 0
                assert np.array_equal(e, want), (name, d)
            _after(cl, calls + 1, keys[1])
    finally:
        cl.close()
