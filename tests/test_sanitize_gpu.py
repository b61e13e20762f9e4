"""Sanitised replies on the GPU (include/fhelin.h "Sanitised replies"): the wide sampler equals its definition restated with NumPy
ChaCha20 and Python integers on every residue; a re-randomised ciphertext differs from its input by ONE centred polynomial - a fresh
encryption of zero plus the flood term - of the predicted spread on the limbs that are kept; the slot values survive to the predicted
bound, alone, in a mixed batch, under a mask (which empties the other slots) and from degree 2; a server without the secret sanitises
what it was sent; the flooded decryption is the plain one at flood_bits = 0 and off by the predicted spread otherwise; every refusal
carries its status code and leaves the context usable.

Spreads.  v = e u + e0 + e1 s + f: e, e0, e1 rounded Gaussians of sigma 3.19, u uniform ternary (N coefficients of variance 2/3), s of
Hamming weight h, f uniform on [-2^B, 2^B) (variance 4^B / 3), so Var v = 4^B / 3 + 3.19^2 (2N/3 + h + 1).  A slot is a sum of the N
coefficients times unit roots over Delta: its real part has standard deviation sqrt(N/2) sigma_v / Delta = sqrt(n) sigma_v / Delta at
full packing (n = N/2)."""
import struct

import numpy as np
import pytest

from sampler_model import chacha20_words, flood_values  # noqa: F401  (the restatement lives with the sampler model)

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_NO_DEVICE, ERR_KEY = 1, 2, 5
SIGMA = 3.19


def sigma_v(eng, bits):
    return np.sqrt(4.0 ** bits / 3 + SIGMA ** 2 * (2 * eng.N / 3 + eng.params.hamming + 1))


def slot_sigma(eng, ct, bits):
    """predicted standard deviation of a slot of decrypt(sanitize(ct)) - decrypt(ct) at full packing"""
    hi, lo = ct.scale_parts()
    return np.sqrt(1 << eng.params.log_slots) * sigma_v(eng, bits) / (hi + lo)


def _code(fa, fn, *a, **kw):
    with pytest.raises(fa.FhelinError) as ei:
        fn(*a, **kw)
    return ei.value.code


@pytest.fixture(scope="module")
def clients(fa):
    """one keyed client per preset, shared by the tests of this module"""
    made = {}

    def get(preset):
        if preset not in made:
            e = fa.Engine(preset, seed=31)
            e.keygen()
            made[preset] = e
        return made[preset]
    yield get
    for e in made.values():
        e.close()


def test_flood_sampler_equals_its_definition_on_every_residue(clients):
    eng = clients("toy")
    q = [int(v) for v in eng.q]
    key = bytes((7 * i + 3) & 0xFF for i in range(32))
    for bits, stream in ((1, 0), (20, 5), (52, (9 << 32) | 2), (62, (1 << 64) - 1)):
        got = eng.debug_flood(key, stream, bits)
        assert got.shape == (eng.n_q, eng.N)
        f = flood_values(key, stream, bits, eng.N)
        assert min(f) >= -(1 << bits) and max(f) < (1 << bits)
        if bits == 62:
            assert max(abs(v) for v in f) > max(q[1:])          # |f| > q_l on the 52-bit limbs
        if bits == 1:
            assert set(f) == {-2, -1, 0, 1}                      # both signs and the boundary values
        for l in range(eng.n_q):
            want = np.array([v % q[l] for v in f], dtype=np.uint64)
            assert np.array_equal(got[l], want), (bits, l)
    # fewer limbs, another key: the first limbs' residues only
    assert np.array_equal(eng.debug_flood(bytes(32), 1, 20, ell=2)[1],
                          np.array([v % q[1] for v in flood_values(bytes(32), 1, 20, eng.N)], dtype=np.uint64))


def _phase_difference(eng, orc, ct, out, s):
    """phase(out) - phase(ct) on out's limbs after the oracle's inverse NTT: one centred polynomial, checked identical on every limb"""
    c, o = ct.export(), out.export()
    nl = o.shape[1]
    q, psi = eng.q[:nl], eng.psi_q[:nl]
    ph_o = orc.muladd(np.ascontiguousarray(o[0]), np.ascontiguousarray(o[1]), s[:nl], q)
    ph_c = orc.muladd(np.ascontiguousarray(c[0][:nl]), np.ascontiguousarray(c[1][:nl]), s[:nl], q)
    d = orc.ntt_batch(orc.sub(ph_o, ph_c, q), q, psi, inverse=True)
    v = d[0].astype(np.int64)
    v = np.where(v > int(q[0]) // 2, v - int(q[0]), v)
    for t in range(1, nl):
        vt = d[t].astype(np.int64)
        assert np.array_equal(np.where(vt > int(q[t]) // 2, vt - int(q[t]), vt), v), t
    return v.astype(np.float64), c, o


@pytest.mark.parametrize("preset", ["toy", "toy13"])
def test_rerandomisation_is_an_encryption_of_zero_plus_the_flood(clients, orc, preset):
    eng = clients(preset)
    n = 1 << eng.params.log_slots
    z = np.random.default_rng(8).uniform(-1, 1, n)
    ct = eng.encrypt(z, level=eng.n_q - 4)
    assert ct.info()["ell"] == 4
    s = eng.secret_export()
    for bits in (0, 24):                                        # 0: the negative control, the encryption-only figure
        out = eng.sanitize(ct, flood_bits=bits, out_ell=2)
        inf, src = out.info(), ct.info()
        assert (inf["npoly"], inf["ell"], inf["deg"], inf["slots"]) == (2, 2, 1, src["slots"])
        assert out.scale_parts() == ct.scale_parts()
        v, c, o = _phase_difference(eng, orc, ct, out, s)
        std = sigma_v(eng, bits)
        print(preset, bits, "std", v.std(), "predicted", std, "mean", v.mean(), "max", np.abs(v).max())
        assert abs(v.std() / std - 1) < 0.1, (v.std(), std)
        assert abs(v.mean()) < 0.1 * std
        assert np.abs(v).max() <= 2.0 ** bits + 6.5 * SIGMA * np.sqrt(2 * eng.N / 3 + eng.params.hamming + 1)
        if bits:
            assert np.abs(v).max() > 0.9 * 2.0 ** bits          # the flood is there: N uniform draws reach the edge
        assert np.mean(o[1] != c[1][:2]) >= 0.99                # c1 is a new polynomial
        again = eng.sanitize(ct, flood_bits=bits, out_ell=2).export()
        assert np.mean(again != o) >= 0.99                      # and another one on every call


def test_values_survive_single_and_mixed_batch(clients):
    eng = clients("toy")
    n = 1 << eng.params.log_slots
    rng = np.random.default_rng(9)
    zs = [rng.uniform(-1, 1, n) for _ in range(3)]
    cts = [eng.encrypt(z, level=eng.n_q - ell) for z, ell in zip(zs, (4, 5, 3))]
    base = [eng.decrypt(c) for c in cts]
    for bits in (24, 30):
        outs = [eng.sanitize(cts[0], flood_bits=bits)] + eng.sanitize(cts, flood_bits=bits, out_ell=2)
        for out, k in zip(outs, (0, 0, 1, 2)):
            assert out.info()["ell"] == 2
            d = eng.decrypt(out) - base[k]
            sd = slot_sigma(eng, cts[k], bits)
            print("bits", bits, "input", k, "std", d.std(), "predicted", sd, "max", np.abs(d).max())
            assert abs(d.std() / sd - 1) < 0.15, (d.std(), sd)
            assert np.abs(d).max() < 6 * sd
            assert np.abs(eng.decrypt(out) - zs[k]).max() < 6 * sd + 1e-9
    three = eng.sanitize(cts[1], flood_bits=24, out_ell=3)      # another limb count on request
    assert three.info()["ell"] == 3 and np.abs(eng.decrypt(three) - zs[1]).max() < 6 * slot_sigma(eng, cts[1], 24) + 1e-9


def test_mask_keeps_the_answer_and_empties_the_rest(clients):
    eng = clients("toy")
    n = 1 << eng.params.log_slots
    z = np.random.default_rng(10).uniform(0.5, 1, n)
    keep = [0, 128, 256]
    m = np.zeros(n)
    m[keep] = 1.0
    ct = eng.encrypt(z, level=eng.n_q - 4)
    base = eng.decrypt(ct)
    for mask in (m, eng.encode(m)):                             # slot values, or a plaintext handle
        out = eng.sanitize(ct, mask=mask, flood_bits=24, out_ell=2)
        assert out.info()["ell"] == 2 and out.info()["deg"] == 1
        bound = 6 * slot_sigma(eng, out, 24)
        got = eng.decrypt(out)
        print("mask: kept error", np.abs(got[keep] - base[keep]).max(), "others", np.abs(np.delete(got, keep)).max(), "bound", bound)
        assert bound < 1e-5
        assert np.abs(got[keep] - base[keep]).max() < bound
        assert np.abs(np.delete(got, keep)).max() < bound       # 0.5 .. 1 before
    assert eng.sanitize(ct, mask=m, flood_bits=24, out_ell=3).info()["ell"] == 3   # 4 limbs - the mask's rescale


def test_server_without_the_secret_sanitises(fa, clients, tmp_path):
    cl = clients("toy")
    path = str(tmp_path / "reply.evk")
    cl.save_eval_keys(path)
    n = 1 << cl.params.log_slots
    z = np.random.default_rng(11).uniform(-1, 1, n)
    sent = cl.encrypt(z, level=cl.n_q - 4)
    sv = fa.Engine.from_eval_keys(path, seed=123)
    try:
        inf = sent.info()
        at_server = sv.ct_import(sent.export(), deg=inf["deg"], scale=inf["scale"], slots=inf["slots"])
        reply = sv.sanitize(at_server, flood_bits=24, out_ell=2)
        assert _code(fa, sv.decrypt, reply) == ERR_KEY                # still no secret there
        assert _code(fa, sv.decrypt_flooded, reply, 20) == ERR_KEY
        rinf = reply.info()
        limbs = reply.export()
        assert limbs.shape == (2, 2, cl.N)
        back = cl.ct_import(limbs, deg=rinf["deg"], scale=rinf["scale"], slots=rinf["slots"])
        assert np.abs(cl.decrypt(back) - z).max() < 6 * slot_sigma(cl, sent, 24) + 1e-9
    finally:
        sv.close()


def test_degree_two_input_is_rescaled_first(clients):
    eng = clients("toy")
    n = 1 << eng.params.log_slots
    rng = np.random.default_rng(12)
    z, w = rng.uniform(-1, 1, n), rng.uniform(-1, 1, n)
    prod = eng.mult(eng.encrypt(z, level=eng.n_q - 4), eng.encode(w))
    assert prod.info()["deg"] == 2 and prod.info()["ell"] == 4
    out = eng.sanitize(prod, flood_bits=24, out_ell=2)
    inf = out.info()
    assert (inf["ell"], inf["deg"], inf["npoly"]) == (2, 1, 2)
    assert np.abs(eng.decrypt(out) - z * w).max() < 6 * slot_sigma(eng, out, 24) + 1e-9
    # with three limbs the rescale leaves exactly out_ell; with two it cannot
    assert eng.sanitize(eng.mult(eng.encrypt(z, level=eng.n_q - 3), eng.encode(w)), out_ell=2).info()["ell"] == 2


def test_decrypt_flooded(clients):
    eng = clients("toy")
    n = 1 << eng.params.log_slots
    z = np.random.default_rng(13).uniform(-1, 1, n)
    for ell in (4, 1):                                          # two limbs read, and one
        ct = eng.encrypt(z, level=eng.n_q - ell)
        plain = eng.decrypt(ct)
        assert np.array_equal(eng.decrypt_flooded(ct, 0), plain)
        hi, lo = ct.scale_parts()
        sd = np.sqrt(n) * np.sqrt(4.0 ** 30 / 3) / (hi + lo)
        a, b = eng.decrypt_flooded(ct, 30), eng.decrypt_flooded(ct, 30)
        print("decrypt_flooded ell", ell, "std", (a - plain).std(), "predicted", sd)
        assert abs((a - plain).std() / sd - 1) < 0.15 and np.abs(a - plain).max() < 6 * sd
        assert not np.array_equal(a, b)
        assert np.array_equal(eng.decrypt(ct), plain)           # the ciphertext is untouched


def _wrapped_blob(eng):
    """a version 2 compact blob (include/fhelin.h "Wrapped inputs") over the ring's first three moduli: c0 = 0, whose digest is 0"""
    ell, positions = 3, [0, 1, 2]
    H = 104 + 8 * ell + 8 * ((len(positions) + 1) // 2)
    b = bytearray(b"FHELINCC")
    b += struct.pack("<II", 2, H)
    b += struct.pack("<iiii", eng.log_n, ell, 1, 1 << eng.params.log_slots)
    b += struct.pack("<dd", 2.0 ** 52, 0.0)
    b += struct.pack("<Q", 5) + bytes(range(32)) + struct.pack("<Q", 0)
    b += struct.pack("<II", len(positions), len(positions))
    b += struct.pack(f"<{ell}Q", *[int(v) for v in eng.q[:ell]])
    b += struct.pack(f"<{len(positions)}I", *positions)
    b += bytes(H - len(b))
    b += bytes(8 * ell * eng.N)
    return bytes(b)


def test_refusals_carry_their_codes_and_leave_the_context_usable(fa, clients):
    eng = clients("toy")
    n = 1 << eng.params.log_slots
    z = np.random.default_rng(14).uniform(-1, 1, n)
    ct = eng.encrypt(z, level=eng.n_q - 4)
    two = eng.encrypt(z, level=eng.n_q - 2)
    m = np.ones(n)
    # flood_bits outside [0, 62]
    assert _code(fa, eng.sanitize, ct, flood_bits=-1) == ERR_ARG
    assert _code(fa, eng.sanitize, ct, flood_bits=63) == ERR_ARG
    assert _code(fa, eng.decrypt_flooded, ct, -1) == ERR_ARG
    assert _code(fa, eng.decrypt_flooded, ct, 63) == ERR_ARG
    assert _code(fa, eng.debug_flood, bytes(32), 0, 0) == ERR_ARG
    assert _code(fa, eng.debug_flood, bytes(32), 0, 63) == ERR_ARG
    # 2^(flood_bits + 2) not below the product of the limbs kept: q_0 has 55 bits
    assert _code(fa, eng.sanitize, ct, flood_bits=54, out_ell=1) == ERR_ARG
    assert eng.sanitize(ct, flood_bits=52, out_ell=1).info()["ell"] == 1
    assert _code(fa, eng.decrypt_flooded, eng.encrypt(z, level=eng.n_q - 1), 54) == ERR_ARG
    # too few limbs for the rescale, the mask and out_ell
    assert _code(fa, eng.sanitize, two, mask=m, out_ell=2) == ERR_ARG
    assert _code(fa, eng.sanitize, eng.mult(two, eng.encode(m)), out_ell=2) == ERR_ARG
    assert _code(fa, eng.sanitize, ct, out_ell=5) == ERR_ARG
    assert _code(fa, eng.sanitize, ct, out_ell=eng.n_q + 1) == ERR_ARG
    assert _code(fa, eng.sanitize, [ct, two], mask=m, out_ell=2) == ERR_ARG      # one short input refuses the batch
    # a 3-component input
    rng = np.random.default_rng(15)
    three = eng.ct_import(np.stack([[rng.integers(0, int(q), eng.N, dtype=np.uint64) for q in eng.q[:4]] for _ in range(3)]), deg=2)
    assert _code(fa, eng.sanitize, three) == ERR_ARG
    # a wrapped input
    wrapped = eng.import_compact([_wrapped_blob(eng)])[0]
    assert wrapped.wrapped_info()["count"] == 3
    assert _code(fa, eng.sanitize, wrapped) == ERR_ARG
    assert _code(fa, eng.sanitize, []) == ERR_ARG
    # no public key
    bare = fa.Engine("toy", seed=5)
    try:
        limbs = ct.export()
        assert _code(fa, bare.sanitize, bare.ct_import(limbs)) == ERR_KEY
    finally:
        bare.close()
    # the context is still usable
    out = eng.sanitize(ct, flood_bits=24)
    assert np.abs(eng.decrypt(out) - z).max() < 6 * slot_sigma(eng, ct, 24) + 1e-9
