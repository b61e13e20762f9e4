"""Seeded evaluation keys on the GPU (include/fhelin.h "Seeded evaluation keys"): every a half of a seeded-key client equals the
expansion restated here from fhelin_prng_block, the key-set seed and the documented nonces; every key is a valid key of the
secret; a compact set round-trips every key at half the bytes with the full set's digests; a server loaded from it evaluates
bit-identically to the client (toy13 operations, boot12 bootstraps, the reference-ring forward pass); corrupted compact sets are
refused atomically; and the mode's rules hold."""
import ctypes as C
import os
import struct

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_STATE, ERR_KEY = 1, 4, 5
SIGMA = 3.19


def read_table(data):
    compact = data[:8] == b"FHELINEC"
    n_keys = struct.unpack_from("<I", data, 12)[0]
    prm = struct.unpack_from("<9i", data, 16)
    base = (128 if compact else 96) + 8 * (prm[1] + prm[4])
    ents = []
    for k in range(n_keys):
        kind, digits, g, off, words, dg = struct.unpack_from("<IIQQQQ", data, base + 40 * k)
        ents.append(dict(kind=kind, digits=digits, galois=g, offset=off, words=words, digest=dg, at=base + 40 * k))
    return ents


def payload(data, ent):
    return np.frombuffer(data, dtype=np.uint64, count=ent["words"], offset=ent["offset"])


def move(ct, dst):
    """a ciphertext of one context as a handle of another: residues and the exact (80-bit) scale"""
    inf = ct.info()
    hi, lo = ct.scale_parts()
    buf = dst.upload(ct.export())
    try:
        out = dst.ct_import_device(buf.ptr.value, inf["npoly"], inf["ell"], inf["deg"], hi, lo, inf["slots"])
        dst.sync()
    finally:
        buf.free()
    return out


def _code(fa, fn, *a):
    with pytest.raises(fa.FhelinError) as ei:
        fn(*a)
    return ei.value.code, str(ei.value)


def _client(fa, preset, rotations=(1, -1, 5), boot=False, seed=77, seeded=True, **kw):
    e = fa.Engine(preset, seed=seed, **kw)
    if seeded:
        e.set_seeded_keys(True)
    e.keygen()
    e.gen_relin_key()
    if rotations:
        e.gen_rotation_keys(list(rotations))
    e.gen_conj_key()
    if boot:
        e.bootstrap_setup(3, 3, 0)
    return e


def nonce(kind, digit, galois):
    return (kind << 56) | (digit << 40) | galois


def expand(fa, seed, nc, limb, m, N):
    """limb `limb` of an a half, restated from fhelin_prng_block: residue 4b + k = (W[2k+1] 2^64 + W[2k]) mod m"""
    lib = fa.load_library()
    sb = (C.c_uint8 * 32)(*seed)
    blk = (C.c_uint8 * 64)()
    out = np.empty(N, dtype=np.uint64)
    for b in range(N // 4):
        assert lib.fhelin_prng_block(sb, (limb << 32) | b, nc, blk) == 0
        W = struct.unpack("<8Q", bytes(blk))
        for k in range(4):
            out[4 * b + k] = ((W[2 * k + 1] << 64) | W[2 * k]) % int(m)
    return out


def _keys(fa, e, rotations):
    """(kind, galois, engine export kind, index) of every switching key of a _client"""
    two_n = 2 * e.N
    out = [(1, 0, 0, 0), (3, two_n - 1, 2, 0)]
    out += [(2, pow(5, r, two_n), 1, r) for r in rotations]
    return out


def test_expansion_matches_the_specification(fa, tmp_path):
    rot = (1, -1, 5)
    cl = _client(fa, "toy", rotations=rot)
    path = str(tmp_path / "full.evk")
    try:
        seed = cl.key_set_seed()
        assert len(seed) == 32
        N, m, nl, n_q = cl.N, cl.moduli, cl.n_limbs, cl.n_q
        for kind, g, ek, idx in _keys(fa, cl, rot):
            key = cl.key_export(ek, idx)
            for j in range(cl.dnum_digits):
                for l in range(nl):     # Q and P limbs
                    want = expand(fa, seed, nonce(kind, j, g), l, m[l], N)
                    assert np.array_equal(key[j, 1, l], want), (kind, g, j, l)
        # the public key, from the full set's first payload [2][n_q][N]
        cl.save_eval_keys(path)
        data = open(path, "rb").read()
        ent = read_table(data)[0]
        assert ent["kind"] == 0
        pk = payload(data, ent).reshape(2, n_q, N)
        for l in range(n_q):
            assert np.array_equal(pk[1, l], expand(fa, seed, nonce(0, 0, 0), l, m[l], N)), l
    finally:
        cl.close()


def _small(fa, v, moduli, roots):
    """v [nl][N] NTT form -> the centred integer polynomial it represents, asserting it is the same on every limb"""
    import oracle as orc
    co = orc.ntt_batch(v, moduli, roots, inverse=True)
    cent = [np.where(co[l] > np.uint64(int(q) // 2), -(np.uint64(int(q)) - co[l]).astype(np.int64), co[l].astype(np.int64))
            for l, q in enumerate(moduli)]
    for l in range(1, len(moduli)):
        assert np.array_equal(cent[l], cent[0]), l
    return cent[0]


def key_noise(fa, key, s_from, s_to, m, roots, n_q, alpha, P):
    """per digit j of a switching key [digits][2][nl][N]: b_j + a_j s_to - (P mod q_t) s_from on the digit's limbs, as the centred integer
    polynomial it is on all Q and P limbs (tests/test_client_randomness_gpu.py compares it with the sampler model)"""
    import oracle as orc
    out = []
    for j in range(key.shape[0]):
        v = orc.add(key[j, 0], orc.mul(key[j, 1], s_to, m), m)
        for t in range(j * alpha, min((j + 1) * alpha, n_q)):
            pm = P % m[t]
            v[t] = (v[t].astype(object) - pm * s_from[t].astype(object)) % m[t]
        out.append(_small(fa, v.astype(np.uint64), m, roots))
    return out


def test_keys_are_valid_keys_of_the_secret(fa, tmp_path):
    import oracle as orc
    rot = (1, -1, 5)
    cl = _client(fa, "toy", rotations=rot)
    path = str(tmp_path / "full.evk")
    try:
        N, m, nl, n_q, alpha = cl.N, [int(x) for x in cl.moduli], cl.n_limbs, cl.n_q, cl.alpha
        roots = [int(x) for x in cl.roots]
        s = cl.secret_export()                       # [nl][N] NTT form
        P = 1
        for p in m[n_q:]:
            P *= p
        for kind, g, ek, idx in _keys(fa, cl, rot):
            key = cl.key_export(ek, idx)
            if kind == 1:
                s_from, s_to = orc.mul(s, s, m), s
            else:
                gi = pow(g, -1, 2 * N)
                s_from, s_to = s, np.stack([orc.automorph_ntt(s[l], gi) for l in range(nl)])
            for j, e in enumerate(key_noise(fa, key, s_from, s_to, m, roots, n_q, alpha, P)):
                assert np.abs(e).max() <= 10 * SIGMA, (kind, g, j)
                assert np.abs(e).max() > 0
        cl.save_eval_keys(path)
        data = open(path, "rb").read()
        pk = payload(data, read_table(data)[0]).reshape(2, n_q, N)
        v = orc.add(pk[0], orc.mul(pk[1], s[:n_q], m[:n_q]), m[:n_q])
        e = _small(fa, v, m[:n_q], roots[:n_q])
        assert 0 < np.abs(e).max() <= 10 * SIGMA
    finally:
        cl.close()


@pytest.mark.parametrize("preset,boot", [("toy", False), ("boot12", True)])
def test_compact_round_trip(fa, tmp_path, preset, boot):
    rot = (1, -1, 5) if not boot else (1,)
    cl = _client(fa, preset, rotations=rot, boot=boot)
    full, cmp_, again = str(tmp_path / "a.evk"), str(tmp_path / "a.evc"), str(tmp_path / "b.evc")
    try:
        cl.save_eval_keys(full)
        cl.save_eval_keys(cmp_, compact=True)
        fdata, cdata = open(full, "rb").read(), open(cmp_, "rb").read()
        fe, ce = read_table(fdata), read_table(cdata)
        # size: the documented layout, half of the full set's payload
        N, nm, n_q = cl.N, cl.n_limbs, cl.n_q
        n_sw = len(ce) - 1
        off = -(-(128 + 8 * nm + 40 * len(ce)) // 4096) * 4096
        assert len(cdata) == off + 8 * (n_q * N + n_sw * cl.dnum_digits * nm * N)
        assert abs((len(cdata) - off) / (len(fdata) - read_table(fdata)[0]["offset"]) - 0.5) < 1e-12
        print(f"{preset}: compact {len(cdata)} bytes, full {len(fdata)} bytes")
        assert [(x["kind"], x["galois"], x["digest"]) for x in ce] == [(x["kind"], x["galois"], x["digest"]) for x in fe]
        assert cdata[96:128] == cl.key_set_seed()
        params, bt, n = fa.Engine.eval_keys_params(cmp_)
        assert n == len(ce) and (bt is not None) == boot
        ev = fa.Engine.from_eval_keys(cmp_, seed=3)
        try:
            assert ev.key_set_seed() == cl.key_set_seed()
            for kind, g, ek, idx in _keys(fa, cl, rot):
                assert np.array_equal(cl.key_export(ek, idx), ev.key_export(ek, idx)), (kind, g)
            ev.save_eval_keys(again, compact=True)
            assert open(again, "rb").read() == cdata         # a re-save is the identical file
            ev.save_eval_keys(again)
            assert open(again, "rb").read() == fdata         # and its full set is the client's (public key included)
        finally:
            ev.close()
    finally:
        cl.close()


def test_toy13_evaluation_is_bit_identical_from_a_compact_set(fa, tmp_path):
    rot = (1, -1, 3, 5)
    cl = _client(fa, "toy13", rotations=rot)
    path = str(tmp_path / "t.evc")
    try:
        cl.save_eval_keys(path, compact=True)
        ev = fa.Engine.from_eval_keys(path, seed=9)
        try:
            rng = np.random.default_rng(1)
            n = 1 << cl.params.log_slots
            x, y = rng.uniform(-0.5, 0.5, n), rng.uniform(-0.5, 0.5, n)
            cx, cy = cl.encrypt(x), cl.encrypt(y)
            sx, sy = move(cx, ev), move(cy, ev)

            def run(e, a, b):
                r = e.rotate(a, 3)
                m = e.rescale(e.mult(r, b))
                return [r, m, e.rotate(m, -1), e.rotate(e.rotate(a, 1), 5)]

            want, got = run(cl, cx, cy), run(ev, sx, sy)
            for w, g in zip(want, got):
                assert np.array_equal(w.export(), g.export())
            back = move(got[1], cl)
            assert np.max(np.abs(cl.decrypt(back) - np.roll(x, -3) * y)) < 1e-6
            z = cl.decrypt(move(ev.encrypt(x), cl))      # the server's public-key encryption under the loaded public key
            assert np.max(np.abs(z - x)) < 1e-6
        finally:
            ev.close()
    finally:
        cl.close()


def test_boot12_bootstraps_are_bit_identical_from_a_compact_set(fa, tmp_path):
    """the bootstrap's key switches include the conjugation key (CoeffsToSlots)"""
    cl = _client(fa, "boot12", rotations=(), boot=True)
    path = str(tmp_path / "b.evc")
    try:
        cl.save_eval_keys(path, compact=True)
        ev = fa.Engine.from_eval_keys(path, seed=9)
        try:
            rng = np.random.default_rng(2)
            n = 1 << cl.params.log_slots
            x = rng.uniform(-0.5, 0.5, n)
            ct = cl.encrypt(x, level=cl.n_q - 3)
            want, got = cl.bootstrap(ct), ev.bootstrap(move(ct, ev))
            assert np.array_equal(want.export(), got.export())
            assert np.max(np.abs(cl.decrypt(move(got, cl)) - x)) < 1e-2
        finally:
            ev.close()
    finally:
        cl.close()


def test_reference_whole_pass_from_a_compact_set(fa, tmp_path):
    """forward_encrypted at the reference ring on a context loaded from the compact set, as
    test_evalkeys_gpu.py::test_reference_whole_pass_on_an_evaluation_context does from the full one"""
    from fhe_linformer_amd import linformer as lf
    from oracle import plain_forward as pf
    LOGIT_TOL = 1.2e-2
    S = 129
    w = pf.synthetic_model(1234)
    x_in, X_E, X_F = pf.client_inputs(w, pf.synthetic_tokens(S, 4321))
    cl = fa.Engine("reference", seed=11, n_q=28, n_p=-1)
    path = str(tmp_path / "ref.evc")
    try:
        cl.set_seeded_keys(True)
        cl.keygen()
        cl.gen_relin_key()
        cl.gen_rotation_keys(fa.circuit_rotation_indices())
        cl.bootstrap_setup(3, 3, 16384)
        cl.save_eval_keys(path, compact=True)
        print(f"compact evaluation-key set at the reference ring: {os.path.getsize(path) / 1e9:.2f} GB")
        ev = fa.Engine.from_eval_keys(path, seed=12)
        os.remove(path)
        try:
            cctl, sctl = lf.GpuController(cl), lf.GpuController(ev)
            for variant in ("main_2", "main"):
                enc = lf.encrypt_inputs(cctl, x_in, X_E, X_F)
                own = lf.forward_encrypted(cctl, w, enc, None, variant)
                senc = {k: [move(c, ev) for c in v] for k, v in enc.items()}
                srv = lf.forward_encrypted(sctl, w, senc, None, variant)
                back = move(srv, cl)
                if variant == "main_2":
                    assert np.array_equal(back.export(), own.export())
                lg, lo = lf.logits_from_slots(cl.decrypt(back)), lf.logits_from_slots(cl.decrypt(own))
                assert np.max(np.abs(lg - lo)) < LOGIT_TOL
                assert int(np.argmax(lg)) == int(np.argmax(lo))
        finally:
            ev.close()
    finally:
        cl.close()
        if os.path.exists(path):
            os.remove(path)


def _assert_holds_no_keys(fa, e):
    assert _code(fa, e.key_export, 0)[0] == ERR_KEY
    assert _code(fa, e.key_export, 2)[0] == ERR_KEY
    assert _code(fa, e.encrypt, np.zeros(4))[0] == ERR_KEY
    assert _code(fa, e.key_set_seed)[0] == ERR_STATE


def test_corrupted_compact_sets_are_refused_atomically(fa, tmp_path):
    cl = _client(fa, "toy", rotations=(1, 2, -1))
    path = str(tmp_path / "c.evc")
    try:
        cl.save_eval_keys(path, compact=True)
        good = open(path, "rb").read()
        ents = read_table(good)
        e = fa.Engine("toy", seed=2)
        try:
            # one flipped bit in a stored b residue
            bad = bytearray(good)
            last = ents[-1]
            bad[last["offset"] + 8 * (last["words"] // 2) + 3] ^= 0x10
            # one changed seed byte
            bad2 = bytearray(good)
            bad2[96 + 17] ^= 0x01
            # a changed (still valid and ordered) Galois element of the last rotation key
            rk = [x for x in ents if x["kind"] == 2]
            g = rk[-1]["galois"] + 2
            assert g < 2 * cl.N - 1
            bad3 = bytearray(good)
            struct.pack_into("<Q", bad3, rk[-1]["at"] + 8, g)
            for blob in (bad, bad2, bad3):
                open(path, "wb").write(blob)
                code, msg = _code(fa, e.load_eval_keys, path)
                assert code == ERR_ARG and ("digest" in msg or "residue" in msg), msg
                _assert_holds_no_keys(fa, e)
            # the same context is still fresh: the intact set loads
            open(path, "wb").write(good)
            e.load_eval_keys(path)
            assert np.array_equal(e.key_export(0), cl.key_export(0))
            assert e.key_set_seed() == cl.key_set_seed()
        finally:
            e.close()
    finally:
        cl.close()


def test_mode_rules(fa, tmp_path):
    p1, p2, p3 = (str(tmp_path / n) for n in ("1.evc", "2.evc", "v1.evk"))
    # after keygen: ERR_STATE; a default-mode context has no key-set seed and no compact form
    d = _client(fa, "toy", rotations=(1,), seeded=False)
    try:
        assert _code(fa, d.set_seeded_keys, True)[0] == ERR_STATE
        assert _code(fa, d.key_set_seed)[0] == ERR_STATE
        assert _code(fa, d.save_eval_keys, p1, True)[0] == ERR_STATE
        d.save_eval_keys(p3)
    finally:
        d.close()
    # on an evaluation context: ERR_KEY
    ev = fa.Engine.from_eval_keys(p3, seed=5)
    try:
        assert _code(fa, ev.set_seeded_keys, True)[0] == ERR_KEY
        assert _code(fa, ev.save_eval_keys, p1, True)[0] == ERR_STATE     # loaded from a full set: not seeded
    finally:
        ev.close()
    # a context that holds an imported key is not fresh
    k = fa.Engine("toy", seed=8)
    try:
        k.key_import(1, 3, np.zeros((k.dnum_digits, 2, k.n_limbs, k.N), dtype=np.uint64))
        assert _code(fa, k.set_seeded_keys, True)[0] == ERR_STATE
    finally:
        k.close()
    # two contexts from one secret seed: identical compact files; an imported key makes the set non-compact, naming it
    a, b = _client(fa, "toy", rotations=(1, 5), seed=31), _client(fa, "toy", rotations=(1, 5), seed=31)
    try:
        a.save_eval_keys(p1, compact=True)
        b.save_eval_keys(p2, compact=True)
        assert open(p1, "rb").read() == open(p2, "rb").read()
        # the full save of a seeded context loads, and evaluates with the same keys
        a.save_eval_keys(p3)
        ev = fa.Engine.from_eval_keys(p3, seed=6)
        try:
            assert np.array_equal(ev.key_export(1, 5), a.key_export(1, 5))
        finally:
            ev.close()
        b.key_import(1, 3, b.key_export(1, 1))
        code, msg = _code(fa, b.save_eval_keys, p2, True)
        assert code == ERR_STATE and "rotation key" in msg and str(pow(5, 3, 2 * b.N)) in msg, msg
    finally:
        a.close()
        b.close()
