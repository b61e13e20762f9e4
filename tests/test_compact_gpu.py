"""Seeded secret-key encryption and compact ciphertexts on the GPU (include/fhelin.h "Compact ciphertexts"): c1 of seeded
encryptions equals the expansion restated in test_compact_host.py's terms (restated again here), the fresh noise is one rounded
Gaussian, compact export / import round-trips every residue and the exact scale, an evaluation context computes bit-identically on
imported values (rotate, mult + relin, rescale, bootstrap, the reference-ring forward pass), seeds are fresh per call, malformed
or foreign blobs are refused atomically, and a level plan recorded in public-key mode applies in seeded mode."""
import os
import struct

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

P61 = (1 << 61) - 1
ERR_ARG, ERR_STATE, ERR_KEY = 1, 4, 5


def chacha20_words(seed, counter, stream):
    """ChaCha20 blocks (RFC 8439) for 64-bit counters (array), one 64-bit stream -> uint64 [len(counter)][8], little-endian"""
    ctr = np.atleast_1d(np.asarray(counter, dtype=np.uint64))
    key = np.frombuffer(bytes(seed), dtype="<u4")
    init = np.empty((16, ctr.size), dtype=np.uint32)
    init[0:4] = np.array([0x61707865, 0x3320646E, 0x79622D32, 0x6B206574], dtype=np.uint32)[:, None]
    init[4:12] = key[:, None]
    init[12] = (ctr & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    init[13] = (ctr >> np.uint64(32)).astype(np.uint32)
    init[14] = np.uint32(stream & 0xFFFFFFFF)
    init[15] = np.uint32(stream >> 32)
    x = init.copy()

    def rotl(v, k):
        return (v << np.uint32(k)) | (v >> np.uint32(32 - k))

    def qr(a, b, c, d):
        x[a] += x[b]; x[d] ^= x[a]; x[d] = rotl(x[d], 16)
        x[c] += x[d]; x[b] ^= x[c]; x[b] = rotl(x[b], 12)
        x[a] += x[b]; x[d] ^= x[a]; x[d] = rotl(x[d], 8)
        x[c] += x[d]; x[b] ^= x[c]; x[b] = rotl(x[b], 7)

    with np.errstate(over="ignore"):
        for _ in range(10):
            qr(0, 4, 8, 12); qr(1, 5, 9, 13); qr(2, 6, 10, 14); qr(3, 7, 11, 15)
            qr(0, 5, 10, 15); qr(1, 6, 11, 12); qr(2, 7, 8, 13); qr(3, 4, 9, 14)
        x += init
    w = x.astype(np.uint64)
    return (w[0::2] | (w[1::2] << np.uint64(32))).T


def expand_c1(seed, nonce, limb, q, N):
    b = np.arange(N // 4, dtype=np.uint64)
    W = chacha20_words(seed, (np.uint64(limb) << np.uint64(32)) | b, nonce)
    lo, hi = W[:, 0::2].reshape(-1), W[:, 1::2].reshape(-1)
    return ((hi.astype(object) * (1 << 64) + lo.astype(object)) % int(q)).astype(np.uint64)


def mix32(x):
    x = np.asarray(x, dtype=np.uint64) & 0xFFFFFFFF
    x ^= x >> 16
    x = (x * 0x7FEB352D) & 0xFFFFFFFF
    x ^= x >> 15
    x = (x * 0x846CA68B) & 0xFFFFFFFF
    x ^= x >> 16
    return x


def c0_digest(c0):
    """the evaluation-key digest over c0's limb vectors (include/fhelin.h)"""
    c0 = np.asarray(c0, dtype=np.uint64)
    k = mix32(np.arange(c0.shape[1], dtype=np.uint64) ^ 0x9E3779B9).astype(object)
    w = mix32(np.arange(c0.shape[0], dtype=np.uint64) | 0x80000000)
    d = [int(((v % np.uint64(P61)).astype(object) * k).sum() % P61) for v in c0]
    return sum(dj * int(wj) for dj, wj in zip(d, w)) % P61


def header(blob):
    log_n, ell, deg, slots = struct.unpack_from("<4i", blob, 16)
    hi, lo, nonce = struct.unpack_from("<2dQ", blob, 32)
    return dict(log_n=log_n, ell=ell, deg=deg, slots=slots, scale=(hi, lo), nonce=nonce, seed=bytes(blob[56:88]),
                digest=struct.unpack_from("<Q", blob, 88)[0])


def c0_of(blob, N):
    ell = header(blob)["ell"]
    return np.frombuffer(blob, dtype="<u8", count=ell * N, offset=96 + 8 * ell).reshape(ell, N)


def with_c0(blob, c0, digest=None):
    """the blob with c0 replaced (and the digest field, when given)"""
    ell = header(blob)["ell"]
    b = bytearray(blob)
    b[96 + 8 * ell:] = np.ascontiguousarray(c0, dtype="<u8").tobytes()
    if digest is not None:
        struct.pack_into("<Q", b, 88, digest)
    return bytes(b)


def _code(fa, fn, *a):
    with pytest.raises(fa.FhelinError) as ei:
        fn(*a)
    return ei.value.code


def _client(fa, preset, rotations=True, boot=False, seed=77):
    e = fa.Engine(preset, seed=seed)
    e.keygen()
    e.gen_relin_key()
    if rotations:
        e.gen_rotation_keys([1, -1, 3, 5])
    if boot:
        e.bootstrap_setup(3, 3, 0)
    return e


def _check_c1(eng, ct, limbs):
    blob = ct.export_compact()
    h = header(blob)
    full = ct.export()
    assert h["ell"] == full.shape[1]
    assert np.array_equal(c0_of(blob, eng.N), full[0])
    for l in limbs:
        assert np.array_equal(full[1][l], expand_c1(h["seed"], h["nonce"], l, eng.q[l], eng.N)), l
    return h


def test_c1_is_the_expansion(fa):
    e = _client(fa, "toy", rotations=False)
    try:
        e.set_seeded_encryption(True)
        rng = np.random.default_rng(1)
        n = 1 << e.params.log_slots
        for lvl in (0, 2):
            for ct in e.encrypt_batch(rng.uniform(-1, 1, (3, n)), level=lvl):
                _check_c1(e, ct, range(e.n_q - lvl))
        h = _check_c1(e, e.encrypt(rng.uniform(-1, 1, n)), range(e.n_q))
        # the import path's kernel alone: a batch of nonces, a lower level = a prefix of the same limbs
        got, _ = e.debug_seeded_expand(h["seed"], h["nonce"], e.n_q - 2, n_ct=3)
        for i in range(3):
            for l in range(e.n_q - 2):
                assert np.array_equal(got[i][l], expand_c1(h["seed"], h["nonce"] + i, l, e.q[l], e.N)), (i, l)
    finally:
        e.close()
    b = _client(fa, "bench", rotations=False)
    try:
        b.set_seeded_encryption(True)
        ct = b.encrypt(np.random.default_rng(2).uniform(-1, 1, 1 << b.params.log_slots))
        top = b.n_q - 1
        _check_c1(b, ct, [0, top // 2, top])
    finally:
        b.close()


def _noise(eng, pt, ct, ell):
    """raw_phase - the encoding, back in coefficient form, centred per limb: [ell][N] int64"""
    ph = eng.raw_phase(ct).export()[0]
    m = eng.pt_export(pt, ell)
    q = eng.q[:ell].astype(np.uint64)[:, None]
    d = (ph + (q - m)) % q
    buf = eng.upload(d)
    try:
        eng.ntt(buf, ell, 0, ell, inverse=True)
        co = buf.download(d.shape)
    finally:
        buf.free()
    return np.where(co > q // np.uint64(2), co.astype(np.int64) - q.astype(np.int64), co.astype(np.int64))


def test_fresh_noise_is_one_gaussian(fa):
    e = _client(fa, "bench", rotations=False)
    try:
        x = np.random.default_rng(3).uniform(-1, 1, 1 << e.params.log_slots)
        pt = e.encode(x, 0)
        e.set_seeded_encryption(True)
        z = _noise(e, pt, e.encrypt(pt), e.n_q)
        assert all(np.array_equal(z[0], z[l]) for l in range(1, z.shape[0])), "the noise is not one integer polynomial (CRT)"
        var, mx = float(np.var(z[0].astype(np.float64))), int(np.max(np.abs(z[0])))
        print(f"seeded: noise variance {var:.3f} (3.19^2 = {3.19 ** 2:.3f}), max {mx}")
        assert abs(var - 3.19 ** 2) < 0.05 * 3.19 ** 2 and mx <= 41
        e.set_seeded_encryption(False)
        zp = _noise(e, pt, e.encrypt(pt), e.n_q)
        vp = float(np.var(zp[0].astype(np.float64)))
        print(f"public-key: noise variance {vp:.1f}")
        assert vp > 1000 * var
    finally:
        e.close()


def test_compact_round_trip_single_and_194_of_mixed_levels(fa):
    e = _client(fa, "toy13", rotations=False)
    try:
        e.set_seeded_encryption(True)
        rng = np.random.default_rng(4)
        n = 1 << e.params.log_slots
        ct = e.encrypt(rng.uniform(-1, 1, n))
        blob = ct.export_compact()
        ell = ct.info()["ell"]
        assert len(blob) == 96 + 8 * ell + 8 * ell * e.N == ct.compact_bytes()
        (back,) = e.import_compact([blob])
        assert np.array_equal(back.export(), ct.export())
        assert back.scale_parts() == ct.scale_parts()
        assert {k: back.info()[k] for k in ("ell", "deg", "slots")} == {k: ct.info()[k] for k in ("ell", "deg", "slots")}
        # 194 ciphertexts of mixed levels, shuffled, in ONE call
        cts = []
        for lvl, cnt in ((0, 80), (1, 60), (3, 40), (5, 14)):
            cts += e.encrypt_batch(rng.uniform(-1, 1, (cnt, n)), level=lvl)
        order = rng.permutation(len(cts))
        cts = [cts[i] for i in order]
        blobs = [c.export_compact() for c in cts]
        for c, b in zip(cts, blobs):
            el = c.info()["ell"]
            assert len(b) == 96 + 8 * el + 8 * el * e.N
        backs = e.import_compact(blobs)
        assert len(backs) == 194
        for c, b in zip(cts, backs):
            assert np.array_equal(b.export(), c.export())
            assert b.scale_parts() == c.scale_parts()
            assert {k: b.info()[k] for k in ("ell", "deg", "slots")} == {k: c.info()[k] for k in ("ell", "deg", "slots")}
        print(f"194 inputs: {sum(map(len, blobs)) / 1e6:.1f} MB compact, "
              f"{sum(c.export().nbytes for c in cts) / 1e6:.1f} MB full")
    finally:
        e.close()


def test_toy13_server_is_bit_identical_on_imported_values(fa, tmp_path):
    cl = _client(fa, "toy13")
    path = str(tmp_path / "t.evk")
    try:
        cl.save_eval_keys(path)
        ev = fa.Engine.from_eval_keys(path, seed=9)
        try:
            cl.set_seeded_encryption(True)
            rng = np.random.default_rng(5)
            n = 1 << cl.params.log_slots
            x, y = rng.uniform(-0.5, 0.5, n), rng.uniform(-0.5, 0.5, n)
            cx, cy = cl.encrypt_batch(np.stack([x, y]))
            sx, sy = ev.import_compact([cx.export_compact(), cy.export_compact()])

            def run(e, a, b):
                r = e.rotate(a, 3)
                m = e.mult(r, b)
                return [r, m, e.rescale(m)]

            for w, g in zip(run(cl, cx, cy), run(ev, sx, sy)):
                assert np.array_equal(w.export(), g.export())
            assert np.max(np.abs(cl.decrypt(cx) - x)) < 1e-6
        finally:
            ev.close()
    finally:
        cl.close()
        os.remove(path)


def test_boot12_server_bootstraps_imported_values_bit_identically(fa, tmp_path):
    cl = _client(fa, "boot12", rotations=False, boot=True)
    path = str(tmp_path / "b.evk")
    try:
        cl.save_eval_keys(path)
        ev = fa.Engine.from_eval_keys(path, seed=9)
        try:
            cl.set_seeded_encryption(True)
            rng = np.random.default_rng(6)
            x = rng.uniform(-0.5, 0.5, 1 << cl.params.log_slots)
            ct = cl.encrypt(x, level=cl.n_q - 3)
            (sct,) = ev.import_compact([ct.export_compact()])
            want, got = cl.bootstrap(ct), ev.bootstrap(sct)
            assert np.array_equal(want.export(), got.export())
            assert np.max(np.abs(cl.decrypt(want) - x)) < 1e-2
        finally:
            ev.close()
    finally:
        cl.close()
        os.remove(path)


def test_reference_whole_pass_on_compact_inputs(fa, tmp_path):
    """forward_encrypted (main_2) at the reference ring on a context loaded from the set, its 194 inputs moved as compact blobs:
    bit for bit the client's own pass, logits within the tolerance of tests/test_forward_gpu.py with the same argmax"""
    from fhe_linformer_amd import linformer as lf
    from oracle import plain_forward as pf
    LOGIT_TOL = 1.2e-2
    S = 129
    w = pf.synthetic_model(1234)
    x_in, X_E, X_F = pf.client_inputs(w, pf.synthetic_tokens(S, 4321))
    cl = fa.Engine("reference", seed=11, n_q=28, n_p=-1)
    path = str(tmp_path / "ref.evk")
    try:
        cl.keygen()
        cl.gen_relin_key()
        cl.gen_rotation_keys(fa.circuit_rotation_indices())
        cl.bootstrap_setup(3, 3, 16384)
        cl.save_eval_keys(path)
        ev = fa.Engine.from_eval_keys(path, seed=12)
        os.remove(path)
        try:
            cctl, sctl = lf.GpuController(cl), lf.GpuController(ev)
            cl.set_seeded_encryption(True)
            enc = lf.encrypt_inputs(cctl, x_in, X_E, X_F)
            keys = ("inputs_E", "inputs_F", "inputs")
            flat = [c for k in keys for c in enc[k]]
            blobs = [c.export_compact() for c in flat]
            compact = sum(map(len, blobs))
            full = sum(2 * c.info()["ell"] * cl.N * 8 for c in flat)
            print(f"reference ring, {len(flat)} inputs: {compact / 1e9:.3f} GB compact vs {full / 1e9:.3f} GB full ({compact / full:.3f})")
            imp = ev.import_compact(blobs)
            senc, at = {}, 0
            for k in keys:
                senc[k] = imp[at:at + len(enc[k])]
                at += len(enc[k])
            own = lf.forward_encrypted(cctl, w, enc, None, "main_2")
            srv = lf.forward_encrypted(sctl, w, senc, None, "main_2")
            inf = srv.info()
            hi, lo = srv.scale_parts()
            buf = cl.upload(srv.export())
            try:
                back = cl.ct_import_device(buf.ptr.value, inf["npoly"], inf["ell"], inf["deg"], hi, lo, inf["slots"])
                cl.sync()
            finally:
                buf.free()
            assert np.array_equal(back.export(), own.export())
            lg, lo_ = lf.logits_from_slots(cl.decrypt(back)), lf.logits_from_slots(cl.decrypt(own))
            assert np.max(np.abs(lg - lo_)) < LOGIT_TOL
            assert int(np.argmax(lg)) == int(np.argmax(lo_))
        finally:
            ev.close()
    finally:
        cl.close()
        if os.path.exists(path):
            os.remove(path)


def test_seeds_are_fresh_per_call_and_nonces_count_outputs(fa):
    e = _client(fa, "toy", rotations=False)
    try:
        e.set_seeded_encryption(True)
        n = 1 << e.params.log_slots
        rows = np.zeros((5, n))
        a, b = e.encrypt_batch(rows), e.encrypt_batch(rows)
        ha, hb = [header(c.export_compact()) for c in a], [header(c.export_compact()) for c in b]
        assert [h["nonce"] for h in ha] == list(range(5)) == [h["nonce"] for h in hb]
        assert len({h["seed"] for h in ha}) == 1 and len({h["seed"] for h in hb}) == 1 and ha[0]["seed"] != hb[0]["seed"]
        c1 = [c.export()[1] for c in a + b]
        for i in range(len(c1)):
            for j in range(i + 1, len(c1)):
                assert not np.array_equal(c1[i], c1[j]), (i, j)
        # the ingest path and single encryptions draw their own seeds too
        s1, s2 = header(e.encrypt(rows[0]).export_compact()), header(e.encrypt(rows[0]).export_compact())
        assert s1["nonce"] == s2["nonce"] == 0 and s1["seed"] != s2["seed"] and s1["seed"] not in (ha[0]["seed"], hb[0]["seed"])
    finally:
        e.close()


def test_refusals(fa, tmp_path):
    cl = _client(fa, "toy13")
    path = str(tmp_path / "r.evk")
    try:
        cl.save_eval_keys(path)
        ev = fa.Engine.from_eval_keys(path, seed=9)
        other = _client(fa, "toy", rotations=False)
        try:
            assert _code(fa, ev.set_seeded_encryption, True) == ERR_KEY
            n = 1 << cl.params.log_slots
            x = np.random.default_rng(7).uniform(-0.5, 0.5, n)
            pk_ct = cl.encrypt(x)
            assert _code(fa, pk_ct.export_compact) == ERR_STATE
            cl.set_seeded_encryption(True)
            ct, ct2 = cl.encrypt_batch(np.stack([x, x]))
            for res in (cl.rotate(ct, 1), cl.add(ct, ct2), cl.mult(ct, ct2), cl.rescale(cl.mult(ct, ct2)), cl.negate(ct)):
                assert _code(fa, res.export_compact) == ERR_STATE
            blob, blob2 = ct.export_compact(), ct2.export_compact()
            (imp,) = ev.import_compact([blob])
            assert _code(fa, imp.export_compact) == ERR_STATE          # an imported value is not a seeded encryption of this context
            # another ring dimension
            other.set_seeded_encryption(True)
            oblob = other.encrypt(np.zeros(1 << other.params.log_slots)).export_compact()
            assert _code(fa, ev.import_compact, [oblob]) == ERR_ARG
            # other moduli
            b = bytearray(blob)
            struct.pack_into("<Q", b, 96, struct.unpack_from("<Q", b, 96)[0] - 2)
            assert _code(fa, ev.import_compact, [bytes(b)]) == ERR_ARG
            # a flipped c0 word: digest mismatch
            c0 = c0_of(blob, cl.N).copy()
            c0[1, 17] ^= np.uint64(1)
            assert _code(fa, ev.import_compact, [with_c0(blob, c0)]) == ERR_ARG
            # a residue >= q with a digest that matches it: the range check
            c0 = c0_of(blob, cl.N).copy()
            c0[2, 5] = cl.q[2]
            assert c0_digest(c0_of(blob, cl.N)) == header(blob)["digest"]
            assert _code(fa, ev.import_compact, [with_c0(blob, c0, c0_digest(c0))]) == ERR_ARG
            # a malformed header
            assert _code(fa, ev.import_compact, [blob[:-8]]) == ERR_ARG
            # one bad blob in a batch: no handle at all
            assert _code(fa, ev.import_compact, [blob, blob2, with_c0(blob2, c0_of(blob, cl.N))]) == ERR_ARG
            good = ev.import_compact([blob, blob2])
            assert np.array_equal(good[1].export(), ct2.export())
        finally:
            other.close()
            ev.close()
    finally:
        cl.close()
        os.remove(path)


def test_level_plan_recorded_in_public_key_mode_applies_in_seeded_mode(fa):
    """the ingest outputs are level-plan sources in the same order and count in both modes: a plan recorded with public-key
    encryption starts every output of a seeded ingest at the level it gives a public-key one"""
    e = _client(fa, "bench", rotations=False)
    try:
        rng = np.random.default_rng(8)
        S = 3
        inp = dict(cls=rng.uniform(-1, 1, 128), pos=rng.uniform(-1, 1, (S, 128)), E_w=rng.uniform(-0.1, 0.1, (32, S + 1)),
                   E_b=rng.uniform(-0.1, 0.1, 32), F_w=rng.uniform(-0.1, 0.1, (32, S + 1)), F_b=rng.uniform(-0.1, 0.1, 32),
                   emb=rng.uniform(-1, 1, (S, 128)))

        def program():
            r = e.client_ingest(**inp)
            outs = r["inputs_E"] + r["inputs_F"] + r["inputs"]
            d = e.rescale(e.mult(outs[0], outs[64]))
            e.decrypt(e.rescale(e.mult(d, outs[1])))
            e.decrypt(outs[65])
            return outs

        e.level_plan_begin("record")
        program()
        plan = e.level_plan_end()
        e.level_plan_begin("apply")
        want = [c.info()["ell"] for c in program()]
        e.level_plan_end()
        e.set_seeded_encryption(True)
        e.level_plan_begin("apply")
        outs = program()
        e.level_plan_end()
        assert [c.info()["ell"] for c in outs] == want, (plan, want)
        assert min(want) < e.n_q and len(set(want)) > 1
        for c in (outs[0], outs[64], outs[65]):
            assert header(c.export_compact())["ell"] == c.info()["ell"]
    finally:
        e.close()
