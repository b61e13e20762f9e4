"""Evaluation-key sets on the GPU: a client context saves its public key material, a context that never held the secret loads it
and evaluates bit-identically to the client; the set carries no secret; corrupted sets are refused without installing anything;
the device digest kernel equals the restatement in test_evalkeys_host.py's terms (restated again here)."""
import os
import struct

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

P61 = (1 << 61) - 1
ERR_ARG, ERR_STATE, ERR_KEY = 1, 4, 5


def mix32(x):
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


def read_table(data):
    n_keys = struct.unpack_from("<I", data, 12)[0]
    n_q, n_p = struct.unpack_from("<9i", data, 16)[1], struct.unpack_from("<9i", data, 16)[4]
    base = 96 + 8 * (n_q + n_p)
    ents = []
    for k in range(n_keys):
        kind, digits, g, off, words, dg = struct.unpack_from("<IIQQQQ", data, base + 40 * k)
        ents.append(dict(kind=kind, digits=digits, galois=g, offset=off, words=words, digest=dg, at=base + 40 * k))
    return ents


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


def _client(fa, preset, rotations=True, boot=False, seed=77):
    e = fa.Engine(preset, seed=seed)
    e.keygen()
    e.gen_relin_key()
    if rotations:
        e.gen_rotation_keys(fa.circuit_rotation_indices())
    e.gen_conj_key()
    if boot:
        e.bootstrap_setup(3, 3, 0)
    return e


@pytest.mark.parametrize("preset,boot", [("toy", False), ("toy13", False), ("boot12", True)])
def test_keys_round_trip(fa, tmp_path, preset, boot):
    cl = _client(fa, preset, rotations=not boot, boot=boot)
    path, path2 = str(tmp_path / "a.evk"), str(tmp_path / "b.evk")
    try:
        cl.save_eval_keys(path)
        ev = fa.Engine.from_eval_keys(path, seed=3)
        try:
            idx = [1, -1, 5] if not boot else [1]
            for kind, i in [(0, 0), (2, 0)] + [(1, r) for r in idx]:
                assert np.array_equal(cl.key_export(kind, i), ev.key_export(kind, i)), (kind, i)
            # every key, byte for byte: the evaluation context writes the identical set
            ev.save_eval_keys(path2)
            with open(path, "rb") as f1, open(path2, "rb") as f2:
                assert f1.read() == f2.read()
        finally:
            ev.close()
    finally:
        cl.close()
        for p in (path, path2):
            if os.path.exists(p):
                os.remove(p)


def test_toy13_evaluation_is_bit_identical_without_the_secret(fa, tmp_path):
    cl = _client(fa, "toy13")
    path = str(tmp_path / "t.evk")
    try:
        cl.save_eval_keys(path)
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
                return [r, m, e.eval_chebyshev(m, [0.3, 0.5, -0.2, 0.1, 0.05], -1.0, 1.0)]

            want, got = run(cl, cx, cy), run(ev, sx, sy)
            for w, g in zip(want, got):
                assert np.array_equal(w.export(), g.export())
            back = move(got[1], cl)
            assert np.max(np.abs(cl.decrypt(back) - np.roll(x, -3) * y)) < 1e-6
            # public-key encryption on the evaluation context: the client decrypts it
            z = cl.decrypt(move(ev.encrypt(x), cl))
            assert np.max(np.abs(z - x)) < 1e-6
        finally:
            ev.close()
    finally:
        cl.close()
        os.remove(path)


def test_boot12_bootstraps_are_bit_identical_without_the_secret(fa, tmp_path):
    cl = _client(fa, "boot12", rotations=False, boot=True)
    path = str(tmp_path / "b.evk")
    try:
        cl.save_eval_keys(path)
        ev = fa.Engine.from_eval_keys(path, seed=9)
        try:
            rng = np.random.default_rng(2)
            n = 1 << cl.params.log_slots
            xs = [rng.uniform(-0.5, 0.5, n) for _ in range(2)]
            cts = [cl.encrypt(x, level=cl.n_q - 3) for x in xs]
            scs = [move(c, ev) for c in cts]

            def run(e, v):
                return [e.bootstrap(v[0]), e.bootstrap_iter(v[1], 8)] + e.bootstrap_batch(v)

            want, got = run(cl, cts), run(ev, scs)
            for w, g in zip(want, got):
                assert np.array_equal(w.export(), g.export())
            for g, x in zip(got, [xs[0], xs[1], xs[0], xs[1]]):
                assert np.max(np.abs(cl.decrypt(move(g, cl)) - x)) < 1e-2
        finally:
            ev.close()
    finally:
        cl.close()
        os.remove(path)


def test_no_secret_on_the_server(fa, tmp_path):
    cl = _client(fa, "toy")
    path = str(tmp_path / "s.evk")
    try:
        cl.save_eval_keys(path)
        seed, s = cl.secret_seed(), cl.secret_export()
        data = open(path, "rb").read()
        assert data.find(seed) < 0
        # no 8 consecutive words of any limb of s, at any byte alignment
        first = {}
        for li, limb in enumerate(s):
            for pos in range(0, limb.size - 7):
                first.setdefault(int(limb[pos]), []).append((li, pos))
        keys = np.fromiter(first.keys(), dtype=np.uint64)
        for a in range(8):
            m = (len(data) - a) // 8
            arr = np.frombuffer(data, dtype=np.uint64, count=m, offset=a)
            for i in np.nonzero(np.isin(arr, keys))[0]:
                for li, pos in first[int(arr[i])]:
                    assert not np.array_equal(arr[i:i + 8], s[li, pos:pos + 8])
        ev = fa.Engine.from_eval_keys(path, seed=4)
        try:
            ct = ev.encrypt(np.zeros(16))
            assert _code(fa, ev.decrypt, ct)[0] == ERR_KEY
            assert _code(fa, ev.secret_export)[0] == ERR_KEY
            assert _code(fa, ev.secret_seed)[0] == ERR_KEY
            assert _code(fa, ev.keygen)[0] == ERR_KEY
            ev.gen_rotation_keys([1, -4, 3])      # present: confirmed
            ev.gen_conj_key()
            ev.gen_relin_key()
            code, msg = _code(fa, ev.gen_rotation_keys, [1, 11])
            assert code == ERR_KEY and "11" in msg
            # a second load into an evaluation context
            assert _code(fa, ev.load_eval_keys, path)[0] == ERR_STATE
        finally:
            ev.close()
    finally:
        cl.close()
        os.remove(path)
    # a context that ran keygen is not fresh
    c2 = fa.Engine("toy", seed=5)
    c3 = _client(fa, "toy", rotations=False)
    try:
        c3.save_eval_keys(path)
        c2.keygen()
        assert _code(fa, c2.load_eval_keys, path)[0] == ERR_STATE
        c4 = fa.Engine("toy13", seed=6)
        try:
            assert _code(fa, c4.load_eval_keys, path)[0] == ERR_STATE     # other parameters
        finally:
            c4.close()
    finally:
        c2.close()
        c3.close()
        os.remove(path)


def test_bootstrap_setup_names_a_missing_key(fa, tmp_path):
    cl = _client(fa, "boot12", rotations=False)     # relinearisation and conjugation keys, none of the bootstrap's rotations
    path = str(tmp_path / "m.evk")
    try:
        cl.save_eval_keys(path)
        ev = fa.Engine.from_eval_keys(path, seed=1)
        try:
            code, msg = _code(fa, ev.bootstrap_setup, 3, 3, 0)
            assert code == ERR_KEY and "rotation key for index" in msg
        finally:
            ev.close()
    finally:
        cl.close()
        os.remove(path)


def _assert_holds_no_keys(fa, e):
    assert _code(fa, e.key_export, 0)[0] == ERR_KEY
    assert _code(fa, e.key_export, 2)[0] == ERR_KEY
    assert _code(fa, e.encrypt, np.zeros(4))[0] == ERR_KEY


def test_corrupted_sets_are_refused_atomically(fa, tmp_path):
    cl = _client(fa, "toy", rotations=False)
    cl.gen_rotation_keys([1, 2, -1])
    path = str(tmp_path / "c.evk")
    try:
        cl.save_eval_keys(path)
        good = open(path, "rb").read()
        ents = read_table(good)
        N = cl.N
        # one flipped bit in the last payload
        bad = bytearray(good)
        last = ents[-1]
        bad[last["offset"] + 8 * (last["words"] // 2) + 3] ^= 0x10
        open(path, "wb").write(bad)
        e = fa.Engine("toy", seed=2)
        try:
            code, msg = _code(fa, e.load_eval_keys, path)
            assert code == ERR_ARG and "digest" in msg
            _assert_holds_no_keys(fa, e)
            # one residue set to its modulus, with the key's digest recomputed: refused by the range check
            rk = next(x for x in ents if x["kind"] == 1)
            words = np.frombuffer(good, dtype=np.uint64, count=rk["words"], offset=rk["offset"]).copy()
            nl = cl.n_limbs
            j, i = 2 * nl + 3, 77                              # digit 1, component 0, limb 3
            words[j * N + i] = cl.moduli[j % nl]
            bad = bytearray(good)
            bad[rk["offset"]: rk["offset"] + 8 * rk["words"]] = words.tobytes()
            struct.pack_into("<Q", bad, rk["at"] + 32, key_digest(words, N))
            open(path, "wb").write(bad)
            code, msg = _code(fa, e.load_eval_keys, path)
            assert code == ERR_ARG and "residue" in msg, msg
            _assert_holds_no_keys(fa, e)
            # the same context is still fresh: the intact set loads
            open(path, "wb").write(good)
            e.load_eval_keys(path)
            assert np.array_equal(e.key_export(0), cl.key_export(0))
        finally:
            e.close()
    finally:
        cl.close()
        os.remove(path)


def test_digest_kernel_matches_restatement(fa):
    e = fa.Engine("toy13", seed=1)
    try:
        rng = np.random.default_rng(7)
        N, m = e.N, e.moduli
        first = 2
        rows = [rng.integers(0, int(m[first + i]), N, dtype=np.uint64) for i in range(5)]
        rows += [np.full(N, int(m[first + 5]) - 1, dtype=np.uint64), np.zeros(N, dtype=np.uint64)]
        w = np.stack(rows)
        d, ok = e.debug_key_digest(w, first)
        assert ok.all()
        assert [int(v) for v in d] == [limb_digest(r) for r in w]
        w[3, 100] = m[first + 3]                    # == q: out of range
        w[4, 5] = np.uint64(2**64 - 1)
        d, ok = e.debug_key_digest(w, first)
        assert list(ok) == [True, True, True, False, False, True, True]
        assert [int(v) for v in d] == [limb_digest(r) for r in w]
    finally:
        e.close()


def test_reference_whole_pass_on_an_evaluation_context(fa, tmp_path):
    """forward_encrypted at the reference ring on a context loaded from the set: main_2 (no server encryption) bit for bit equal
    to the client's own pass; main (two server encryptions under the evaluation context's public key) within the logits'
    tolerance of tests/test_forward_gpu.py with the same argmax."""
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
        print(f"evaluation-key set at the reference ring: {os.path.getsize(path) / 1e9:.2f} GB")
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
