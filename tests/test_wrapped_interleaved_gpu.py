"""Wrapped inputs of interleaved samples (include/fhelin.h "Wrapped inputs", "Interleaved samples"): a group of s samples travels as
the wrapped ciphertexts of ONE sample - logical slot j*128 + t of sample i in the physical slot s (j*128 + t) + i - and one unwrap
serves every lane.  Checked here through the C ABI: layout, grouping, limbs and exact scales against fhelin_client_ingest_wrapped and
fhelin_client_ingest_interleaved, the unwrapped residues against a restatement from the oracle's primitives (Galois elements
5^(s r)), the sampler draws, the compact round trip into an evaluation context that adopted the stride, the level plan, batching,
the refusals and (FHELIN_SLOW_TESTS=1) the `main` driver at the headline ring.
Rings: the layout needs 16384 logical slots, so stride 2 runs at N = 2^16 and stride 4 at N = 2^17 (tests/test_wrapped_inputs_gpu.py's
TOY chain one and two rings up).  The samples of a group come from different seeds, so that a lane swap shows.
Bounds: a decrypted wrapped ciphertext within 1e-6 and an unwrapped value within 1e-8 * max(1, max|row|), both as
tests/test_wrapped_inputs_gpu.py holds them at stride 1; the measured worst values are printed (one MI355X: layout 6.0e-13 at
stride 2 and 8.5e-13 at stride 4; unwrapped inputs 1.4e-10 at stride 2 and 2.8e-10 at stride 4)."""
import ctypes as C
import os
import struct

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_STATE, ERR_KEY = 1, 4, 5
CHAIN = dict(n_q=5, n_p=2, dnum=3, log_slots=14, hamming=64)
# the unwrap's rotations (include/fhelin.h "Wrapped inputs"): +-1..7, +-8..56 in steps of 8, +-64 - logical indices
UNWRAP_KEYS = [k for k in range(-7, 8) if k] + [8 * k for k in range(-7, 8) if k] + [-64, 64]


def _ring(s):
    return dict(log_n=15 + (s.bit_length() - 1), **CHAIN)


def _shared(S, seed):
    rng = np.random.default_rng(seed)
    return dict(cls=rng.uniform(-1, 1, 128), pos=rng.uniform(-1, 1, (S, 128)), E_w=rng.uniform(-0.1, 0.1, (32, S + 1)),
                E_b=rng.uniform(-0.1, 0.1, 32), F_w=rng.uniform(-0.1, 0.1, (32, S + 1)), F_b=rng.uniform(-0.1, 0.1, 32))


def _embs(S, s, seed):
    return [np.random.default_rng(1000 * seed + i).uniform(-1, 1, (S, 128)) for i in range(s)]


def _engine(fa, s, seed=31, keys=UNWRAP_KEYS, relin=False, **kw):
    e = fa.Engine("toy13", seed=seed, interleave=s, **_ring(s), **kw)
    e.keygen()
    if relin:
        e.gen_relin_key()
    if keys:
        e.gen_rotation_keys(keys)
    return e


def _wrapped_layout(rows):
    out = np.zeros(16384)
    for t, r in enumerate(rows):
        out[t::128] = r
    return out


def _expanded(r):
    return np.repeat(np.asarray(r), 128)


def _flat(r):
    return r["inputs_E"] + r["inputs_F"] + r["inputs"]


def _expand_c1(seed, nonce, limb, q, N):
    """c1 of a seeded ciphertext (include/fhelin.h "Compact ciphertexts"), limb index over Q then P, via fhelin_prng_block"""
    import fhe_linformer_amd as fa
    lib = fa.load_library()
    out = np.empty(N, dtype=np.uint64)
    buf = (C.c_uint8 * 64)()
    sb = (C.c_uint8 * 32)(*seed)
    for b in range(N // 4):
        lib.fhelin_prng_block(sb, C.c_uint64((limb << 32) | b), C.c_uint64(nonce), buf)
        w = np.frombuffer(bytes(buf), dtype="<u8")
        for k in range(4):
            out[4 * b + k] = (int(w[2 * k + 1]) * (1 << 64) + int(w[2 * k])) % q
    return out


@pytest.fixture(scope="module")
def single(fa):
    """a stride-1 client at the stride-1 toy ring: what fhelin_client_ingest_wrapped gives for one sample alone"""
    e = fa.Engine("toy13", seed=31, **_ring(1))
    e.keygen()
    yield e
    e.close()


@pytest.fixture(scope="module")
def eng2(fa):
    e = _engine(fa, 2, relin=True)
    yield e
    e.close()


# ---- 1. layout, grouping, limbs, scales ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", [2, 4])
def test_layout_grouping_limbs_and_scales(fa, single, eng2, s):
    e = eng2 if s == 2 else _engine(fa, 4)
    try:
        S = 70
        n = 64 + S + 1
        sh, embs = _shared(S, 3), _embs(S, s, 3)
        # 132 inputs at n_q: one full ciphertext over the p_0 limb and a partial one of 4; three inputs at 2 limbs
        targets = [e.n_q] * 32 + [2] * 3 + [e.n_q] * (n - 35)
        ws, x_in, proj = e.client_ingest_wrapped_interleaved(**sh, embs=embs, targets=targets, want_proj=True)
        assert len(ws) == 3
        infos = [w.wrapped_info() for w in ws]
        rows = []
        for i in range(s):      # per sample: the single-sample call on a stride-1 engine gives the same grouping and, bit for bit, the rows
            w1, x1, p1 = single.client_ingest_wrapped(**sh, emb=embs[i], targets=targets, want_proj=True)
            assert [w.wrapped_info() for w in w1] == infos
            assert np.array_equal(x1, x_in[i]) and np.array_equal(p1, proj[i])
            rows.append(np.vstack([proj[i], x_in[i]]))
        assert np.max(np.abs(rows[0] - rows[1])) > 0.1                      # the lanes differ
        assert [i["ell"] for i in infos] == [e.n_q, e.n_q, 2] and [i["count"] for i in infos] == [128, 4, 3]
        assert infos[0]["positions"] == list(range(32)) + list(range(35, 131)) and infos[1]["positions"] == list(range(131, n))
        assert infos[2]["positions"] == [32, 33, 34]
        assert [w.info()["level"] for w in ws] == [0, 0, e.n_q - 2]
        worst_w = 0.0
        for w, i in zip(ws, infos):
            assert w.info()["ell"] == i["ell"] + 1 and i["total"] == n and w.info()["slots"] == 16384     # logical slots
            got = e.decrypt_interleaved(w, 16384)
            assert got.shape == (s, 16384)
            for lane in range(s):
                worst_w = max(worst_w, np.max(np.abs(got[lane] - _wrapped_layout(rows[lane][i["positions"]]))))
            assert np.array_equal(e.decrypt(w, 16384), got[0])                                            # decrypt: sample 0
            assert np.array_equal(e.decrypt_batch([w], 16384, all_lanes=True)[0], got)
        print(f"stride {s}: max wrapped-layout error = {worst_w:.3e}")
        assert worst_w < 1e-6
        outs = e.unwrap_inputs(ws)
        assert len(outs) == n
        ref, ref2 = _flat(e.client_ingest_interleaved(**sh, embs=embs, level=0)), _flat(e.client_ingest_interleaved(**sh, embs=embs, level=e.n_q - 2))
        for v in range(n):
            r = ref2[v] if 32 <= v < 35 else ref[v]
            a, b = outs[v].info(), r.info()
            assert (a["ell"], a["deg"], a["slots"]) == (b["ell"], b["deg"], b["slots"]) == (targets[v], 1, 16384)
            assert outs[v].scale_parts() == r.scale_parts()
        got = e.decrypt_batch(outs, 16384, all_lanes=True)                   # [n][s][16384]
        worst, per_lane = 0.0, []
        for lane in range(s):
            w_l = max(np.max(np.abs(got[v, lane] - _expanded(rows[lane][v]))) / max(1.0, np.max(np.abs(rows[lane][v]))) for v in range(n))
            per_lane.append(w_l)
            worst = max(worst, w_l)
        print(f"stride {s}: max unwrapped input error / max(1, max|row|) per lane = " + ", ".join(f"{x:.3e}" for x in per_lane))
        assert worst < 1e-8
        with pytest.raises(fa.FhelinError) as ex:                            # every other entry point still refuses a wrapped handle
            e.add(ws[0], ws[0])
        assert ex.value.code == ERR_ARG
    finally:
        if s != 2:
            e.close()


# ---- 2. residues equal a restatement ---------------------------------------------------------------------------------------------
def test_residues_equal_a_restatement(fa, eng2, orc):
    """the unwrap outputs bit for bit = the masked drop (oracle product and rescale over the extended basis, the replicated mask
    read through the automorphism of rotation -t s) followed by three merged rotate-and-sums with the Galois elements 5^(s k)"""
    e, s = eng2, 2
    S = 70
    n = 64 + S + 1
    targets = [e.n_q] * 128 + [3] * (n - 128)                 # one full ciphertext over the p_0 limb, one of 7 at 3 limbs
    ws = e.client_ingest_wrapped_interleaved(**_shared(S, 5), embs=_embs(S, s, 5), targets=targets)
    outs = e.unwrap_inputs(ws)
    blobs = [w.export_compact() for w in ws]
    moduli = [int(m) for m in list(e.q) + list(e.p)]
    psi = [int(r) for r in list(e.psi_q) + list(e.psi_p)]
    mask = np.zeros(16384)
    mask[::128] = 1.0
    pt = e.encode(mask)                                       # replicated into both lanes
    full = e.n_q + e.p.size
    picks = {0: [0, 9, 45, 63, 64, 100, 127], 1: [0, 6]}      # every a, b >= 5 and both c: R1, R2, R3 with all their offset sets
    evk = {}
    for wi, w in enumerate(ws):
        inf = w.wrapped_info()
        ell1 = inf["ell"] + 1
        blob = blobs[wi]
        seed, nonce = bytes(blob[56:88]), struct.unpack_from("<Q", blob, 48)[0]
        c0 = np.frombuffer(blob, dtype="<u8", count=ell1 * e.N, offset=len(blob) - 8 * ell1 * e.N).reshape(ell1, e.N)
        c1 = np.stack([_expand_c1(seed, nonce, l, moduli[l], e.N) for l in range(ell1)])
        W = np.stack([c0, c1])
        q = moduli[ell1 - 1]                                  # p_0 has 60 bits: the scale travels exactly, as hi + lo doubles
        m0 = e.pt_export(pt, full, np.longdouble(q >> 32) * np.longdouble(2 ** 32) + np.longdouble(q & 0xffffffff))[:ell1]
        assert inf["count"] == (128 if wi == 0 else 7)
        for t in picks[wi]:
            g = orc.galois(e.log_n, -t * s)
            mt = np.stack([orc.automorph_ntt(m0[l], g) for l in range(ell1)])
            qs = np.array(moduli[:ell1], dtype=np.uint64)
            y = np.stack([orc.mul(W[p], mt, qs) for p in range(2)])
            x = orc.rescale(y, qs, np.array(psi[:ell1], dtype=np.uint64))
            a, b, c = t % 8, (t // 8) % 8, t // 64
            for offs in ([k for k in range(a - 7, a + 1) if k], [8 * k for k in range(b - 7, b + 1) if k], [64 if c else -64]):
                for k in offs:
                    if k not in evk:
                        evk[k] = e.key_export(1, k)
                x = orc.rotate_sum(x, np.stack([evk[k] for k in offs]), [orc.galois(e.log_n, k * s) for k in offs], e.alpha, e.q, e.p,
                                   e.psi_q, e.psi_p)
            got = outs[inf["positions"][t]].export()
            assert np.array_equal(got, x), (wi, t)


# ---- 3. sampler draws are those of one call ----------------------------------------------------------------------------------------
def test_sampler_draws_are_those_of_one_call(fa):
    S = 8
    sh, embs = _shared(S, 6), _embs(S, 2, 6)
    targets = [5] * 40 + [2] * (64 + S + 1 - 40)
    ring = _ring(2)
    A = fa.Engine("toy13", seed=77, **ring)                   # stride 1
    B = fa.Engine("toy13", seed=77, interleave=2, **ring)     # stride 2, the same ring and seed
    try:
        for e in (A, B):
            e.keygen()
        blobs = []
        for e, call in ((A, lambda t: A.client_ingest_wrapped(**sh, emb=embs[0], targets=t)),
                        (B, lambda t: B.client_ingest_wrapped_interleaved(**sh, embs=embs, targets=t))):
            got = []
            for t in (targets, None):                         # two calls each: a fresh seed per call
                got += [w.export_compact() for w in call(t)]
            blobs.append(got)
        assert len(blobs[0]) == len(blobs[1]) == 3
        for a, b in zip(*blobs):
            assert a[56:88] == b[56:88] and a[48:56] == b[48:56]          # seed and nonce
            assert len(a) == len(b)                                       # a group in the bytes of one sample
        assert blobs[0][0][56:88] != blobs[0][2][56:88]
        ka, kb = A.debug_sampler_peek(2), B.debug_sampler_peek(2)
        assert ka[1] == kb[1] and np.array_equal(ka[0], kb[0])
        # at stride 1 with one sample the new call is fhelin_client_ingest_wrapped itself
        A2 = fa.Engine("toy13", seed=77, **ring)
        try:
            A2.keygen()
            mine = []
            for t in (targets, None):
                mine += [w.export_compact() for w in A2.client_ingest_wrapped_interleaved(**sh, embs=[embs[0]], targets=t)]
            assert mine == blobs[0]
            k2 = A2.debug_sampler_peek(2)
            assert k2[1] == ka[1] and np.array_equal(k2[0], ka[0])
        finally:
            A2.close()
    finally:
        A.close()
        B.close()


# ---- 4. compact round trip into an evaluation context; the missing key --------------------------------------------------------------
def test_compact_round_trip_eval_context_and_missing_key(fa, tmp_path):
    s, S = 2, 8
    sh, embs = _shared(S, 7), _embs(S, s, 7)
    path = str(tmp_path / "s2.evc")
    cl = fa.Engine("toy13", seed=42, interleave=s, **_ring(s))
    try:
        cl.set_seeded_keys(True)
        cl.keygen()
        cl.gen_rotation_keys(UNWRAP_KEYS)
        cl.save_eval_keys(path, compact=True)
        ev = fa.Engine.from_eval_keys(path, seed=43)
        try:
            assert ev.interleave == s                                      # the key set carries the stride
            ws = cl.client_ingest_wrapped_interleaved(**sh, embs=embs, targets=[5] * 60 + [3] * (64 + S + 1 - 60))
            blobs = [w.export_compact() for w in ws]
            for w, b in zip(ws, blobs):                                    # no format change: version 2, the stride-1 size
                i = w.wrapped_info()
                ell1 = i["ell"] + 1
                assert struct.unpack_from("<I", b, 8)[0] == 2
                assert len(b) == 104 + 8 * ell1 + 8 * ((i["count"] + 1) // 2) + 8 * ell1 * cl.N == w.compact_bytes()
            imp = ev.import_compact(blobs)
            assert [w.wrapped_info() for w in imp] == [w.wrapped_info() for w in ws]
            assert all(w.info()["slots"] == 16384 for w in imp)
            srv, own = ev.unwrap_inputs(imp), cl.unwrap_inputs(ws)
            assert len(srv) == len(own) == 64 + S + 1
            for x, y in zip(srv, own):
                assert x.info() == y.info() and x.scale_parts() == y.scale_parts()
                assert np.array_equal(x.export(), y.export())
            with pytest.raises(fa.FhelinError) as ex:                      # the client side needs the secret
                ev.client_ingest_wrapped_interleaved(**sh, embs=embs)
            assert ex.value.code == ERR_KEY
        finally:
            ev.close()
    finally:
        cl.close()
        if os.path.exists(path):
            os.remove(path)
    short = _engine(fa, s, seed=42, keys=[k for k in UNWRAP_KEYS if k != -56])
    try:
        ws = short.client_ingest_wrapped_interleaved(**sh, embs=embs)
        short.level_plan_begin("record")
        before, tell = short.stats(), short.level_plan_tell()
        with pytest.raises(fa.FhelinError) as ex:
            short.unwrap_inputs(ws)
        assert ex.value.code == ERR_KEY and "-56" in str(ex.value) and "-112" not in str(ex.value)    # the LOGICAL index
        after = short.stats()
        assert all(after[k] == before[k] for k in ("limb_ntt", "keyswitch", "rescale", "ct_pt_mult")) and short.level_plan_tell() == tell
        short.level_plan_end()
    finally:
        short.close()


# ---- 5. level plan -----------------------------------------------------------------------------------------------------------------
def test_level_plan_recorded_with_interleaved_ingest_applies_to_wrapped(eng2):
    e, s, S = eng2, 2, 8
    sh, embs = _shared(S, 11), _embs(S, s, 11)
    n = 64 + S + 1

    def program(wrapped):
        if wrapped:
            outs = e.unwrap_inputs(e.client_ingest_wrapped_interleaved(**sh, embs=embs))
        else:
            outs = _flat(e.client_ingest_interleaved(**sh, embs=embs))
        d = e.rescale(e.mult(outs[0], outs[64]))
        e.decrypt(e.rescale(e.mult(d, outs[1])))
        e.decrypt(outs[65])
        return outs

    try:
        e.level_plan_begin("record")
        program(False)
        plan = e.level_plan_end()
        e.level_plan_begin("apply")
        want = [c.info()["ell"] for c in program(False)]
        e.level_plan_end()
        e.level_plan_begin("apply")
        ws = e.client_ingest_wrapped_interleaved(**sh, embs=embs)            # the peek: every input wrapped at its planned limbs
        e.level_plan_end()
        e.level_plan_begin("apply")
        outs = program(True)
        e.level_plan_end()
        assert [c.info()["ell"] for c in outs] == want, (plan, want)
        assert min(want) < e.n_q and len(set(want)) > 1
        assert sorted({w.info()["ell"] - 1 for w in ws}) == sorted(set(want))
        # a client without the plan wraps everything at n_q limbs; the server applying the plan makes each output at its planned limbs
        # with the fresh scale there, as the interleaved ingest's planned output
        e.level_plan_begin("apply")
        regular = _flat(e.client_ingest_interleaved(**sh, embs=embs))
        e.level_plan_end()
        full, x_in, proj = e.client_ingest_wrapped_interleaved(**sh, embs=embs, want_proj=True)
        assert {w.info()["ell"] for w in full} == {e.n_q + 1}
        e.level_plan_begin("apply")
        low = e.unwrap_inputs(full)
        e.level_plan_end()
        assert [c.info()["ell"] for c in low] == want
        assert [c.scale_parts() for c in low] == [c.scale_parts() for c in regular]
        for v in (0, 40, 64, 64 + S):
            got = e.decrypt_interleaved(low[v], 16384)
            for lane in range(s):
                row = np.vstack([proj[lane], x_in[lane]])[v]
                assert np.max(np.abs(got[lane] - _expanded(row))) < 1e-8 * max(1.0, np.max(np.abs(row)))
        assert len(low) == n
    finally:
        if e.level_plan_tell()[0] != "off":
            e.level_plan_end()


# ---- 6. batch ------------------------------------------------------------------------------------------------------------------------
def test_two_groups_in_one_unwrap(eng2):
    e, s, S = eng2, 2, 8
    sh = _shared(S, 12)
    w1 = e.client_ingest_wrapped_interleaved(**sh, embs=_embs(S, s, 12))
    w2 = e.client_ingest_wrapped_interleaved(**sh, embs=_embs(S, s, 13))
    both = e.unwrap_inputs(w1 + w2)
    one, two = e.unwrap_inputs(w1), e.unwrap_inputs(w2)
    assert len(both) == len(one) + len(two) == 2 * (64 + S + 1)
    for x, y in zip(both, one + two):
        assert np.array_equal(x.export(), y.export())


def test_batched_controller_wrapped_route(fa):
    """ingest_sample(BatchedController, wrapped=True) at stride 2: one group per batch entry, all groups unwrapped in one call, every
    lane of every entry within the bound of its own sample's expanded row; the single controller's route likewise"""
    from fhe_linformer_amd import linformer as lf
    from oracle import plain_forward as pf
    s, S, B = 2, 6, 2
    e = _engine(fa, s, keys=fa.circuit_rotation_indices())
    try:
        w = pf.synthetic_model(1234)
        xs = [[pf.synthetic_tokens(S, 50 + 10 * x + i) for i in range(s)] for x in range(B)]
        before = e.stats()["ct_pt_mult"]
        enc = lf.ingest_sample(lf.BatchedController(e, B), w, xs, wrapped=True)
        assert e.stats()["ct_pt_mult"] - before == B * (64 + S + 1)
        assert [len(enc[k]) for k in ("inputs_E", "inputs_F", "inputs")] == [32, 32, S + 1]
        one = lf.ingest_sample(lf.GpuController(e), w, xs[1], wrapped=True)
        for x in range(B):
            ins = [pf.client_inputs(w, xs[x][i]) for i in range(s)]
            for k, i, pick in (("inputs_E", 3, lambda c: c[1][3]), ("inputs_F", 31, lambda c: c[2][31]), ("inputs", 0, lambda c: c[0][0]),
                               ("inputs", S, lambda c: c[0][S])):
                ct = enc[k][i][x]
                assert ct.info()["ell"] == e.n_q and ct.info()["slots"] == 16384
                for c, name in ((ct, "batched"),) + (((one[k][i], "single"),) if x == 1 else ()):
                    got = e.decrypt_interleaved(c, 16384)
                    for lane in range(s):
                        row = pick(ins[lane])
                        assert np.max(np.abs(got[lane] - _expanded(row))) < 1e-8 * max(1.0, np.max(np.abs(row))), (name, x, k, i, lane)
    finally:
        e.close()


# ---- 7. refusals -------------------------------------------------------------------------------------------------------------------
def _raw(e, embs, tokens, table, S, sh, level=0, targets=None, n_samples=None):
    """the C call itself: (return code, *n_out, the handles it left)"""
    f = lambda a: np.ascontiguousarray(a, dtype=np.float64)
    keep = [f(sh[k]) for k in ("cls", "pos", "E_w", "E_b", "F_w", "F_b")]
    p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None
    xs = [None if x is None else (f(x) if embs is not None else np.ascontiguousarray(x, dtype=np.int32)) for x in (embs if embs is not None else tokens)]
    ptrs = (C.c_void_p * len(xs))(*[None if x is None else x.ctypes.data for x in xs])
    tab = f(table) if table is not None else None
    tg = np.ascontiguousarray(targets, dtype=np.int32) if targets is not None else None
    outs = (C.c_void_p * (64 + S + 1))()
    n_out = C.c_int32(-1)
    rc = e.lib.fhelin_client_ingest_wrapped_interleaved(e.h, len(xs) if n_samples is None else n_samples, ptrs if embs is not None else None,
                                                        ptrs if embs is None else None, p(tab), tab.shape[0] if tab is not None else 0, S,
                                                        *[p(a) for a in keep], keep[2].shape[1], level, p(tg), outs, C.byref(n_out), None)
    return rc, n_out.value, [h for h in outs if h]


def test_refusals(fa, eng2):
    e, s, S = eng2, 2, 8
    sh, embs = _shared(S, 14), _embs(S, s, 14)
    n = 64 + S + 1
    table = np.random.default_rng(15).uniform(-1, 1, (20, 128))
    toks = [np.arange(S) % 20, (np.arange(S) + 3) % 20]
    bad_tok = [toks[0], toks[1].copy()]
    bad_tok[1][S - 1] = 20
    e.level_plan_begin("record")
    try:
        before, tell = e.stats(), e.level_plan_tell()
        cases = [
            ("n_samples != stride", dict(embs=embs + embs[:1], tokens=None, table=None), ERR_ARG),
            ("one sample at stride 2", dict(embs=embs[:1], tokens=None, table=None), ERR_ARG),
            ("a NULL sample pointer", dict(embs=[embs[0], None], tokens=None, table=None), ERR_ARG),
            ("a NULL token list", dict(embs=None, tokens=[toks[0], None], table=table), ERR_ARG),
            ("a token id out of range", dict(embs=None, tokens=bad_tok, table=table), ERR_ARG),
            ("targets out of range (0)", dict(embs=embs, tokens=None, table=None, targets=[0] + [2] * (n - 1)), ERR_ARG),
            ("targets out of range (n_q + 1)", dict(embs=embs, tokens=None, table=None, targets=[2] * (n - 1) + [e.n_q + 1]), ERR_ARG),
            ("level out of range", dict(embs=embs, tokens=None, table=None, level=e.n_q), ERR_ARG),
        ]
        for what, kw, code in cases:
            rc, n_out, left = _raw(e, S=S, sh=sh, **kw)
            assert (rc, n_out, left) == (code, 0, []), what
        after = e.stats()
        assert all(after[k] == before[k] for k in ("limb_ntt", "encode", "ct_pt_mult")) and e.level_plan_tell() == tell
        assert _raw(e, embs=None, tokens=toks, table=table, S=S, sh=sh)[:2] == (0, 1)     # the token route itself works
        assert e.level_plan_tell() == tell                                                # and is no level-plan source
    finally:
        e.level_plan_end()
    with pytest.raises(fa.FhelinError) as ex:                                             # the single-sample call still refuses a stride
        e.client_ingest_wrapped(**sh, emb=embs[0])
    assert ex.value.code == ERR_STATE
    nop = fa.Engine("toy13", seed=5, interleave=2, **dict(_ring(2), n_p=0))         # no special prime: no p_0 limb
    try:
        nop.keygen()
        assert _raw(nop, embs=embs, tokens=None, table=None, S=S, sh=sh) == (ERR_STATE, 0, [])
    finally:
        nop.close()


# ---- 8. the driver -------------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not os.environ.get("FHELIN_SLOW_TESTS"), reason="a whole forward pass at N=2^16, 28+7 limbs; FHELIN_SLOW_TESTS=1 runs it "
                    "(recorded: profiles/wrapped_interleaved_forward_test.txt)")
def test_driver_on_wrapped_interleaved_inputs_matches_the_circuit_oracle_per_lane(fa):
    from fhe_linformer_amd import linformer as lf
    from oracle import plain_forward as pf, circuit_sim as cs
    LOGIT_TOL = 1.2e-2          # tests/test_forward_gpu.py
    S, s = 129, 2
    w = pf.synthetic_model(1234)
    xs = [pf.synthetic_tokens(S, 4321 + i) for i in range(s)]
    refs = [lf.logits_from_slots(lf.forward(cs.SlotSimController(), w, *pf.client_inputs(w, x), None, "main")) for x in xs]
    assert np.max(np.abs(refs[0] - refs[1])) > 10 * LOGIT_TOL          # a lane swap cannot pass
    eng = fa.Engine("bench", seed=11, n_q=28, n_p=-1, interleave=s)
    try:
        eng.keygen()
        eng.gen_relin_key()
        eng.gen_rotation_keys(fa.circuit_rotation_indices())
        eng.bootstrap_setup(3, 3, 16384)
        ctl = lf.GpuController(eng)
        x0 = [pf.synthetic_tokens(S, 4300 + i) for i in range(s)]
        eng.level_plan_begin("record")                                  # recorded with the regular interleaved ingest
        ctl.decrypt_lanes(lf.forward_encrypted(ctl, w, lf.ingest_sample(ctl, w, x0), None, "main"))
        targets = eng.level_plan_end()
        eng.level_plan_begin("apply")
        enc = lf.ingest_sample(ctl, w, xs, wrapped=True)
        assert [c.info()["ell"] for c in _flat(enc)] == [t if t > 0 else eng.n_q for t in targets[:64 + S + 1]]
        lanes = ctl.decrypt_lanes(lf.forward_encrypted(ctl, w, enc, None, "main"))
        eng.level_plan_end()
        for i in range(s):
            lg = lf.logits_from_slots(lanes[i])
            err = np.max(np.abs(lg - refs[i]))
            print(f"wrapped interleaved main bench S={S} lane {i}: logits {err:.2e} (< {LOGIT_TOL:.0e})")
            assert err < LOGIT_TOL, (i, err)
            assert int(np.argmax(lg)) == int(np.argmax(refs[i])), i
    finally:
        eng.close()
