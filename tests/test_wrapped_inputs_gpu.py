"""Wrapped inputs on the GPU (include/fhelin.h "Wrapped inputs"): the client packs a sample's 64 + S + 1 inputs into a few wrapped
ciphertexts over one limb more than the inputs need; the server unwraps them into what fhelin_client_ingest gives.  Checked here:
the wrapped layout and grouping, the unwrapped values, limbs and exact scales, the residues against a restatement (masked drop and
merged rotate-and-sum key switches from the oracle's primitives), the compact form version 2, batching, evaluation contexts, the
missing-key refusal and the level plan.  Error bound of an unwrapped value: 1e-8 * max(1, max|row|) (not measured beforehand:
about 100x an estimate of fresh noise plus three key switches; the measured value is printed)."""
import os
import struct

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_KEY = 1, 5
TOY = dict(log_n=15, n_q=5, n_p=2, dnum=3, log_slots=14, hamming=64)   # the smallest ring with the 16384 slots of the layout


def _inputs(S, seed):
    rng = np.random.default_rng(seed)
    return dict(cls=rng.uniform(-1, 1, 128), pos=rng.uniform(-1, 1, (S, 128)), E_w=rng.uniform(-0.1, 0.1, (32, S + 1)),
                E_b=rng.uniform(-0.1, 0.1, 32), F_w=rng.uniform(-0.1, 0.1, (32, S + 1)), F_b=rng.uniform(-0.1, 0.1, 32),
                emb=rng.uniform(-1, 1, (S, 128)))


def _client(fa, preset, seed=31, **over):
    e = fa.Engine(preset, seed=seed, **over)
    e.keygen()
    e.gen_rotation_keys(fa.circuit_rotation_indices())
    return e


def _expand_c1(seed, nonce, limb, q, N):
    """c1 of a seeded ciphertext (include/fhelin.h "Compact ciphertexts"), limb index over Q then P, via fhelin_prng_block"""
    import fhe_linformer_amd as fa
    import ctypes as C
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


def _proj_row(inp, i):
    """input i of a sample in read order, in NumPy (dimReduce.py:141-160 as the device computes it, up to rounding)"""
    S = inp["emb"].shape[0]
    x_in = np.vstack([inp["cls"].reshape(1, -1), inp["emb"] + inp["pos"][:S] / 3.0])
    if i < 32:
        return inp["E_w"][i] @ x_in + inp["E_b"][i]
    if i < 64:
        return inp["F_w"][i - 32] @ x_in + inp["F_b"][i - 32]
    return x_in[i - 64]


def _rows(proj, x_in):
    return np.vstack([proj, x_in])          # read order: E rows, F rows, tokens


def _wrapped_layout(rows):
    out = np.zeros(16384)
    for t, r in enumerate(rows):
        out[t::128] = r
    return out


def _expanded(r):
    return np.repeat(np.asarray(r), 128)


@pytest.mark.parametrize("preset,over", [("toy13", TOY), ("bench", {})])
def test_layout_values_limbs_and_scales(fa, preset, over):
    e = _client(fa, preset, **over)
    try:
        S = 100
        inp = _inputs(S, 3)
        n = 64 + S + 1
        targets = [e.n_q] * 32 + [2] * 32 + [e.n_q] * (S + 1)   # n_q exercises the p_0 limb; 133 inputs at n_q fill t = 0..127
        ws, x_in, proj = e.client_ingest_wrapped(**inp, targets=targets, want_proj=True)
        rows = _rows(proj, x_in)
        assert len(ws) == 3
        infos = [w.wrapped_info() for w in ws]
        assert [i["ell"] for i in infos] == [e.n_q, e.n_q, 2] and [i["count"] for i in infos] == [128, 5, 32]
        assert infos[0]["positions"] == list(range(32)) + list(range(64, 160)) and infos[1]["positions"] == list(range(160, n))
        assert infos[2]["positions"] == list(range(32, 64))
        assert [w.info()["level"] for w in ws] == [0, 0, e.n_q - 2]
        for w, i in zip(ws, infos):
            assert w.info()["ell"] == i["ell"] + 1 and i["total"] == n
            got = e.decrypt(w, 16384)
            want = _wrapped_layout(rows[i["positions"]])
            assert np.max(np.abs(got - want)) < 1e-6, np.max(np.abs(got - want))
        outs = e.unwrap_inputs(ws)
        assert len(outs) == n
        ref = e.client_ingest(**inp, level=0)
        ref = ref["inputs_E"] + ref["inputs_F"] + ref["inputs"]
        ref2 = e.client_ingest(**inp, level=e.n_q - 2)
        ref2 = ref2["inputs_E"] + ref2["inputs_F"] + ref2["inputs"]
        worst = 0.0
        for v in range(n):
            r = ref2[v] if 32 <= v < 64 else ref[v]
            a, b = outs[v].info(), r.info()
            assert (a["ell"], a["deg"], a["slots"]) == (b["ell"], b["deg"], b["slots"]) == (targets[v], 1, 16384)
            assert outs[v].scale_parts() == r.scale_parts()
            err = np.max(np.abs(e.decrypt(outs[v], 16384) - _expanded(rows[v])))
            worst = max(worst, err / max(1.0, np.max(np.abs(rows[v]))))
        print(f"{preset}: max unwrapped input error / max(1, max|row|) = {worst:.3e}")
        assert worst < 1e-8
        # every other entry point refuses a wrapped handle
        with pytest.raises(fa.FhelinError) as ex:
            e.add(ws[0], ws[0])
        assert ex.value.code == ERR_ARG
        with pytest.raises(fa.FhelinError) as ex:
            ws[0].export()
        assert ex.value.code == ERR_ARG
    finally:
        e.close()


def test_headline_grouping_default(fa):
    e = _client(fa, "bench")
    try:
        S = 129
        ws = e.client_ingest_wrapped(**_inputs(S, 4))
        assert [w.wrapped_info()["count"] for w in ws] == [128, 66]
        assert [w.info()["ell"] for w in ws] == [e.n_q + 1] * 2
    finally:
        e.close()


def test_residues_equal_a_restatement(fa):
    """toy ring: the unwrap outputs bit for bit = the masked drop (oracle product and rescale over the extended basis, the mask
    read through the automorphism of rotation -t) followed by three merged rotate-and-sums from the oracle"""
    import oracle as orc
    e = _client(fa, "toy13", **TOY)
    try:
        S = 70
        n = 64 + S + 1
        targets = [e.n_q] * 128 + [3] * (n - 128)                 # one full ciphertext over the p_0 limb, one of 7 at 3 limbs
        ws = e.client_ingest_wrapped(**_inputs(S, 5), targets=targets)
        outs = e.unwrap_inputs(ws)
        blobs = [w.export_compact() for w in ws]
        moduli = [int(m) for m in list(e.q) + list(e.p)]
        psi = [int(r) for r in list(e.psi_q) + list(e.psi_p)]
        mask = np.zeros(16384)
        mask[::128] = 1.0
        pt = e.encode(mask)
        full = e.n_q + e.p.size
        picks = {0: [0, 9, 45, 63, 64, 100, 127], 1: [0, 6]}      # every a, b >= 5 and both c: R1, R2, R3 with all their offset sets
        for wi, w in enumerate(ws):
            inf = w.wrapped_info()
            ell1 = inf["ell"] + 1
            blob = blobs[wi]
            seed, nonce = bytes(blob[56:88]), struct.unpack_from("<Q", blob, 48)[0]
            c0 = np.frombuffer(blob, dtype="<u8", count=ell1 * e.N, offset=len(blob) - 8 * ell1 * e.N).reshape(ell1, e.N)
            c1 = np.stack([_expand_c1(seed, nonce, l, moduli[l], e.N) for l in range(ell1)])
            W = np.stack([c0, c1])
            m0 = e.pt_export(pt, full, float(moduli[ell1 - 1]))[:ell1]
            assert inf["count"] == (128 if wi == 0 else 7)
            for t in picks[wi]:
                g = orc.galois(e.log_n, -t)
                mt = np.stack([orc.automorph_ntt(m0[l], g) for l in range(ell1)])
                qs = np.array(moduli[:ell1], dtype=np.uint64)
                y = np.stack([orc.mul(W[p], mt, qs) for p in range(2)])
                x = orc.rescale(y, qs, np.array(psi[:ell1], dtype=np.uint64))
                a, b, c = t % 8, (t // 8) % 8, t // 64
                for offs in ([k for k in range(a - 7, a + 1) if k], [8 * k for k in range(b - 7, b + 1) if k], [64 if c else -64]):
                    evks = np.stack([e.key_export(1, k) for k in offs])
                    x = orc.rotate_sum(x, evks, [orc.galois(e.log_n, k) for k in offs], e.alpha, e.q, e.p, e.psi_q, e.psi_p)
                got = outs[inf["positions"][t]].export()
                assert np.array_equal(got, x), (wi, t)
    finally:
        e.close()


def test_compact_round_trip_and_refusals(fa):
    e = _client(fa, "toy13", **TOY)
    try:
        S = 3
        ws = e.client_ingest_wrapped(**_inputs(S, 6), targets=[e.n_q] * 50 + [2] * (64 + S + 1 - 50))
        blobs = [w.export_compact() for w in ws]
        for w, b in zip(ws, blobs):
            i = w.wrapped_info()
            ell1 = i["ell"] + 1
            assert len(b) == 104 + 8 * ell1 + 8 * ((i["count"] + 1) // 2) + 8 * ell1 * e.N == w.compact_bytes()
            assert fa.compact_info(b)["ell"] == ell1
        imp = e.import_compact(blobs)
        assert [w.wrapped_info() for w in imp] == [w.wrapped_info() for w in ws]
        a, b = e.unwrap_inputs(ws), e.unwrap_inputs(imp)
        for x, y in zip(a, b):
            assert np.array_equal(x.export(), y.export())
        bad = bytearray(blobs[0])
        H = len(bad) - 8 * (e.n_q + 1) * e.N
        bad[H + 3] ^= 1                                              # a flipped residue
        wrong_count = bytearray(blobs[0])
        wrong_count[96:100] = struct.pack("<I", ws[0].wrapped_info()["count"] - 1)
        wrong_mod = bytearray(blobs[0])
        wrong_mod[104 + 8 * e.n_q] ^= 2                              # p_0 changed
        for blob in (bad, wrong_count, wrong_mod):
            with pytest.raises(fa.FhelinError) as ex:
                e.import_compact([blobs[1], bytes(blob)])
            assert ex.value.code == ERR_ARG
        e.set_seeded_encryption(True)
        v1 = e.encrypt(np.ones(16384)).export_compact()             # version 1 unchanged
        assert e.import_compact([v1])[0].info()["ell"] == e.n_q
    finally:
        e.close()


def test_batched_unwrap_eval_context_and_missing_key(fa, tmp_path):
    e = _client(fa, "toy13", seed=41, **TOY)
    path = str(tmp_path / "toy.evc")
    try:
        S = 2
        w1 = e.client_ingest_wrapped(**_inputs(S, 7))
        w2 = e.client_ingest_wrapped(**_inputs(S, 8))
        both = e.unwrap_inputs(w1 + w2)
        one, two = e.unwrap_inputs(w1), e.unwrap_inputs(w2)
        assert len(both) == len(one) + len(two)
        for x, y in zip(both, one + two):
            assert np.array_equal(x.export(), y.export())
    finally:
        e.close()
    cl = fa.Engine("toy13", seed=42, **TOY)
    try:
        cl.set_seeded_keys(True)
        cl.keygen()
        keys = fa.circuit_rotation_indices()
        cl.gen_rotation_keys(keys)
        cl.save_eval_keys(path, compact=True)
        ev = fa.Engine.from_eval_keys(path, seed=43)
        try:
            inp = _inputs(2, 9)
            ws = cl.client_ingest_wrapped(**inp)
            srv = ev.unwrap_inputs(ev.import_compact([w.export_compact() for w in ws]))
            own = cl.unwrap_inputs(ws)
            for x, y in zip(srv, own):
                assert np.array_equal(x.export(), y.export())
        finally:
            ev.close()
        short = fa.Engine("toy13", seed=42, **TOY)
        try:
            short.keygen()
            short.gen_rotation_keys([k for k in keys if k != -56])
            ws = short.client_ingest_wrapped(**_inputs(2, 10))
            with pytest.raises(fa.FhelinError) as ex:
                short.unwrap_inputs(ws)
            assert ex.value.code == ERR_KEY and "-56" in str(ex.value)
        finally:
            short.close()
    finally:
        cl.close()
        if os.path.exists(path):
            os.remove(path)


def test_level_plan_recorded_with_regular_ingest_applies_to_wrapped(fa):
    e = _client(fa, "bench")
    try:
        e.gen_relin_key()
        S = 3
        inp = _inputs(S, 11)

        def program(wrapped):
            if wrapped:
                outs = e.unwrap_inputs(e.client_ingest_wrapped(**inp))
            else:
                r = e.client_ingest(**inp)
                outs = r["inputs_E"] + r["inputs_F"] + r["inputs"]
            d = e.rescale(e.mult(outs[0], outs[64]))
            e.decrypt(e.rescale(e.mult(d, outs[1])))
            e.decrypt(outs[65])
            return outs

        e.level_plan_begin("record")
        program(False)
        plan = e.level_plan_end()
        e.level_plan_begin("apply")
        want = [c.info()["ell"] for c in program(False)]
        e.level_plan_end()
        e.level_plan_begin("apply")
        ws = e.client_ingest_wrapped(**inp)
        e.level_plan_end()
        e.level_plan_begin("apply")
        outs = program(True)
        e.level_plan_end()
        assert [c.info()["ell"] for c in outs] == want, (plan, want)
        assert min(want) < e.n_q and len(set(want)) > 1
        assert sorted({w.info()["ell"] - 1 for w in ws}) == sorted(set(want))
        # a client without the plan wraps everything at n_q limbs; the server applying the plan makes each output at its planned limbs
        # with the fresh scale there, as the regular ingest's planned output
        e.level_plan_begin("apply")
        r = e.client_ingest(**inp)
        e.level_plan_end()
        regular = r["inputs_E"] + r["inputs_F"] + r["inputs"]
        full = e.client_ingest_wrapped(**inp)
        assert {w.info()["ell"] for w in full} == {e.n_q + 1}
        e.level_plan_begin("apply")
        low = e.unwrap_inputs(full)
        e.level_plan_end()
        assert [c.info()["ell"] for c in low] == want
        assert [c.scale_parts() for c in low] == [c.scale_parts() for c in regular]
        rows = np.vstack([np.asarray([_proj_row(inp, i) for i in range(64 + S + 1)])])
        for v in (0, 40, 64, 64 + S):
            assert np.max(np.abs(e.decrypt(low[v], 16384) - _expanded(rows[v]))) < 1e-8 * max(1.0, np.max(np.abs(rows[v])))
    finally:
        e.close()


@pytest.mark.parametrize("variant,preset,plan", [("main_2", "reference", False), ("main", "bench", True)])
def test_driver_on_wrapped_inputs_matches_the_circuit_oracle(fa, variant, preset, plan):
    """the driver (forward_encrypted) fed by unwrapped inputs against the clear-text circuit (oracle/circuit_sim.py), with
    tests/test_forward_gpu.py's per-stage tolerances and LOGIT_TOL and the same class: at the reference ring, and at the headline ring
    under a level plan recorded with the REGULAR ingest and applied to the wrapped one (every unwrapped input at its planned limbs)"""
    from fhe_linformer_amd import linformer as lf
    from oracle import plain_forward as pf, circuit_sim as cs
    LOGIT_TOL = 1.2e-2
    tol = {"scores": 5e-8, "exp": 5e-8, "self_attention": 5e-8, "affine1_0": 5e-8, "encoder_out": 1e-4, "pooled": 5e-3}
    S = 129
    w = pf.synthetic_model(1234)
    eng = fa.Engine(preset, seed=11, n_q=28, n_p=-1)
    try:
        eng.keygen()
        eng.gen_relin_key()
        eng.gen_rotation_keys(fa.circuit_rotation_indices())
        eng.bootstrap_setup(3, 3, 16384)
        ctl = lf.GpuController(eng)
        targets = None
        if plan:
            x0 = pf.synthetic_tokens(S, 4320)
            eng.level_plan_begin("record")
            eng.decrypt(lf.forward_encrypted(ctl, w, lf.ingest_sample(ctl, w, x0), None, variant))
            targets = eng.level_plan_end()
            assert 0 < min(t for t in targets[:194] if t > 0) < max(targets[:194]) <= eng.n_q   # the F inputs start far lower
            eng.level_plan_begin("apply")
        x = pf.synthetic_tokens(S, 4321)
        enc = lf.ingest_sample(ctl, w, x, wrapped=True)
        flat = enc["inputs_E"] + enc["inputs_F"] + enc["inputs"]
        if plan:
            assert [c.info()["ell"] for c in flat] == [t if t > 0 else eng.n_q for t in targets[:194]]
        tr = {}
        out = lf.forward_encrypted(ctl, w, enc, tr, variant)
        errs = {}
        lg = lf.logits_from_slots(eng.decrypt(out))
        if plan:
            eng.level_plan_end()
        st = {}
        ref = lf.forward(cs.SlotSimController(), w, *pf.client_inputs(w, x), st, variant)
        for k, t in tol.items():
            errs[k] = np.max(np.abs(eng.decrypt(tr[k]) - st[k]))
        errs["logits"] = np.max(np.abs(lg - lf.logits_from_slots(ref)))
        print(f"wrapped {variant} {preset} plan={plan}: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
        for k, t in tol.items():
            assert errs[k] < t, (k, errs[k])
        assert errs["logits"] < LOGIT_TOL
        assert int(np.argmax(lg)) == int(np.argmax(lf.logits_from_slots(ref)))
    finally:
        eng.close()


def test_batched_controller_wrapped_route(fa):
    """ingest_sample(BatchedController, wrapped=True): every sample's wrapped ciphertexts unwrapped in one call, the B samples'
    inputs as Batches in read order, each within the bound of the expanded row"""
    from fhe_linformer_amd import linformer as lf
    from oracle import plain_forward as pf
    e = _client(fa, "toy13", **TOY)
    try:
        w = pf.synthetic_model(1234)
        S = 6
        xs = [pf.synthetic_tokens(S, 50 + x) for x in range(2)]
        enc = lf.ingest_sample(lf.BatchedController(e, 2), w, xs, wrapped=True)
        assert [len(enc[k]) for k in ("inputs_E", "inputs_F", "inputs")] == [32, 32, S + 1]
        for x in range(2):
            x_in, X_E, X_F = pf.client_inputs(w, xs[x])
            for k, i, row in (("inputs_E", 3, X_E[3]), ("inputs_F", 31, X_F[31]), ("inputs", 0, x_in[0]), ("inputs", S, x_in[S])):
                ct = enc[k][i][x]
                assert ct.info()["ell"] == e.n_q
                assert np.max(np.abs(e.decrypt(ct, 16384) - _expanded(row))) < 1e-8 * max(1.0, np.max(np.abs(row)))
    finally:
        e.close()
