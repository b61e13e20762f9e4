"""Interleaved samples through the composites (include/fhelin.h "Interleaved samples"): lane independence by decryption.  Two samples
drawn from different seeds share every ciphertext of an engine with stride 2 (N = 2^16, 16384 logical slots: the 32768 physical
slots are the ring's full packing); each composite runs ONCE on the interleaved inputs and every lane must match oracle/slotsim.py
on that lane's own inputs, within the tolerance the same assertion carries in tests/test_composites_gpu.py (TOL = 1e-5; the
Chebyshev series: tests/test_polyeval_gpu.py, 1e-5; the ciphertext product: tests/test_scheme_gpu.py, 1e-7; the ingestion:
tests/test_client_gpu.py).  The two lanes' expected outputs are first shown to differ by far more than the tolerance, so a lane
swap or a leak between lanes cannot pass."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TOL = 1e-5
S = 2


@pytest.fixture(scope="module")
def eng(fa):
    e = fa.Engine("bench", seed=99, n_q=8, n_p=2, dnum=4, interleave=S)
    e.keygen()
    e.gen_relin_key()
    e.gen_rotation_keys(fa.circuit_rotation_indices())
    yield e
    e.close()


@pytest.fixture(scope="module")
def sim():
    from oracle import slotsim
    return slotsim


def _v(seed, lane, n=16384, lo=-1, hi=1):
    """the vector of `seed` for sample `lane`: different seeds per lane"""
    return np.random.default_rng(seed + 100003 * lane).uniform(lo, hi, n)


def _pair(seed, **kw):
    return [_v(seed, i, **kw) for i in range(S)]


def _enc(eng, xs, level=0):
    return eng.encrypt_interleaved_batch(np.stack(xs)[None], level)[0]


def _close(eng, ct, wants, tol=TOL):
    """every lane against its own expectation; the expectations differ by far more than the tolerance"""
    wants = [np.asarray(w) for w in wants]
    assert np.max(np.abs(wants[0] - wants[1])) > 1000 * tol
    got = eng.decrypt_interleaved(ct)
    assert got.shape == (S, 16384)
    for i in range(S):
        err = np.max(np.abs(got[i] - wants[i]))
        assert err < tol, (i, err)


def test_rotsum_repeat_masks(eng, sim):
    xs = _pair(1)
    c = _enc(eng, xs)
    L = lambda f: [f(x) for x in xs]
    _close(eng, eng.rotsum(c, 128, 128), L(lambda x: sim.rotsum(x, 128, 128)))
    _close(eng, eng.rotsum(c, 128, 1), L(lambda x: sim.rotsum(x, 128, 1)))
    _close(eng, eng.rotsum(c, 32, 128), L(lambda x: sim.rotsum(x, 32, 128)))
    _close(eng, eng.repeat(c, 128), L(lambda x: sim.repeat(x, 128)))
    _close(eng, eng.repeat(c, 128, -128), L(lambda x: sim.repeat(x, 128, -128)))
    _close(eng, eng.mask_block(c, 256, 384, 0.5), L(lambda x: sim.mask_block(x, 256, 384, 0.5)))
    _close(eng, eng.mask_heads(c, 2.0), L(lambda x: sim.mask_mod_n(x, 64, 0, 2.0)))
    _close(eng, eng.mask_heads_128(c, 1 / 64), L(lambda x: sim.mask_mod_n(x, 128, 0, 1 / 64)), )
    _close(eng, eng.mask_mod_n(c, 128, 64), L(lambda x: sim.mask_mod_n(x, 128, 64)))
    _close(eng, eng.mask_first_n(c, 128, 3.0), L(lambda x: sim.mask_first_n(x, 128, 3.0)))
    _close(eng, eng.mult_const(c, -0.25), L(lambda x: -0.25 * x))


def test_matmulRE_and_CR(eng, sim):
    rng = np.random.default_rng(2)
    W = rng.uniform(-1, 1, (128, 128)) / 8
    b = rng.uniform(-1, 1, 128)
    xs = [[np.random.default_rng(20 + 10 * i + k).uniform(-1, 1, 128) for i in range(S)] for k in range(2)]     # [row][lane]
    rows = [_enc(eng, [np.repeat(x, 128) for x in lanes]) for lanes in xs]
    w_pt, b_pt = eng.encode(W.reshape(-1)), eng.encode(np.tile(b, 128))                 # the model is the same for every lane
    outs = eng.matmulRE(rows, w_pt, b_pt)
    for lanes, o in zip(xs, outs):
        _close(eng, o, [np.tile(x @ W + b, 128) for x in lanes])
    per_lane = [sim.matmul([np.repeat(xs[k][i], 128) for k in range(2)], W.reshape(-1), np.tile(b, 128), 128, 128) for i in range(S)]
    for k, o in enumerate(outs):
        _close(eng, o, [per_lane[i][k] for i in range(S)])
    ys = [np.random.default_rng(30 + i).uniform(-1, 1, 128) for i in range(S)]
    row = _enc(eng, [np.tile(y, 128) for y in ys])
    got = eng.decrypt_interleaved(eng.matmulCR([row], eng.encode(W.reshape(-1)), eng.encode(np.repeat(b, 128)))[0])
    assert np.max(np.abs((W @ ys[0] + b) - (W @ ys[1] + b))) > 1000 * TOL
    for i in range(S):
        assert np.max(np.abs(got[i][::128] - (W @ ys[i] + b))) < TOL
    cw = _enc(eng, [W.reshape(-1)] * S)                                                   # ciphertext weights
    _close(eng, eng.matmulCR([row], cw)[0], [sim.rotsum(np.tile(y, 128) * W.reshape(-1), 64, 1) for y in ys])
    _close(eng, eng.matmulCR_128([row], cw)[0], [sim.rotsum(np.tile(y, 128) * W.reshape(-1), 128, 1) for y in ys])


def test_matmul_large_variants(eng, sim):
    rng = np.random.default_rng(4)
    ws = [rng.uniform(-1, 1, 16384) / 8 for _ in range(4)]
    bias = rng.uniform(-1, 1, 16384)
    xs = [_pair(40 + k) for k in range(2)]                                               # [row][lane]
    rows = [_enc(eng, lanes) for lanes in xs]
    wp = [eng.encode(w) for w in ws]
    outs = eng.matmulRElarge(rows, wp, eng.encode(bias), 0.5)
    sims = [sim.matmulRElarge([xs[k][i] for k in range(2)], ws, bias, 0.5) for i in range(S)]
    for k, o in enumerate(outs):
        _close(eng, o, [sims[i][k] for i in range(S)])
    blocks = [[_pair(50 + 4 * r + j) for j in range(4)] for r in range(2)]               # [row][block][lane]
    cts = [[_enc(eng, lanes) for lanes in r] for r in blocks]
    outs = eng.matmulCRlarge(cts, wp, eng.encode(bias))
    sims = [sim.matmulCRlarge([[blocks[r][j][i] for j in range(4)] for r in range(2)], ws, bias) for i in range(S)]
    for k, o in enumerate(outs):
        _close(eng, o, [sims[i][k] for i in range(S)])


def test_matmulScores(eng, sim):
    keys = _pair(60)
    qs = [_pair(61 + k) for k in range(3)]
    ck = _enc(eng, keys)
    cq = [_enc(eng, lanes) for lanes in qs]
    _close(eng, eng.matmulScores(cq, ck), [sim.matmulScores([qs[k][i] for k in range(3)], keys[i]) for i in range(S)])


def test_wrap_unwrap(eng, sim):
    vs = [_pair(70 + k) for k in range(3)]
    cs = [_enc(eng, lanes) for lanes in vs]
    lane = lambda i: [vs[k][i] for k in range(3)]
    _close(eng, eng.wrapUpRepeated(cs), [sim.wrapUpRepeated(lane(i)) for i in range(S)])
    w = eng.wrapUpExpanded(cs)
    ws = [sim.wrapUpExpanded(lane(i)) for i in range(S)]
    _close(eng, w, ws)
    un = [sim.unwrapExpanded(ws[i], 3) for i in range(S)]
    for k, o in enumerate(eng.unwrapExpanded(w, 3)):
        _close(eng, o, [un[i][k] for i in range(S)])
    un = [sim.unwrapScoresExpanded(ws[i], 2) for i in range(S)]
    for k, o in enumerate(eng.unwrapScoresExpanded(w, 2)):
        _close(eng, o, [un[i][k] for i in range(S)])
    un = [sim.unwrap_512_in_4_128(vs[0][i], 1) for i in range(S)]
    for k, o in enumerate(eng.unwrap_512_in_4_128(cs[0], 1)):
        _close(eng, o, [un[i][k] for i in range(S)])
    _close(eng, eng.add_many(cs), [sum(lane(i)) for i in range(S)])


def test_containers(eng, sim):
    n = 34                                                                               # two containers (32 + 2): the ragged case
    vs = [[sim.mask_block(_v(80 + k, i), 0, 512) for i in range(S)] for k in range(n)]  # [input][lane]
    cs = eng.encrypt_interleaved_batch(np.stack([np.stack(lanes) for lanes in vs]), level=4)
    bias = np.random.default_rng(200).uniform(-1, 1, 16384)
    conts = eng.generate_containers(cs, eng.encode(bias))
    sims = [sim.generate_containers([vs[k][i] for k in range(n)], bias) for i in range(S)]
    assert len(conts) == len(sims[0]) == 2
    for k, o in enumerate(conts):
        _close(eng, o, [sims[i][k] for i in range(S)])
    un = eng.unwrapRepeatedLarge(conts, n)
    us = [sim.unwrapRepeatedLarge(sims[i], n) for i in range(S)]
    assert len(un) == n
    for j in (0, 31, 33):
        for k, o in enumerate(un[j]):
            _close(eng, o, [us[i][j][k] for i in range(S)])
    _close(eng, eng.wrap_containers(cs[:3], 3), [sim.wrap_containers([vs[k][i] for k in range(3)], 3) for i in range(S)])


def test_chebyshev_and_ciphertext_product(eng):
    from numpy.polynomial import chebyshev as Ch
    rng = np.random.default_rng(31)
    c = rng.uniform(-1, 1, 32) / np.arange(1, 33)                                        # degree 31 (tests/test_polyeval_gpu.py)
    cc = c.copy()
    cc[0] *= 0.5
    xs = _pair(3)
    ct = _enc(eng, xs)
    _close(eng, eng.eval_chebyshev(ct, c), [Ch.chebval(x, cc) for x in xs], 1e-5)
    ys = _pair(4)
    _close(eng, eng.mult(ct, _enc(eng, ys)), [x * y for x, y in zip(xs, ys)], 1e-7)


def test_client_ingest_interleaved(fa):
    """fhelin_client_ingest_interleaved for S = 129, two samples: x_in and the projections of each sample are fhelin_client_ingest's
    on a stride-1 engine BIT FOR BIT, and each lane of each of the 194 decrypted inputs is that sample's expanded row to encoder
    precision (1e-9: tests/test_client_gpu.py)."""
    from oracle import plain_forward as pf
    from fhe_linformer_amd import linformer as lf
    w = pf.synthetic_model(1234)
    T = 129
    xs = [pf.synthetic_tokens(T, 4321 + 17 * i) for i in range(S)]
    arg = (w["cls_token"], w["posEmb"], w["E_w"], w["E_b"], w["F_w"], w["F_b"])
    one = fa.Engine("bench", seed=5, n_q=4, n_p=2, dnum=2)
    try:
        one.keygen()
        ref = [one.client_ingest(*arg, emb=x, level=1, want_proj=True) for x in xs]
        ref = [(r["x_in"].copy(), r["proj"].copy()) for r in ref]
    finally:
        one.close()
    eng = fa.Engine("bench", seed=5, n_q=4, n_p=2, dnum=2, interleave=S)
    try:
        eng.keygen()
        got = eng.client_ingest_interleaved(*arg, embs=xs, level=1, want_proj=True)
        for i in range(S):
            assert np.array_equal(got["x_in"][i], ref[i][0]) and np.array_equal(got["proj"][i], ref[i][1]), i
        assert not np.array_equal(ref[0][1], ref[1][1])
        assert len(got["inputs_E"]) == len(got["inputs_F"]) == 32 and len(got["inputs"]) == T + 1
        cts = got["inputs_E"] + got["inputs_F"] + got["inputs"]
        assert len(cts) == 194
        for v, ct in enumerate(cts):
            inf = ct.info()
            assert inf["ell"] == 3 and inf["slots"] == 16384
            dec = eng.decrypt_interleaved(ct)
            for i in range(S):
                row = ref[i][1][v] if v < 64 else ref[i][0][v - 64]
                assert np.max(np.abs(dec[i] - lf.expanded(row))) < 1e-9, (v, i)
        # the NumPy statement itself (dimReduce.py:141-160) per sample, as tests/test_client_gpu.py states it
        for i in range(S):
            x_in, X_E, X_F = pf.client_inputs(w, xs[i])
            assert np.array_equal(got["x_in"][i], x_in)
            assert np.max(np.abs(got["proj"][i] - np.vstack([X_E, X_F]))) < 1e-13
        # token ids into a shared table give the same rows
        table = np.random.default_rng(2).normal(0, 0.3, (50, 128))
        toks = [np.random.default_rng(3 + i).integers(0, 50, T) for i in range(S)]
        a = eng.client_ingest_interleaved(*arg, tokens=toks, table=table, want_proj=True)
        b = eng.client_ingest_interleaved(*arg, embs=[table[t] for t in toks], want_proj=True)
        for i in range(S):
            assert np.array_equal(a["x_in"][i], b["x_in"][i]) and np.array_equal(a["proj"][i], b["proj"][i])
        with pytest.raises(fa.FhelinError):
            eng.client_ingest(*arg, emb=xs[0])                                            # one sample alone has no lane to go to
        with pytest.raises(fa.FhelinError):
            eng.client_ingest_interleaved(*arg, embs=xs[:1])                              # one sample per lane
    finally:
        eng.close()
