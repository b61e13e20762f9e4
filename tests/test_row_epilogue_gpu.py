"""Row-pass epilogues of the forward NTT (kernels.h NttEpilogue): the rescale, the merged ModDown + rescale and the ModDown
finished in registers by the transform's row pass must give the same bytes as the separate finishing kernels
(FHELIN_FUSE_FINISH=0) and as the oracle.  The rotation case (output through the inverse automorphism map) is opt-in
(FHELIN_FUSE_MODDOWN=1) and is compared the same way.  Levels 24, 12 and 2 of the bench chain cover the 55-bit first prime, the
scaling primes and the few-limb tail; batches of one and of several ciphertexts go through different launch shapes."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PRESET = "bench"
ELLS = [24, 12, 2]
ROTS = [1, 128]


def _ct(orc, eng, seed, ell, npoly=2):
    return np.stack([orc.uniform_residues(seed + 1000 * p, eng.q[:ell], eng.N) for p in range(npoly)])


def _evk(orc, eng, seed):
    d = eng.dnum_digits
    k = np.stack([orc.uniform_residues(seed + 50 * j, eng.moduli, eng.N) for j in range(2 * d)])
    return k.reshape(d, 2, eng.n_limbs, eng.N)


def _engine(fa, env):
    """a context created with the given knobs (they are read when the context is created)"""
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return fa.Engine(PRESET, device=0)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.fixture(scope="module")
def engines(fa, orc):
    """fused (default), separate kernels, fused rotations; every engine holds the same uniform keys"""
    es = {"fused": _engine(fa, {"FHELIN_FUSE_FINISH": "1", "FHELIN_FUSE_MODDOWN": "0"}),
          "separate": _engine(fa, {"FHELIN_FUSE_FINISH": "0", "FHELIN_FUSE_MODDOWN": "0"}),
          "fused_rot": _engine(fa, {"FHELIN_FUSE_FINISH": "1", "FHELIN_FUSE_MODDOWN": "1"})}
    e0 = es["fused"]
    relin = _evk(orc, e0, 4242)
    rots = {r: _evk(orc, e0, 7100 + 17 * r) for r in ROTS}
    for e in es.values():
        e.key_import(0, 0, relin)
        for r, k in rots.items():
            e.key_import(1, r, k)
    yield es, relin, rots
    for e in es.values():
        e.close()


def _bytes(cts):
    return [c.export() for c in cts]


@pytest.mark.parametrize("ell", ELLS)
def test_rescale_epilogue(engines, orc, ell):
    es, _, _ = engines
    e0 = es["fused"]
    xs = [_ct(orc, e0, 100 + 7 * i + ell, ell) for i in range(3)]
    want = [orc.rescale(x, e0.q[:ell], e0.psi_q[:ell]) for x in xs]
    for name in ("fused", "separate"):
        e = es[name]
        one = e.raw_rescale(e.ct_import(xs[0])).export()                        # batch 1 (Evaluator::raw_rescale)
        assert np.array_equal(one, want[0]), (name, ell)
        many = _bytes(e.rescale_batch([e.ct_import(x) for x in xs]))           # batch 3 (Evaluator::rescale_batch)
        for g, w in zip(many, want):
            assert np.array_equal(g, w), (name, ell)


@pytest.mark.parametrize("ell", ELLS)
def test_relin_moddown_epilogue(engines, orc, ell):
    """identity-map ModDown with both addends (relinearisation), alone and as a batch"""
    es, relin, _ = engines
    e0 = es["fused"]
    a = [_ct(orc, e0, 500 + 7 * i + ell, ell) for i in range(3)]
    b = [_ct(orc, e0, 600 + 7 * i + ell, ell) for i in range(3)]
    want = orc.mult_relin(a[0], b[0], relin, e0.alpha, e0.q, e0.p, e0.psi_q, e0.psi_p)
    got = {}
    for name in ("fused", "separate"):
        e = es[name]
        one = e.raw_mult_relin(e.ct_import(a[0]), e.ct_import(b[0])).export()
        assert np.array_equal(one, want), (name, ell)
        got[name] = _bytes(e.mult_batch([e.ct_import(x) for x in a], [e.ct_import(y) for y in b]))
    for g, s in zip(got["fused"], got["separate"]):
        assert g.dtype == s.dtype and g.shape == s.shape and g.tobytes() == s.tobytes(), ell


@pytest.mark.parametrize("ell", ELLS)
def test_moddown_rescale_epilogue(engines, orc, ell):
    """merged ModDown + rescale (hoisted_dot with rescale): the oracle comparison of this path is test_default_path_gpu.py's"""
    es, _, _ = engines
    rng = np.random.default_rng(ell)
    ns = 1 << es["fused"].params.log_slots
    vals = [rng.uniform(-1, 1, ns) for _ in range(len(ROTS) + 1)]
    xs = [_ct(orc, es["fused"], 800 + 7 * i + ell, ell) for i in range(3)]
    got = {}
    for name in ("fused", "separate"):
        e = es[name]
        pts = [e.encode(v) for v in vals]
        got[name] = (_bytes(e.hoisted_dot([e.ct_import(xs[0])], pts, ROTS, rescale=True)),
                     _bytes(e.hoisted_dot([e.ct_import(x) for x in xs], pts, ROTS, rescale=True)))
    for gf, gs in zip(got["fused"], got["separate"]):
        assert len(gf) == len(gs)
        for f, s in zip(gf, gs):
            assert f.shape == s.shape and f.shape[1] == ell - 1
            assert f.tobytes() == s.tobytes(), ell


@pytest.mark.parametrize("ell", ELLS)
def test_rotation_moddown_epilogue(engines, orc, ell):
    """permuted ModDown (rotation): the opt-in fused form against the default and the oracle, alone and as a batch"""
    es, _, rots = engines
    e0 = es["fused"]
    xs = [_ct(orc, e0, 300 + 7 * i + ell, ell) for i in range(3)]
    for r in ROTS:
        want = orc.rotate(xs[0], rots[r], orc.galois(e0.log_n, r), e0.alpha, e0.q, e0.p, e0.psi_q, e0.psi_p)
        got = {}
        for name in ("fused", "fused_rot"):
            e = es[name]
            one = e.raw_rotate(e.ct_import(xs[0]), r).export()
            assert np.array_equal(one, want), (name, r, ell)
            got[name] = _bytes(e.rotate_batch([e.ct_import(x) for x in xs], r))
        for f, s in zip(got["fused"], got["fused_rot"]):
            assert f.shape == s.shape and f.tobytes() == s.tobytes(), (r, ell)
