"""Addressing of the NTT tile passes (kernels_ntt.hip): every global access is a workgroup-uniform 64-bit base, a 32-bit lane offset
and a constant.  What can go wrong there is an offset, not a butterfly, so these are the smallest shapes that reach every way an address
is formed, each compared bit for bit with the oracle:
  * every compiled tile split (log_n 12 ... 17; 12 has one tile per vector, 13 is the first with a tile index), forward and inverse, on
    the 55-bit first prime, the 52-bit scaling primes (lazy path) and the 60-bit special primes (semi-lazy path);
  * vector counts 1, 7, 8 and 24 at one tile per vector, so the row pass's XCD remap (grid a multiple of 8) is off and on, with its
    period split (count a multiple of the limb count, and larger) active and inactive;
  * key switching, whose transforms use a limb table with a repeat length and skipped (negative) entries, strided first-pass sources
    with one and with two levels of groups, and the row-pass epilogue: identity map and inverse automorphism map, one map and one map
    per row, with and without the addends and the post addend, results of one and of several limbs, rows behind the first;
  * the rescale, whose column pass lifts its input while loading it;
  * a batch whose last vector starts past byte offset 2^32: the vector offset has to stay in the 64-bit base."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROTS = [1, 3, 128]


def _ring(engine_factory, log_n):
    """preset toy13 (7 + 3 limbs) at another ring size"""
    return engine_factory("toy13", log_n=log_n, log_slots=log_n - 1)


@pytest.mark.parametrize("log_n", [12, 13, 14, 15, 16, 17])
def test_every_tile_split(engine_factory, orc, log_n):
    """two polynomials over Q (first prime + scaling primes) and over P, forward, inverse and back"""
    eng = _ring(engine_factory, log_n)
    assert eng.log_n == log_n
    for mods, psis, first, seed in ((eng.q, eng.psi_q, 0, 11), (eng.p, eng.psi_p, eng.n_q, 12)):
        x = np.stack([orc.uniform_residues(seed + 100 * p, mods, eng.N) for p in range(2)])
        nvec = x.shape[0] * x.shape[1]
        buf = eng.upload(x)
        eng.ntt(buf, nvec, limb_first=first, limb_count=len(mods))
        fwd = buf.download(x.shape)
        assert np.array_equal(fwd, orc.ntt_batch(x, mods, psis)), (log_n, first, "forward")
        eng.ntt(buf, nvec, limb_first=first, limb_count=len(mods), inverse=True)
        assert np.array_equal(buf.download(x.shape), x), (log_n, first, "inverse of forward")
        buf.upload(x)
        eng.ntt(buf, nvec, limb_first=first, limb_count=len(mods), inverse=True)
        assert np.array_equal(buf.download(x.shape), orc.ntt_batch(x, mods, psis, inverse=True)), (log_n, first, "inverse")
        buf.free()


@pytest.mark.parametrize("log_n", [12, 13])
@pytest.mark.parametrize("nvec", [1, 7, 8, 24])
@pytest.mark.parametrize("count", [1, 4, 6])
def test_vector_counts(engine_factory, orc, log_n, nvec, count):
    """vector v uses limb first + v % count.  At log_n 12 the grid is the vector count: 8 and 24 take the XCD remap, 1 and 7 do not;
    the period split is on where count divides nvec and is smaller (8 and 24 with 1 and 4, 24 with 6, 7 with 1)"""
    eng = _ring(engine_factory, log_n)
    first = 1
    mods = [eng.moduli[first + v % count] for v in range(nvec)]
    x = orc.uniform_residues(1000 * nvec + count, mods, eng.N)
    q, psi = eng.moduli[first:first + count], eng.roots[first:first + count]
    for inverse in (False, True):
        buf = eng.upload(x)
        eng.ntt(buf, nvec, limb_first=first, limb_count=count, inverse=inverse)
        assert np.array_equal(buf.download(x.shape), orc.ntt_batch(x, q, psi, inverse=inverse)), (nvec, count, inverse)
        buf.free()


def test_base_past_4gib(engine_factory, orc):
    """8193 vectors at N = 2^16: the last one starts at byte 2^32.  Only the first and the last vector are set and compared; the
    others are transformed as they lie in memory"""
    eng = engine_factory("bench")
    nvec, limb = 8193, 1
    vec_bytes = eng.N * 8
    x = orc.uniform_residues(4242, [eng.q[limb]] * 2, eng.N)
    want = orc.ntt_batch(x, eng.q[limb:limb + 1], eng.psi_q[limb:limb + 1])
    buf = eng.buf(nvec * vec_bytes)
    last = C.c_void_p(buf.ptr.value + (nvec - 1) * vec_bytes)
    assert (nvec - 1) * vec_bytes == 1 << 32
    try:
        for dst, row in ((buf.ptr, x[0]), (last, x[1])):
            eng._ck(eng.lib.fhelin_dev_upload(eng.h, dst, np.ascontiguousarray(row).ctypes.data_as(C.c_void_p), vec_bytes))
        eng.ntt(buf, nvec, limb_first=limb, limb_count=1)
        got = np.empty_like(x)
        for src, row in ((buf.ptr, got[0]), (last, got[1])):
            eng._ck(eng.lib.fhelin_dev_download(eng.h, row.ctypes.data_as(C.c_void_p), src, vec_bytes))
        assert np.array_equal(got[0], want[0]), "first vector"
        assert np.array_equal(got[1], want[1]), "vector at byte offset 2^32"
    finally:
        buf.free()


# ---- transforms inside key switching and rescaling -------------------------------------------------------------------------------
def _ct(orc, eng, seed, ell):
    return np.stack([orc.uniform_residues(seed + 1000 * p, eng.q[:ell], eng.N) for p in range(2)])


def _evk(orc, eng, seed):
    d = eng.dnum_digits
    k = np.stack([orc.uniform_residues(seed + 50 * j, eng.moduli, eng.N) for j in range(2 * d)])
    return k.reshape(d, 2, eng.n_limbs, eng.N)


def _engine(fa, env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return fa.Engine("toy13", device=0)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.fixture(scope="module")
def engines(fa, orc):
    """the default (rotations gathered, identity-map epilogue), rotations written through the inverse automorphism map by the
    epilogue, and the separate finishing kernels; the same uniform keys everywhere"""
    es = {"default": _engine(fa, {"FHELIN_FUSE_FINISH": "1", "FHELIN_FUSE_MODDOWN": "0"}),
          "map": _engine(fa, {"FHELIN_FUSE_FINISH": "1", "FHELIN_FUSE_MODDOWN": "1"}),
          "separate": _engine(fa, {"FHELIN_FUSE_FINISH": "0", "FHELIN_FUSE_MODDOWN": "0"})}
    e0 = es["default"]
    relin = _evk(orc, e0, 4242)
    rots = {r: _evk(orc, e0, 7100 + 17 * r) for r in ROTS}
    for e in es.values():
        e.key_import(0, 0, relin)
        for r, k in rots.items():
            e.key_import(1, r, k)
    yield es, relin, rots
    for e in es.values():
        e.close()


def _orc_rotate(orc, e, x, key, r):
    return orc.rotate(x, key, orc.galois(e.log_n, r), e.alpha, e.q, e.p, e.psi_q, e.psi_p)


@pytest.mark.parametrize("ell", [7, 3, 2])
def test_rotations(engines, orc, ell):
    """one rotation, a batch of rows (strided ModUp source, rows behind the first), hoisted rotations of one input and rotations of
    several inputs by their own amounts (one key and one map per row)"""
    es, _, rots = engines
    e0 = es["default"]
    xs = [_ct(orc, e0, 300 + 7 * i + ell, ell) for i in range(3)]
    want_row = [_orc_rotate(orc, e0, x, rots[3], 3) for x in xs]
    want_many = [_orc_rotate(orc, e0, xs[0], rots[r], r) for r in ROTS]
    want_each = [_orc_rotate(orc, e0, x, rots[r], r) for x, r in zip(xs, ROTS)]
    for name in ("default", "map"):
        e = es[name]
        assert np.array_equal(e.raw_rotate(e.ct_import(xs[0]), 3).export(), want_row[0]), (name, ell)
        for g, w in zip(e.rotate_batch([e.ct_import(x) for x in xs], 3), want_row):
            assert np.array_equal(g.export(), w), (name, ell, "rotate_batch")
        for g, w in zip(e.rotate_many(e.ct_import(xs[0]), ROTS), want_many):
            assert np.array_equal(g.export(), w), (name, ell, "rotate_many")
        for g, w in zip(e.rotate_each([e.ct_import(x) for x in xs], ROTS), want_each):
            assert np.array_equal(g.export(), w), (name, ell, "rotate_each")


@pytest.mark.parametrize("ell", [7, 2])
def test_rotation_sums(engines, orc, ell):
    """merged sums: one ModUp and one ModDown for several rotations of a row, and own ModUps (two levels of source groups once the
    rows of a batch lie apart) under one ModDown"""
    es, _, rots = engines
    e0 = es["default"]
    gs = [orc.galois(e0.log_n, r) for r in ROTS]
    evks = np.stack([rots[r] for r in ROTS])
    xs = [_ct(orc, e0, 900 + 7 * i + ell, ell) for i in range(3)]
    want_sum = [orc.rotate_sum(x, evks, gs, e0.alpha, e0.q, e0.p, e0.psi_q, e0.psi_p) for x in xs]
    want_each = orc.rotate_each_sum(np.stack(xs), evks, gs, e0.alpha, e0.q, e0.p, e0.psi_q, e0.psi_p)
    for name in ("default", "map"):
        e = es[name]
        for g, w in zip(e.rotate_sum([e.ct_import(x) for x in xs], ROTS), want_sum):
            assert np.array_equal(g.export(), w), (name, ell, "rotate_sum")
        got = e.rotate_each_sum([e.ct_import(x) for x in xs], ROTS).export()
        assert np.array_equal(got, want_each), (name, ell, "rotate_each_sum")


@pytest.mark.parametrize("ell", [7, 3, 2])
def test_rescale_lift_and_epilogue(engines, orc, ell):
    """the lifting column pass and the rescale epilogue; from 2 limbs the result has one"""
    es, _, _ = engines
    e0 = es["default"]
    xs = [_ct(orc, e0, 100 + 7 * i + ell, ell) for i in range(3)]
    want = [orc.rescale(x, e0.q[:ell], e0.psi_q[:ell]) for x in xs]
    for name in ("default", "separate"):
        e = es[name]
        assert np.array_equal(e.raw_rescale(e.ct_import(xs[0])).export(), want[0]), (name, ell)
        for g, w in zip(e.rescale_batch([e.ct_import(x) for x in xs]), want):
            assert np.array_equal(g.export(), w), (name, ell, "rescale_batch")


@pytest.mark.parametrize("ell", [7, 3, 2])
def test_relinearisation_epilogue(engines, orc, ell):
    """identity map with both addends, alone and as a batch"""
    es, relin, _ = engines
    e0 = es["default"]
    a = [_ct(orc, e0, 500 + 7 * i + ell, ell) for i in range(3)]
    b = [_ct(orc, e0, 600 + 7 * i + ell, ell) for i in range(3)]
    want = orc.mult_relin(a[0], b[0], relin, e0.alpha, e0.q, e0.p, e0.psi_q, e0.psi_p)
    got = {}
    for name in ("default", "separate"):
        e = es[name]
        assert np.array_equal(e.raw_mult_relin(e.ct_import(a[0]), e.ct_import(b[0])).export(), want), (name, ell)
        got[name] = [c.export() for c in e.mult_batch([e.ct_import(x) for x in a], [e.ct_import(y) for y in b])]
    for f, s in zip(got["default"], got["separate"]):
        assert f.shape == s.shape and f.tobytes() == s.tobytes(), ell


@pytest.mark.parametrize("ell", [7, 2])
def test_moddown_rescale_epilogue(engines, orc, ell):
    """merged ModDown + rescale of a hoisted dot product (strided single-limb source, (K+1)-entry limb table): the fused row pass
    against the separate finishing kernels, whose oracle comparison is test_default_path_gpu.py's"""
    es, _, _ = engines
    rng = np.random.default_rng(ell)
    ns = 1 << es["default"].params.log_slots
    vals = [rng.uniform(-1, 1, ns) for _ in range(len(ROTS) + 1)]
    xs = [_ct(orc, es["default"], 800 + 7 * i + ell, ell) for i in range(3)]
    got = {}
    for name in ("default", "separate"):
        e = es[name]
        pts = [e.encode(v) for v in vals]
        got[name] = [c.export() for c in e.hoisted_dot([e.ct_import(x) for x in xs], pts, ROTS, rescale=True)]
    for f, s in zip(got["default"], got["separate"]):
        assert f.shape == s.shape and f.shape[1] == ell - 1 and f.tobytes() == s.tobytes(), ell
