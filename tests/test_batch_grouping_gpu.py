"""The grouping loop of the batched leaf operations (evaluator.cpp for_groups): a list of INTERLEAVED, MIXED shapes that is longer than
the batch limit.

Every batched leaf operation picks the first operand not yet done as the leader of a group, collects the later operands of the leader's
shape up to the batch limit, runs one launch set and scatters the results back to their places.  Here the limit is 2 (FHELIN_BATCH=2)
and the list is  A, B, A, A', B, A, C:
  A   5 limbs, degree 1, the level's scale
  A'  A's shape with the scale times (1 + 1e-12): within the 1e-9 of "the same shape", so it rides in A's groups - with its OWN scale
  B   3 limbs
  C   A's shape with the scale times (1 + 1e-6): a group of its own
so A's group has to split, the second chunk is led by A', and B's group lies between the members of A's.  Every output, in input order,
must equal the same operation applied to that element alone: residues (export), info() and the 80-bit scale (scale_parts), bit for bit -
all of them exact integer functions, row by row independent of what else shares the launch.

What this file pins is the grouping and the scatter back to input order.  The references of rotate_sum and hoisted_dot are the same
functions over a list of one, so the merged rotation-sum stage itself (Evaluator::rotation_sum) is NOT checked here: that is
test_default_path_gpu.py and test_rotation_gather_gpu.py, against the oracle."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
LD = np.longdouble

ELLS = [5, 3, 5, 5, 3, 5, 5]                               # A, B, A, A', B, A, C
FACTOR = [1.0, 1.0, 1.0, 1.0 + 1e-12, 1.0, 1.0, 1.0 + 1e-6]
ROT = [1, 2, 3]


def _residues(orc, eng, seed, ell):
    return np.stack([orc.uniform_residues(seed + 1000 * p, eng.q[:ell], eng.N) for p in range(2)])


def _uniform_key(orc, eng, seed):
    d = eng.dnum_digits
    k = np.stack([orc.uniform_residues(seed + 50 * j, eng.moduli, eng.N) for j in range(2 * d)])
    return k.reshape(d, 2, eng.n_limbs, eng.N)


@pytest.fixture(scope="module")
def eng(fa, orc):
    """preset toy (N = 2^12, 6 + 2 limbs) with a batch limit of 2 (read when the context is created); uniform residues as keys"""
    old = os.environ.get("FHELIN_BATCH")
    os.environ["FHELIN_BATCH"] = "2"
    try:
        e = fa.Engine("toy", device=0, seed=1)
    finally:
        if old is None:
            os.environ.pop("FHELIN_BATCH", None)
        else:
            os.environ["FHELIN_BATCH"] = old
    for r in ROT:
        e.key_import(1, r, _uniform_key(orc, e, 9000 + 17 * r))
    e.key_import(0, 0, _uniform_key(orc, e, 31))
    yield e
    e.close()


def _level_scale(eng, ell):
    return float(eng.scaling_factors[eng.n_q - ell])


def _mixed(orc, eng, seed, deg=1, ells=ELLS, factor=FACTOR):
    """the common list: every element its own residues, so a result scattered to the wrong place shows"""
    out = []
    for i, (ell, f) in enumerate(zip(ells, factor)):
        sc = _level_scale(eng, ell)
        if deg == 2:
            sc = float(LD(sc) * LD(sc))
        out.append(eng.ct_import(_residues(orc, eng, seed + 13 * i, ell), deg=deg, scale=sc * f))
    return out


def _same(got, want, what):
    assert len(got) == len(want), what
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.info() == w.info(), (what, i, g.info(), w.info())
        assert g.scale_parts() == w.scale_parts(), (what, i, "80-bit scale")
        assert g.export().tobytes() == w.export().tobytes(), (what, i)


def test_the_list_is_what_the_cases_assume(eng, orc):
    """A' and C differ from A in their scales by what the grouping's 1e-9 lets through and by what it does not"""
    L = _mixed(orc, eng, 100)
    s = [LD(c.scale_parts()[0]) + LD(c.scale_parts()[1]) for c in L]
    assert s[0] == s[2] == s[5] and s[3] != s[0] and s[6] != s[0]
    assert abs(s[3] / s[0] - 1) < LD(1e-9) < abs(s[6] / s[0] - 1)
    assert [c.info()["ell"] for c in L] == ELLS


def test_the_batch_limit_of_two_is_in_force(eng, orc):
    """the outputs of one group are views of ONE device block, which the pool takes back when the last of them goes.  With a limit of 2
    the groups of rotate_batch are (0, 2), (1, 4), (3, 5), (6): dropping output 0 frees nothing, dropping output 2 as well frees their
    block; likewise 3 and 5.  With a larger limit 0, 2, 3, 5 would share one block and dropping 0 and 2 would free nothing"""
    L = _mixed(orc, eng, 150)
    outs = eng.rotate_batch(L, 1)
    eng.sync()
    live = lambda: eng.cache_stats()["pool_live_bytes"]
    ct_bytes = 2 * 5 * eng.N * 8
    b = live()
    for first, second in ((0, 2), (3, 5)):
        outs[first].free()
        assert live() == b, ("output", first, "shares its block with output", second)
        outs[second].free()
        assert live() == b - 2 * ct_bytes, ("outputs", first, second, "are one group of two")
        b = live()


def test_rotate_batch(eng, orc):
    L = _mixed(orc, eng, 200)
    _same(eng.rotate_batch(L, 1), [eng.rotate(x, 1) for x in L], "rotate_batch")


def test_rotate_each(eng, orc):
    """the zero index takes the copy path; operands with a zero index join no group"""
    L = _mixed(orc, eng, 300)
    idx = [1, 2, 0, 1, 3, 2, 1]
    _same(eng.rotate_each(L, idx), [eng.rotate(x, r) for x, r in zip(L, idx)], "rotate_each")


def test_rotate_sum(eng, orc):
    L = _mixed(orc, eng, 400)
    _same(eng.rotate_sum(L, ROT), [eng.rotate_sum([x], ROT)[0] for x in L], "rotate_sum")


@pytest.mark.parametrize("rescale", [False, True])
def test_hoisted_dot(eng, orc, rescale):
    L = _mixed(orc, eng, 500)
    rng = np.random.default_rng(77)
    ns = 1 << eng.params.log_slots
    pts = [eng.encode(rng.uniform(-1, 1, ns)) for _ in range(3)]
    want = [eng.hoisted_dot([x], pts, [1, 2], rescale=rescale)[0] for x in L]
    _same(eng.hoisted_dot(L, pts, [1, 2], rescale=rescale), want, ("hoisted_dot", rescale))


def test_rescale_batch(eng, orc):
    """degree-2 operands of the same limb pattern: five of 5 limbs leave a group of one behind"""
    L = _mixed(orc, eng, 600, deg=2)
    _same(eng.rescale_batch(L), [eng.rescale(x) for x in L], "rescale_batch")


def _pairs(orc, eng):
    """the list against partners whose limbs differ across the list: the products have 5, 3, 3, 4, 3, 5, 5 limbs"""
    a = _mixed(orc, eng, 700)
    b = _mixed(orc, eng, 800, ells=[5, 5, 3, 4, 3, 5, 5], factor=[1.0] * 7)
    return a, b


def test_mult_batch(eng, orc):
    a, b = _pairs(orc, eng)
    _same(eng.mult_batch(a, b), [eng.mult(x, y) for x, y in zip(a, b)], "mult_batch")


def test_mult_affine_batch(eng, orc):
    """both factors, constants, and addends on some items: a degree-1 addend shared by two items of one group (adjusted once), one at its
    product's limbs, one with more limbs than its product (subtracted), one of degree 2 taken as it stands; none below its product, which
    would send the whole call through the unmerged sequence"""
    a, b = _pairs(orc, eng)
    s5 = _level_scale(eng, 5)
    t = eng.ct_import(_residues(orc, eng, 901, 5))
    u = eng.ct_import(_residues(orc, eng, 902, 3))
    v = eng.ct_import(_residues(orc, eng, 903, 5))
    w = eng.ct_import(_residues(orc, eng, 904, 5), deg=2, scale=float(LD(s5) * LD(s5)))
    f = [1, 2, 2, 1, 2, 1, 2]
    cadd = [0.0, -1.0, 0.0, 0.5, -1.0, 0.0, 0.0]
    addend = [t, u, v, None, None, t, w]
    negate = [False, False, True, False, False, True, False]
    want = [eng.mult_affine_batch([a[i]], [b[i]], [f[i]], [cadd[i]], [addend[i]], [negate[i]])[0] for i in range(7)]
    _same(eng.mult_affine_batch(a, b, f, cadd, addend, negate), want, "mult_affine_batch")


def test_rotate_each_sum_of_mixed_shapes(eng, orc):
    """terms of different shapes fall back to separate rotations, added in the fallback's order: the unrotated terms first, then the
    rotated ones"""
    L = _mixed(orc, eng, 1000)
    idx = [1, 2, 0, 1, 3, 2, 1]
    acc = L[2]
    for i in (0, 1, 3, 4, 5, 6):
        acc = eng.add(acc, eng.rotate(L[i], idx[i]))
    _same([eng.rotate_each_sum(L, idx)], [acc], "rotate_each_sum")
