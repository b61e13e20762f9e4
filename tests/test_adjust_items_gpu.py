"""The integer products of a batched level adjustment in one launch (Evaluator::adjust_deg1_batch, ew_scalar_items_kernel).

fhelin_add_batch / fhelin_mult_batch bring the operand with more limbs of every pair down to its partner: integer multiply on the first
target + 1 limbs, one batched rescale.  The products of a group are written by ONE launch per 32 ciphertexts, each source read at its
own limb stride.  Whatever the group looks like, residues, limbs, degree and the 80-bit scale must equal
  - the same call with one launch per ciphertext (FHELIN_ADJUST_ITEMS=0),
  - fhelin_add / fhelin_mult pair by pair,
  - the oracle's restatement of the adjustment (oracle/residue_eval.py ResidueEvaluator.adjust via add / mult),
bit for bit: all four are the same exact integer function."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
LD = np.longdouble

# ring -> (preset, overrides): targets of 1, 2 and 11 limbs need a chain of 12 and more
RINGS = {"toy": ("toy", dict(n_q=14)), "toy13": ("toy13", {})}
_ENG = {}


def _engine(fa, ring, items):
    """a context created with FHELIN_ADJUST_ITEMS=items (read when the context is created)"""
    if (ring, items) not in _ENG:
        preset, over = RINGS[ring]
        old = os.environ.get("FHELIN_ADJUST_ITEMS")
        os.environ["FHELIN_ADJUST_ITEMS"] = items
        try:
            _ENG[(ring, items)] = fa.Engine(preset, device=0, seed=1, **over)
        finally:
            if old is None:
                os.environ.pop("FHELIN_ADJUST_ITEMS", None)
            else:
                os.environ["FHELIN_ADJUST_ITEMS"] = old
    return _ENG[(ring, items)]


@pytest.fixture(scope="module")
def rings(fa, orc):
    """per ring: the engine under test, the per-ciphertext engine, the oracle's evaluator; one uniform relinearisation key in all three"""
    from oracle.residue_eval import ResidueEvaluator
    made = {}

    def get(ring):
        if ring not in made:
            new, old = _engine(fa, ring, "1"), _engine(fa, ring, "0")
            d = new.dnum_digits
            relin = np.stack([orc.uniform_residues(4242 + 50 * j, new.moduli, new.N) for j in range(2 * d)]).reshape(d, 2, new.n_limbs, new.N)
            for e in (new, old):
                e.key_import(0, 0, relin)
            rev = ResidueEvaluator(new.q, new.p, new.psi_q, new.psi_p, new.alpha, new.log_n, {"relin": relin}, new.params.log_slots)
            made[ring] = (new, old, rev)
        return made[ring]
    yield get
    for e in _ENG.values():
        e.close()
    _ENG.clear()


class Operand:
    """one ciphertext in the three places it lives: both engines and the oracle"""

    def __init__(self, orc, new, old, rev, seed, ell, npoly=2, deg=1, scale=None):
        from oracle.residue_eval import RCt
        x = np.stack([orc.uniform_residues(seed + 1000 * p, new.q[:ell], new.N) for p in range(npoly)])
        sc = float(rev.sf[len(new.q) - ell]) if scale is None else float(scale)
        self.new, self.old = new.ct_import(x, deg=deg, scale=sc), old.ct_import(x, deg=deg, scale=sc)
        self.r = RCt(x, deg, LD(sc))


def _same(ct, r, what):
    inf = ct.info()
    assert (inf["npoly"], inf["ell"], inf["deg"]) == (r.npoly, r.ell, r.deg), (what, inf)
    hi, lo = ct.scale_parts()
    assert LD(hi) + LD(lo) == r.scale, (what, "80-bit scale")
    assert np.array_equal(ct.export(), r.d), what


def _check(new, old, rev, a, b, ops):
    """a[i] (op) b[i] through the batched call under test against the three references"""
    for op in ops:
        want = [getattr(rev, op)(x.r, y.r) for x, y in zip(a, b)]
        batch = "add_batch" if op == "add" else "mult_batch"
        got = getattr(new, batch)([x.new for x in a], [y.new for y in b])
        ref = getattr(old, batch)([x.old for x in a], [y.old for y in b])
        for i, w in enumerate(want):
            _same(got[i], w, (op, i, "one launch per group vs oracle"))
            _same(ref[i], w, (op, i, "one launch per ciphertext vs oracle"))
            _same(getattr(new, op)(a[i].new, b[i].new), w, (op, i, "pair by pair vs oracle"))   # read at once: a batch of one


# (ring, target limbs, limbs of the sources, operations): a source exactly one limb above the target is read densely, one several limbs
# above with a stride that skips its upper limbs; groups of 1, 2 and 5, sources of different limb counts in one call
GROUPS = [
    ("toy", 1, [2], ["add", "mult"]),
    ("toy", 1, [2, 2], ["add", "mult"]),
    ("toy", 1, [2, 9, 14, 2, 5], ["add"]),
    ("toy", 2, [3, 3], ["add"]),
    ("toy", 2, [14, 6], ["add", "mult"]),
    ("toy", 2, [3, 5, 14, 3, 7], ["add", "mult"]),
    ("toy", 11, [12, 12], ["add"]),
    ("toy", 11, [12, 14, 13, 12, 14], ["add", "mult"]),
    ("toy13", 1, [2, 4, 7, 2, 2], ["add", "mult"]),
    ("toy13", 2, [3, 3], ["add"]),
    ("toy13", 2, [7, 3, 5, 7, 3], ["add"]),
]


@pytest.mark.parametrize("ring,target,srcs,ops", GROUPS, ids=[f"{g[0]}-t{g[1]}-n{len(g[2])}-{i}" for i, g in enumerate(GROUPS)])
def test_group_shapes(rings, orc, ring, target, srcs, ops):
    new, old, rev = rings(ring)
    lo = [Operand(orc, new, old, rev, 100 + 7 * i, target) for i in range(len(srcs))]
    hi = [Operand(orc, new, old, rev, 900 + 11 * i, e) for i, e in enumerate(srcs)]
    # the operand with more limbs on either side of the call
    a = [h if i % 2 == 0 else l for i, (h, l) in enumerate(zip(hi, lo))]
    b = [l if i % 2 == 0 else h for i, (h, l) in enumerate(zip(hi, lo))]
    _check(new, old, rev, a, b, ops)


@pytest.mark.parametrize("ring,target,cycle", [("toy", 2, [3, 6, 4]), ("toy", 11, [12, 13]), ("toy13", 2, [3, 7, 5])])
def test_group_crosses_the_item_cap(rings, orc, ring, target, cycle):
    """34 pairs over 33 distinct sources (one ciphertext serves two pairs and is adjusted once): 32 items in the first launch, 1 in the
    second"""
    new, old, rev = rings(ring)
    n = 34
    lo = [Operand(orc, new, old, rev, 100 + 7 * i, target) for i in range(n)]
    hi = [Operand(orc, new, old, rev, 900 + 11 * i, cycle[i % len(cycle)]) for i in range(n)]
    hi[20] = hi[4]
    _check(new, old, rev, hi, lo, ["add"])


def test_shared_source_in_a_small_group(rings, orc):
    """the same ciphertext on three of five pairs"""
    new, old, rev = rings("toy")
    lo = [Operand(orc, new, old, rev, 100 + 7 * i, 2) for i in range(5)]
    s = Operand(orc, new, old, rev, 77, 6)
    hi = [s, Operand(orc, new, old, rev, 78, 3), s, Operand(orc, new, old, rev, 79, 6), s]
    _check(new, old, rev, hi, lo, ["add", "mult"])


def test_component_counts_in_one_group(rings, orc):
    """pairs of two and of three components brought to one target in one call: one block and one launch per component count, a single
    ciphertext of its shape on its own"""
    new, old, rev = rings("toy")
    for n3 in (1, 2):
        lo = [Operand(orc, new, old, rev, 100 + 7 * i, 2, npoly=3 if i < n3 else 2) for i in range(n3 + 3)]
        hi = [Operand(orc, new, old, rev, 900 + 11 * i, 4 + i, npoly=3 if i < n3 else 2) for i in range(n3 + 3)]
        _check(new, old, rev, hi, lo, ["add"])


def test_scale_that_differs_in_its_80_bits_falls_back(rings, orc):
    """a group whose partners agree in the double part of their scale but not in all 80 bits is left to match(), pair by pair"""
    new, old, rev = rings("toy")
    from oracle.residue_eval import RCt
    sf = rev.sf[len(new.q) - 3]
    odd = Operand(orc, new, old, rev, 55, 3, deg=2, scale=float(sf * sf))     # rescaled below: a scale with 80 significant bits, 2 limbs
    odd.new, odd.old, odd.r = new.rescale(odd.new), old.rescale(odd.old), rev.rescale(odd.r)
    hi_s, lo_s = odd.new.scale_parts()
    assert LD(hi_s) + LD(lo_s) == odd.r.scale
    assert lo_s != 0.0, "the rescaled scale is a double: the case needs another seed of scales"
    lo = [Operand(orc, new, old, rev, 100 + 7 * i, 2, scale=hi_s) for i in range(3)]      # the same double, other low bits
    lo.insert(1, odd)
    hi = [Operand(orc, new, old, rev, 900 + 11 * i, 5) for i in range(4)]
    assert isinstance(odd.r, RCt)
    _check(new, old, rev, hi, lo, ["add"])
