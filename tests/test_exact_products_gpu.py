"""Relinearised products that are rescaled inside their ModDown (Evaluator::mult_affine_batch): the power steps of a
Chebyshev evaluation and EvalMod's double angle run rescale(f a b + constant +- addend) through ONE batched key switch whose tail
(Evaluator::moddown_rescale_exact) keeps the two roundings of ModDown and rescale.  Three things must agree byte for byte:

  * the library as it is built (the exact merged tail),
  * the library with FHELIN_EXACT_PRODUCTS=0 (mult_batch, add_batch, add_real / sub_batch, rescale_batch: the sequence itself),
  * oracle/residue_eval.py's default path, which composes that sequence from the oracle's integer functions.

Compared: one round that mixes even powers, odd powers (operands at different levels, a subtrahend from the level above), a degree-2
operand, a factor-1 product with an added degree-2 addend and an item with constant AND subtrahend, at 24, 12, 3 and 2 product limbs, for
1 and 5 rows, on N=2^12 and N=2^13; a Chebyshev evaluation of degree 119; EvalMod; one whole bootstrap."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
LD = np.longdouble


def _uniform_ct(orc, eng, seed, ell):
    return np.stack([orc.uniform_residues(seed + 1000 * p, eng.q[:ell], eng.N) for p in range(2)])


def _uniform_key(orc, eng, seed):
    d = eng.dnum_digits
    k = np.stack([orc.uniform_residues(seed + 50 * j, eng.moduli, eng.N) for j in range(2 * d)])
    return k.reshape(d, 2, eng.n_limbs, eng.N)


def _rev(eng, keys):
    from oracle.residue_eval import ResidueEvaluator
    return ResidueEvaluator(eng.q, eng.p, eng.psi_q, eng.psi_p, eng.alpha, eng.log_n, keys, eng.params.log_slots)


def _same(ct, r, what=""):
    inf = ct.info()
    assert (inf["npoly"], inf["ell"], inf["deg"]) == (r.npoly, r.ell, r.deg), (what, inf, r.ell, r.deg)
    hi, lo = ct.scale_parts()
    assert LD(hi) + LD(lo) == r.scale, (what, "scale")
    got = ct.export()
    assert got.dtype == r.d.dtype and got.tobytes() == r.d.tobytes(), what


def _same_ct(a, b, what=""):
    ia, ib = a.info(), b.info()
    assert (ia["npoly"], ia["ell"], ia["deg"]) == (ib["npoly"], ib["ell"], ib["deg"]), (what, ia, ib)
    assert a.scale_parts() == b.scale_parts(), (what, "scale")
    assert a.export().tobytes() == b.export().tobytes(), what


@pytest.fixture(scope="module")
def engines(fa, orc):
    """(preset, overrides) -> (default engine, engine with the knob at 0, oracle evaluator), one uniform 'relinearisation key' for all
    three (parity of integer functions does not need a real one)"""
    made = {}

    def get(preset, **over):
        key = (preset, tuple(sorted(over.items())))
        if key not in made:
            mp = pytest.MonkeyPatch()
            e1 = fa.Engine(preset, seed=9, **over)
            mp.setenv("FHELIN_EXACT_PRODUCTS", "0")
            try:
                e0 = fa.Engine(preset, seed=9, **over)
            finally:
                mp.undo()
            relin = _uniform_key(orc, e1, 31)
            e1.key_import(0, 0, relin)
            e0.key_import(0, 0, relin)
            made[key] = (e1, e0, _rev(e1, {"relin": relin}))
        return made[key]

    yield get
    for e1, e0, _ in made.values():
        e1.close()
        e0.close()


def _round(orc, eng, rev, ell, rows, seed):
    """operand lists of one mixed round whose products have `ell` limbs: per row, with T1 one level above T2,
         2 T2 T2 - 1          (even power)
         2 T1 T2 - T1         (odd power: the pair and the subtrahend are level-adjusted)
         2 D  T2 - 1 - T1     (D of degree 2 is rescaled first; constant and subtrahend together)
         1 T2 T2 + A          (factor 1; A of degree 2 at the product's limbs is added as it stands)
    each item (a, b, factor, constant, addend or None, negate) over values (residues, degree, scale) that the engines import and the
    oracle wraps as they are"""
    n_q = len(eng.q)
    items = []
    for i in range(rows):
        def val(s, limbs, deg=1):
            sc = LD(float(rev.sf[n_q - limbs]))
            if deg == 2:
                sc = LD(float(sc * sc))
            return (_uniform_ct(orc, eng, seed + 97 * i + s, limbs), deg, sc)
        t1, t2 = val(1, ell + 1), val(2, ell)
        dd = val(3, ell + 1, 2)
        aa = val(4, ell, 2)
        items += [(t2, t2, 2, -1.0, None, False), (t1, t2, 2, 0.0, t1, True), (dd, t2, 2, -1.0, t1, True), (t2, t2, 1, 0.0, aa, False)]
    return items


def _run_lib(eng, items):
    cache = {}

    def h(v):
        if id(v) not in cache:
            cache[id(v)] = eng.ct_import(v[0], deg=v[1], scale=float(v[2]))
        return cache[id(v)]
    a = [h(it[0]) for it in items]
    b = [h(it[1]) for it in items]
    ad = [h(it[4]) if it[4] is not None else None for it in items]
    return eng.mult_affine_batch(a, b, [it[2] for it in items], [it[3] for it in items], ad, [it[5] for it in items])


def _run_oracle(rev, items):
    from oracle.residue_eval import RCt
    cache = {}

    def r(v):
        if id(v) not in cache:
            cache[id(v)] = RCt(v[0], v[1], v[2])
        return cache[id(v)]
    out = []
    for a, b, f, cadd, ad, neg in items:
        t = rev.mult(r(a), r(b))
        if f == 2:
            t = rev.add(t, t)
        if cadd != 0.0:
            t = rev.add_real(t, cadd)
        if ad is not None:
            t = rev.sub(t, r(ad)) if neg else rev.add(t, r(ad))
        out.append(rev.rescale(t))
    return out


@pytest.mark.parametrize("preset,over,ell,rows", [
    ("boot12", {"n_q": 26, "n_p": -1}, 24, 1),
    ("boot12", {"n_q": 26, "n_p": -1}, 24, 5),
    ("boot12", {"n_q": 26, "n_p": -1}, 12, 5),
    ("boot12", {"n_q": 26, "n_p": -1}, 3, 1),
    ("boot12", {"n_q": 26, "n_p": -1}, 2, 5),
    ("toy13", {}, 5, 5),
    ("toy13", {}, 3, 1),
    ("toy13", {}, 2, 5),
])
def test_mixed_round_in_one_call_bit_exact(engines, orc, preset, over, ell, rows):
    e1, e0, rev = engines(preset, **over)
    items = _round(orc, e1, rev, ell, rows, 7000 + 10 * ell + rows)
    got1, got0, want = _run_lib(e1, items), _run_lib(e0, items), _run_oracle(rev, items)
    assert len(got1) == len(got0) == len(want) == 4 * rows
    for k, (g1, g0, w) in enumerate(zip(got1, got0, want)):
        assert w.ell == ell - 1 and w.deg == 1
        _same(g1, w, ("exact tail vs oracle", preset, ell, rows, k))
        _same(g0, w, ("sequence vs oracle", preset, ell, rows, k))
        _same_ct(g1, g0, ("exact tail vs sequence", preset, ell, rows, k))


def test_addend_below_its_product_runs_the_sequence(engines, orc):
    """an addend with FEWER limbs than its product: the sequence adjusts the PRODUCT to the addend (match), which the tail cannot do, so the
    whole call runs the sequence on the prepared operands - same bytes as the oracle and as the knob at 0, an ordinary item included"""
    e1, e0, rev = engines("toy13")
    ell, n_q = 4, len(e1.q)

    def val(s, limbs):
        return (_uniform_ct(orc, e1, 9100 + s, limbs), 1, LD(float(rev.sf[n_q - limbs])))
    t1, t2, low = val(1, ell + 1), val(2, ell), val(3, ell - 1)
    items = [(t2, t2, 2, -1.0, low, True), (t1, t2, 2, -1.0, None, False)]
    got1, got0, want = _run_lib(e1, items), _run_lib(e0, items), _run_oracle(rev, items)
    assert want[0].ell < ell - 1 and want[1].ell == ell - 1
    for k, (g1, g0, w) in enumerate(zip(got1, got0, want)):
        _same(g1, w, ("fallback vs oracle", k))
        _same(g0, w, ("sequence vs oracle", k))
        _same_ct(g1, g0, ("fallback vs sequence", k))


def _cheb_fit(f, a, b, degree):
    n = degree + 1
    j = np.arange(n)
    nodes = np.cos(np.pi * (j + 0.5) / n)
    fx = np.array([f(0.5 * (b - a) * t + 0.5 * (b + a)) for t in nodes])
    return [float(2.0 / n * np.sum(fx * np.cos(np.pi * k * (j + 0.5) / n))) for k in range(n)]


def test_chebyshev_degree_119_bit_exact(engines, orc):
    """eval_gelu_function's series from the top of a 22-limb chain: four baby rounds, two giant squarings"""
    from oracle.residue_eval import RCt
    e1, e0, rev = engines("boot12")
    coeffs = _cheb_fit(lambda x: 1.0 / (x + 130.0), -1.0, 1.0, 119)
    x = _uniform_ct(orc, e1, 4119, 22)
    sc = float(rev.sf[0])
    want = rev.eval_chebyshev(RCt(x, 1, LD(sc)), coeffs, -1.0, 1.0)
    got1 = e1.eval_chebyshev(e1.ct_import(x, deg=1, scale=sc), coeffs, -1.0, 1.0)
    got0 = e0.eval_chebyshev(e0.ct_import(x, deg=1, scale=sc), coeffs, -1.0, 1.0)
    _same(got1, want, "chebyshev 119, exact tail")
    _same(got0, want, "chebyshev 119, sequence")
    _same_ct(got1, got0, "chebyshev 119")
    # two rows through one call: the rounds are twice as wide
    y = _uniform_ct(orc, e1, 4120, 22)
    both = e1.eval_chebyshev_batch([e1.ct_import(x, deg=1, scale=sc), e1.ct_import(y, deg=1, scale=sc)], coeffs, -1.0, 1.0)
    _same(both[0], want, "chebyshev 119, row 0 of 2")
    _same(both[1], rev.eval_chebyshev(RCt(y, 1, LD(sc)), coeffs, -1.0, 1.0), "chebyshev 119, row 1 of 2")


def _boot_setup(fa, preset, log_slots, **over):
    eng = fa.Engine(preset, seed=77, log_slots=log_slots, **over)
    eng.keygen()
    eng.gen_relin_key()
    eng.bootstrap_setup(3, 3, 1 << log_slots)
    return eng


def _boot_oracle(eng):
    from oracle.residue_boot import ResidueBootstrapper
    desc = eng.bootstrap_describe()
    keys = {"relin": eng.key_export(0), "conj": eng.key_export(2)}
    need = set()
    for st in desc["c2s"] + desc["s2c"]:
        for (g, b, _) in st["terms"]:
            need.update((g, b))
    n = desc["slots"]
    j = 1
    while j < (eng.N // 2) // n:
        need.add(n * j)
        j <<= 1
    for r in sorted(need):
        if r:
            keys[r] = eng.key_export(1, r)
    rev = _rev(eng, keys)
    return ResidueBootstrapper(rev, desc, lambda pt: (lambda ell, sc: eng.pt_export(pt, ell, sc)))


def test_evalmod_and_bootstrap_bit_exact(fa, orc, monkeypatch):
    """EvalMod (its double-angle steps but the last rescale inside their ModDown) and the whole bootstrap, N=2^12, sparse packing, real
    keys: the same secret seed gives both engines the same keys and the same input ciphertext"""
    from oracle.residue_eval import RCt
    e1 = _boot_setup(fa, "boot12", 10)
    monkeypatch.setenv("FHELIN_EXACT_PRODUCTS", "0")
    e0 = _boot_setup(fa, "boot12", 10)
    monkeypatch.delenv("FHELIN_EXACT_PRODUCTS")
    try:
        assert e1.key_export(0).tobytes() == e0.key_export(0).tobytes()
        boot = _boot_oracle(e1)
        m = np.random.default_rng(3).uniform(-1, 1, boot.n)
        c1, c0 = e1.encrypt(m, level=e1.n_q - 3), e0.encrypt(m, level=e0.n_q - 3)
        _same_ct(c1, c0, "input")
        hi, lo = c1.scale_parts()
        r = RCt(c1.export(), c1.info()["deg"], LD(hi) + LD(lo))
        want = boot.run(r, stop_after=3)
        g1, g0 = e1.bootstrap_partial(c1, 3), e0.bootstrap_partial(c0, 3)
        assert g1.export().tobytes() == want.d.tobytes(), "EvalMod, exact tail vs oracle"
        assert g0.export().tobytes() == want.d.tobytes(), "EvalMod, sequence vs oracle"
        _same_ct(g1, g0, "EvalMod")
        want = boot.run(r)
        o1, o0 = e1.bootstrap(c1), e0.bootstrap(c0)
        _same(o1, want, "bootstrap, exact tail")
        _same(o0, want, "bootstrap, sequence")
        _same_ct(o1, o0, "bootstrap")
        assert np.max(np.abs(e1.decrypt(o1) - m)) < 2e-4
    finally:
        e1.close()
        e0.close()
