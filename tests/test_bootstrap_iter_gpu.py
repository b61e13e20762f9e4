"""Iterative (two-pass) bootstrapping, the reference's EvalBootstrap(c, 2, precision) (src/FHEController.cpp:454-469), residue for
residue against the oracle.  The engine defines the operation as a fixed composition (include/fhelin.h
fhelin_bootstrap_iter); _iter_oracle below composes the same steps from oracle/residue_eval.py and oracle/residue_boot.py:

    x2 = x rescaled if degree 2, reduced to 2 limbs          (what ModRaise reads)
    y  = BTS_d(x)                                            (ell_y limbs, scale s_y)
    e' = mult_int(sub(y, x2), 2^p)                           (FLEXIBLEAUTO brings y to x2's limbs and exact scale)
    z  = BTS_d(e')                                           (same limbs and scale as y)
    w  = 2^p y - z                                           (scale 2^p s_y)
    out = rescale(mult_int(w, k)),  k = round(Delta_{level(y)+1} q_{ell_y-1} / (2^p s_y))

Exported residues, (npoly, ell, deg) and the 80-bit scale must be EQUAL."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
LD = np.longdouble
FHELIN_ERR_ARG, FHELIN_ERR_STATE = 1, 4


def _rev(eng, keys):
    from oracle.residue_eval import ResidueEvaluator
    return ResidueEvaluator(eng.q, eng.p, eng.psi_q, eng.psi_p, eng.alpha, eng.log_n, keys, eng.params.log_slots)


def _same(ct, r, what=""):
    inf = ct.info()
    assert (inf["npoly"], inf["ell"], inf["deg"]) == (r.npoly, r.ell, r.deg), (what, inf, r.ell, r.deg)
    hi, lo = ct.scale_parts()
    assert LD(hi) + LD(lo) == r.scale, (what, "scale")
    assert np.array_equal(ct.export(), r.d), what


def _boot_setup(fa, preset, log_slots, **over):
    """engine with real keys + bootstrapping set up; returns (engine, oracle-side bootstrapper)"""
    from oracle.residue_boot import ResidueBootstrapper
    eng = fa.Engine(preset, seed=77, log_slots=log_slots, **over)
    eng.keygen()
    eng.gen_relin_key()
    eng.bootstrap_setup(3, 3, 1 << log_slots)
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
    boot = ResidueBootstrapper(_rev(eng, keys), desc, lambda pt: (lambda ell, sc: eng.pt_export(pt, ell, sc)))
    return eng, boot


def _input(eng, n, ell, seed, deg=1):
    """a fresh encryption with `ell` limbs; deg=2: its square (relinearised, not rescaled: ell - 1 limbs after the rescale)"""
    from oracle.residue_eval import RCt
    m = np.random.default_rng(seed).uniform(-1, 1, n)
    ct = eng.encrypt(m, level=eng.n_q - ell)
    if deg == 2:
        ct = eng.mult(ct, ct)
        m = m * m
    hi, lo = ct.scale_parts()
    inf = ct.info()
    assert inf["deg"] == deg
    return m, ct, RCt(ct.export(), inf["deg"], LD(hi) + LD(lo))


def _iter_oracle(boot, r, p, drop):
    from oracle.residue_eval import _llround
    rev = boot.rev
    x2 = rev.rescale(r) if r.deg >= 2 else r
    if x2.ell > 2:
        x2 = rev.level_reduce(x2, 2)
    y = boot.run(r, drop=drop)
    e = rev.sub(y, x2)
    assert e.ell == 2 and e.scale == x2.scale
    e = rev.mult_int(e, 1 << p, False, e.scale)
    z = boot.run(e, drop=drop)
    assert (z.ell, z.deg, z.scale) == (y.ell, y.deg, y.scale)
    w = rev.sub(rev.mult_int(y, 1 << p, False, y.scale * LD(1 << p)), z)
    k = _llround(rev.sf[rev.level(y) + 1] * LD(int(rev.q[y.ell - 1])) / w.scale)
    return rev.rescale(rev.mult_int(w, k, True, w.scale * LD(k))), y


@pytest.fixture(scope="module", params=[10, 11], ids=["packed", "full"])
def boot12(request, fa, orc):
    eng, boot = _boot_setup(fa, "boot12", request.param)
    yield eng, boot
    eng.close()


@pytest.mark.parametrize("p,drop,ell,deg", [
    (8, 0, 3, 1),
    (12, 3, 2, 1),
    (12, 0, 5, 2),      # degree 2 and more than 2 limbs: rescaled, then reduced to 2 limbs before ModRaise
])
def test_bootstrap_iter_bit_exact(boot12, p, drop, ell, deg):
    eng, boot = boot12
    m, ct, r = _input(eng, boot.n, ell, 11 + p + drop, deg)
    want, y = _iter_oracle(boot, r, p, drop)
    assert want.ell == y.ell - 1 == eng.n_q - boot.desc["depth"] - drop - 1
    got = eng.bootstrap_iter_drop(ct, p, drop)
    _same(got, want, ("bootstrap_iter", p, drop, ell, deg))
    # ... and it is a bootstrap: at this small ring the error is the encryption noise's, not the approximation's
    assert np.max(np.abs(eng.decrypt(got) - m)) < 2e-4
    if drop == 0:        # the level plan's default: the deferred per-handle call gives the same bytes
        _same(eng.bootstrap_iter(ct, p), want, "bootstrap_iter (deferred)")


def test_bootstrap_iter_batch_deferral_and_plan(fa, orc):
    """a batch of three inputs at different levels == the single calls; per-handle calls are deferred until the first read, then
    both bootstraps of all three run (stats: 2 x 3); a recorded and applied level plan gives the bytes of the explicit drop"""
    eng, boot = _boot_setup(fa, "boot12", 10)
    try:
        ins = [_input(eng, boot.n, ell, 40 + ell, deg) for ell, deg in ((2, 1), (4, 1), (6, 2))]
        single = [eng.bootstrap_iter_drop(ct, 10, 0) for _, ct, _ in ins]
        batch = eng.bootstrap_iter_batch([ct for _, ct, _ in ins], 10)
        for s, b in zip(single, batch):
            assert np.array_equal(s.export(), b.export()) and s.info() == b.info() and s.scale_parts() == b.scale_parts()
        want, _ = _iter_oracle(boot, ins[2][2], 10, 0)
        _same(batch[2], want, "batch vs oracle")

        eng.sync()
        before = eng.stats()["bootstrap"]
        lazy = [eng.bootstrap_iter(ct, 10) for _, ct, _ in ins]
        # issuing is not reading: nothing runs yet
        assert eng.stats()["bootstrap"] == before
        first = lazy[0].export()
        assert eng.stats()["bootstrap"] == before + 2 * 3
        assert np.array_equal(first, single[0].export())
        for s, h in zip(single[1:], lazy[1:]):
            assert np.array_equal(s.export(), h.export())

        # level plan: the iterative bootstrap is source 0 of the recorded program; three products follow before a decryption
        m, ct, _ = ins[0]
        eng.level_plan_begin("record")
        v = eng.bootstrap_iter(ct, 10)
        for _ in range(3):
            v = eng.mult_const(v, 0.5)
        eng.decrypt(v)
        plan = eng.level_plan_end()
        full = eng.n_q - boot.desc["depth"] - 1
        assert 2 <= plan[0] < full
        eng.level_plan_begin("apply")
        planned = eng.bootstrap_iter(ct, 10)
        planned_data = planned.export()
        eng.level_plan_begin("off")
        explicit = eng.bootstrap_iter_drop(ct, 10, full - plan[0])
        assert planned.info()["ell"] == plan[0]
        assert np.array_equal(planned_data, explicit.export()) and planned.scale_parts() == explicit.scale_parts()
        assert np.max(np.abs(eng.decrypt(planned) - m)) < 2e-4
    finally:
        eng.close()


def test_bootstrap_iter_batch_groups_inputs_by_planned_drop(fa):
    """an applied level plan gives the three inputs of ONE fhelin_bootstrap_iter_batch the drops [2, 1, 2]: inputs of equal drop share
    a batch, every output holds the residues of fhelin_bootstrap_iter_drop with its own drop, and the call takes three sources"""
    eng = fa.Engine("boot12", seed=77, log_slots=10)
    try:
        eng.keygen()
        eng.gen_relin_key()
        eng.bootstrap_setup(3, 3, 1 << 10)
        rng = np.random.default_rng(23)
        cts = [eng.encrypt(rng.uniform(-1, 1, 1 << 10), level=eng.n_q - ell) for ell in (3, 2, 4)]
        drops = [2, 1, 2]
        single = [eng.bootstrap_iter_drop(c, 10, d).export() for c, d in zip(cts, drops)]
        full = eng.n_q - eng.bootstrap_describe()["depth"] - 1
        eng.set_level_plan([full - d for d in drops])
        eng.level_plan_begin("apply")
        got = eng.bootstrap_iter_batch(cts, 10)
        assert eng.level_plan_tell() == ("apply", 3)
        eng.level_plan_begin("off")
        for g, s, d in zip(got, single, drops):
            assert g.info()["ell"] == full - d and np.array_equal(g.export(), s)
    finally:
        eng.close()


def test_bootstrap_iter_errors(boot12, fa):
    eng, boot = boot12
    _, ct, _ = _input(eng, boot.n, 3, 5)
    for p in (0, 31, -1):
        with pytest.raises(fa.FhelinError) as ei:
            eng.bootstrap_iter(ct, p)
        assert ei.value.code == FHELIN_ERR_ARG, p
        with pytest.raises(fa.FhelinError) as ei:
            eng.bootstrap_iter_batch([ct], p)
        assert ei.value.code == FHELIN_ERR_ARG, p
    before = eng.stats()["bootstrap"]
    full = eng.n_q - boot.desc["depth"]
    with pytest.raises(fa.FhelinError) as ei:
        eng.bootstrap_iter_drop(ct, 8, full - 2)          # one bootstrap would keep 2 limbs: none left for the final scaling
    assert ei.value.code == FHELIN_ERR_STATE
    assert eng.stats()["bootstrap"] == before             # refused before any device work
    assert eng.bootstrap_iter_drop(ct, 8, full - 3).info()["ell"] == 2


# worst max |dec(out) - x| of the iterative bootstrap (p = 12) at the headline ring measured on the MI355X, over drop 0 and 4:
# 9.70e-9 (drop 4; drop 0: 9.58e-9), against 3.77e-5 / 3.65e-5 for one bootstrap of the same input
ITER_ERR_MEASURED = 9.70e-9
ITER_ERR_BOUND = 1.5 * ITER_ERR_MEASURED


@pytest.mark.parametrize("drop", [0, 4])
def test_bootstrap_iter_precision_headline_ring(fa, drop):
    """the ring bench.py's forward pass runs (N=2^16, 28+7 limbs, 16384 slots): p = 12 removes at least 2^8 of one bootstrap's
    error on the same input (measured on the MI355X: 3.65e-5 -> 9.58e-9 at drop 0, 3.77e-5 -> 9.70e-9 at drop 4, about 3800 x);
    absolute bound 1.5 x the worst value measured there (convention of test_bootstrap_gpu.py)"""
    eng = fa.Engine("bench", seed=5, n_q=28, n_p=-1)
    try:
        eng.keygen()
        eng.gen_relin_key()
        eng.bootstrap_setup(3, 3, 1 << 14)
        m = np.random.default_rng(21).uniform(-1, 1, 1 << 14)
        ct = eng.encrypt(m, level=eng.n_q - 3)
        one = eng.bootstrap_drop(ct, drop)
        two = eng.bootstrap_iter_drop(ct, 12, drop)
        assert two.info()["ell"] == one.info()["ell"] - 1
        e1 = float(np.max(np.abs(eng.decrypt(one) - m)))
        e2 = float(np.max(np.abs(eng.decrypt(two) - m)))
        print(f"headline ring, drop {drop}: single {e1:.3e}, iterative p=12 {e2:.3e}, gain {e1 / e2:.0f}")
        assert e2 * 2 ** 8 <= e1, (e1, e2)
        assert e2 < ITER_ERR_BOUND, (e1, e2)
    finally:
        eng.close()
