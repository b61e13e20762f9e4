"""Paired bootstrapping (include/fhelin.h "Paired bootstrapping"): two real ciphertexts through ONE bootstrap as a + i b.

Residue for residue against tests/boot_pair_model.py (a composition over oracle/residue_boot.py) at N = 2^12, 22+6 limbs with real keys,
set up as tests/test_boot_residue_gpu.py sets its engines up; the two kernels alone over crafted residues against the oracle's dyadic
functions; the batch entry, the runtime knob, the refusals, and the decryption error next to a single bootstrap's."""
import numpy as np
import pytest

from boot_pair_model import PairBootstrapper

pytestmark = pytest.mark.gpu
LD = np.longdouble
ABS_BOUND = 2e-4        # what the existing bootstrap tests ask at this ring
ERR_ARG, ERR_STATE = 1, 4


def _rev(eng, keys):
    from oracle.residue_eval import ResidueEvaluator
    return ResidueEvaluator(eng.q, eng.p, eng.psi_q, eng.psi_p, eng.alpha, eng.log_n, keys, eng.params.log_slots)


def _same(ct, r, what=""):
    inf = ct.info()
    assert (inf["npoly"], inf["ell"], inf["deg"]) == (r.npoly, r.ell, r.deg), (what, inf, r.ell, r.deg)
    hi, lo = ct.scale_parts()
    assert LD(hi) + LD(lo) == r.scale, (what, "scale")
    assert np.array_equal(ct.export(), r.d), what


def _boot_setup(fa, preset, log_slots, budget=(3, 3), **over):
    """engine with real keys + bootstrapping set up; returns (engine, test-side pair model over the oracle's bootstrapper)"""
    eng = fa.Engine(preset, seed=77, log_slots=log_slots, **over)
    eng.keygen()
    eng.gen_relin_key()
    eng.bootstrap_setup(budget[0], budget[1], 1 << log_slots)
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
    boot = PairBootstrapper(_rev(eng, keys), desc, lambda pt: (lambda ell, sc: eng.pt_export(pt, ell, sc)))
    return eng, boot


def _rct(ct):
    from oracle.residue_eval import RCt
    hi, lo = ct.scale_parts()
    return RCt(ct.export(), ct.info()["deg"], LD(hi) + LD(lo))


def _boot_input(eng, boot, ell_left=3, seed=3):
    m = np.random.default_rng(seed).uniform(-1, 1, boot.n)
    ct = eng.encrypt(m, level=eng.n_q - ell_left)
    return m, ct, _rct(ct)


@pytest.fixture(scope="module")
def boots(fa, orc):
    """(engine, model) per log_slots, made once for the module: 10 = sparse packing (SubSum, one EvalMod ciphertext), 11 = full"""
    made = {}

    def get(log_slots):
        if log_slots not in made:
            made[log_slots] = _boot_setup(fa, "boot12", log_slots)
        return made[log_slots]

    yield get
    for eng, _ in made.values():
        eng.close()


@pytest.fixture(scope="module")
def pair10(boots):
    """the two inputs most tests share (3 and 5 limbs left: different k0 and rho) with the model's complete pair, computed once"""
    eng, boot = boots(10)
    ma, ca, ra = _boot_input(eng, boot, ell_left=3, seed=3)
    mb, cb, rb = _boot_input(eng, boot, ell_left=5, seed=4)
    return dict(eng=eng, boot=boot, m=(ma, mb), ct=(ca, cb), r=(ra, rb), want=boot.pair(ra, rb))


# ---- the pipeline, bit for bit ------------------------------------------------------------------------------------------------------
def test_pair_stages_bit_exact_sparse_packing(pair10):
    """pack + ModRaise + SubSum, CoeffsToSlots + conjugation, EvalMod, then the complete pair: residues, limbs, degree and 80-bit scale
    of BOTH outputs equal the model's; the inputs sit at different levels"""
    eng, boot, (ca, cb), (ra, rb) = pair10["eng"], pair10["boot"], pair10["ct"], pair10["r"]
    assert boot.desc["packed"]
    for stage in (1, 2, 3):
        _same(eng.bootstrap_pair_partial(ca, cb, stage), boot.pair(ra, rb, stop_after=stage), ("stage", stage))
    got_a, got_b = eng.bootstrap_pair(ca, cb)
    _same(got_a, pair10["want"][0], "pair: a")
    _same(got_b, pair10["want"][1], "pair: b")
    single = eng.bootstrap(ca).info()
    for g in (got_a, got_b):           # what everything downstream sees: the shape of a single bootstrap's result
        assert (g.info()["ell"], g.info()["deg"], g.info()["slots"]) == (single["ell"], single["deg"], single["slots"])


def test_pair_stages_bit_exact_full_packing(boots):
    eng, boot = boots(11)
    assert not boot.desc["packed"]
    _, ca, ra = _boot_input(eng, boot, ell_left=3, seed=3)
    _, cb, rb = _boot_input(eng, boot, ell_left=5, seed=4)
    for stage in (1, 2, 3):
        _same(eng.bootstrap_pair_partial(ca, cb, stage), boot.pair(ra, rb, stop_after=stage), ("stage", stage))
    got, want = eng.bootstrap_pair(ca, cb), boot.pair(ra, rb)
    _same(got[0], want[0], "pair: a")
    _same(got[1], want[1], "pair: b")


def test_pair_with_a_degree_2_input_bit_exact(boots):
    """a degree-2 input is rescaled first, as a single bootstrap's is"""
    eng, boot = boots(10)
    ma, c0, _ = _boot_input(eng, boot, ell_left=4, seed=6)
    ca = eng.mult_real(c0, 1.0)
    assert ca.info()["deg"] == 2
    mb, cb, rb = _boot_input(eng, boot, ell_left=5, seed=7)
    got, want = eng.bootstrap_pair(ca, cb), boot.pair(_rct(ca), rb)
    _same(got[0], want[0], "pair: a (degree 2)")
    _same(got[1], want[1], "pair: b")
    assert max(np.max(np.abs(eng.decrypt(got[0]) - ma)), np.max(np.abs(eng.decrypt(got[1]) - mb))) < ABS_BOUND


def test_pair_to_fewer_limbs_bit_exact(boots):
    """an explicit drop and an applied level plan (both outputs are sources of their own) give the model's residues"""
    eng, boot = boots(10)
    _, ca, ra = _boot_input(eng, boot, ell_left=2, seed=5)
    _, cb, rb = _boot_input(eng, boot, ell_left=3, seed=8)
    full = eng.n_q - boot.desc["depth"]
    for drop in (2, 4):
        want = boot.pair(ra, rb, drop=drop)
        assert want[0].ell == want[1].ell == full - drop
        got = eng.bootstrap_pair_drop(ca, cb, drop)
        _same(got[0], want[0], ("drop", drop, "a"))
        _same(got[1], want[1], ("drop", drop, "b"))
    eng.set_level_plan([full - 4, full - 4])
    eng.level_plan_begin("apply")
    out = eng.bootstrap_pair(ca, cb)
    eng.level_plan_begin("off")
    _same(out[0], want[0], "planned pair: a")
    _same(out[1], want[1], "planned pair: b")


# ---- batch, knob ----------------------------------------------------------------------------------------------------------------------
def test_paired_batch_of_three_and_of_four(pair10):
    """3 inputs: one pair + one single in ONE pipeline batch - the pair as the model has it, the single residue for residue what
    fhelin_bootstrap gives; the bootstrap counter advances per pipeline"""
    eng, boot, (ca, cb) = pair10["eng"], pair10["boot"], pair10["ct"]
    _, cc, _ = _boot_input(eng, boot, ell_left=4, seed=9)
    _, cd, _ = _boot_input(eng, boot, ell_left=2, seed=10)
    alone = eng.bootstrap(cc)
    alone_res, alone_info, alone_scale = alone.export(), alone.info(), alone.scale_parts()
    before = eng.stats()["bootstrap"]
    out = eng.bootstrap_paired_batch([ca, cb, cc])
    assert eng.stats()["bootstrap"] - before == 2
    _same(out[0], pair10["want"][0], "batch: a")
    _same(out[1], pair10["want"][1], "batch: b")
    assert np.array_equal(out[2].export(), alone_res) and out[2].info() == alone_info and out[2].scale_parts() == alone_scale
    # 4 inputs: two pairs in one batch, each with the residues of its own pipeline
    before = eng.stats()["bootstrap"]
    out4 = eng.bootstrap_paired_batch([ca, cb, cc, cd])
    assert eng.stats()["bootstrap"] - before == 2
    _same(out4[0], pair10["want"][0], "batch of 4: a")
    _same(out4[1], pair10["want"][1], "batch of 4: b")
    second = eng.bootstrap_pair(cc, cd)
    for k in range(2):
        assert np.array_equal(out4[2 + k].export(), second[k].export()) and out4[2 + k].scale_parts() == second[k].scale_parts()


def test_paired_batch_groups_inputs_by_planned_drop(pair10):
    """an applied level plan gives the three inputs of ONE fhelin_bootstrap_paired_batch the drops [2, 4, 2]: the first and the third
    share a pipeline and are its pair (fhelin_bootstrap_pair_drop), the second runs alone (fhelin_bootstrap_drop); three sources"""
    eng, boot, (ca, cb) = pair10["eng"], pair10["boot"], pair10["ct"]
    _, cc, _ = _boot_input(eng, boot, ell_left=4, seed=9)
    pair = [o.export() for o in eng.bootstrap_pair_drop(ca, cc, 2)]
    alone = eng.bootstrap_drop(cb, 4).export()
    full = eng.n_q - boot.desc["depth"]
    eng.set_level_plan([full - 2, full - 4, full - 2])
    eng.level_plan_begin("apply")
    out = eng.bootstrap_paired_batch([ca, cb, cc])
    assert eng.level_plan_tell() == ("apply", 3)
    eng.level_plan_begin("off")
    assert [o.info()["ell"] for o in out] == [full - 2, full - 4, full - 2]
    assert np.array_equal(out[0].export(), pair[0]) and np.array_equal(out[2].export(), pair[1])
    assert np.array_equal(out[1].export(), alone)


def test_pairing_knob_routes_deferred_bootstraps(pair10):
    """set_bootstrap_pairing(1): three deferred bootstrap() calls, read afterwards, are bootstrap_paired_batch; off (the default) they
    are bootstrap_batch as before"""
    eng, boot, (ca, cb) = pair10["eng"], pair10["boot"], pair10["ct"]
    _, cc, _ = _boot_input(eng, boot, ell_left=4, seed=9)
    ins = [ca, cb, cc]
    paired = [o.export() for o in eng.bootstrap_paired_batch(ins)]
    plain = [o.export() for o in eng.bootstrap_batch(ins)]
    assert not np.array_equal(paired[0], plain[0])
    assert not eng.bootstrap_pairing()
    eng.set_bootstrap_pairing(True)
    try:
        assert eng.bootstrap_pairing()
        before = eng.stats()["bootstrap"]
        outs = [eng.bootstrap(c) for c in ins]
        got = [o.export() for o in outs]
        assert eng.stats()["bootstrap"] - before == 2
    finally:
        eng.set_bootstrap_pairing(False)
    for g, w in zip(got, paired):
        assert np.array_equal(g, w)
    outs = [eng.bootstrap(c) for c in ins]
    for o, w in zip(outs, plain):
        assert np.array_equal(o.export(), w)


# ---- it is a bootstrap ----------------------------------------------------------------------------------------------------------------
def test_pair_decrypts_like_a_single_bootstrap(pair10):
    """Each output within the bound the single bootstrap's tests use at this ring, and within 2 x the larger error of fhelin_bootstrap on
    the same two inputs (each output takes one component of the same complex error whose real part the single path keeps, plus one
    low-level key switch).  The measured ratio is printed."""
    eng, (ma, mb), (ca, cb) = pair10["eng"], pair10["m"], pair10["ct"]
    single = max(np.max(np.abs(eng.decrypt(eng.bootstrap(ca)) - ma)), np.max(np.abs(eng.decrypt(eng.bootstrap(cb)) - mb)))
    oa, ob = eng.bootstrap_pair(ca, cb)
    ea, eb = np.max(np.abs(eng.decrypt(oa) - ma)), np.max(np.abs(eng.decrypt(ob) - mb))
    print(f"pair error a {ea:.3e} b {eb:.3e}; single {single:.3e}; ratio {max(ea, eb) / single:.3f}")
    assert ea < ABS_BOUND and eb < ABS_BOUND
    assert max(ea, eb) <= 2 * single


# ---- the kernels alone ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def bare(fa, orc):
    """no keys, no bootstrap set-up: the debug entries work on imported residues"""
    e = fa.Engine("boot12", seed=9)
    yield e
    e.close()


def _mono_i(orc, eng, ell):
    m = np.zeros((ell, eng.N), dtype=np.uint64)
    m[:, eng.N // 2] = 1
    return orc.ntt_batch(m, eng.q[:ell], eng.psi_q[:ell])


def _crafted(orc, eng, pattern, seed, ell):
    """(x, y) [2][ell][N] each: all 0; all q - 1; y = q - x (the sum wraps to exactly 0); x == y (the difference is 0)"""
    q = np.asarray(eng.q[:ell], dtype=np.uint64)[None, :, None]
    shape = (2, ell, eng.N)
    if pattern == "zero":
        return np.zeros(shape, dtype=np.uint64), np.zeros(shape, dtype=np.uint64)
    if pattern == "max":
        x = np.broadcast_to(q - np.uint64(1), shape).copy()
        return x, x.copy()
    x = np.stack([orc.uniform_residues(seed + 1000 * p, eng.q[:ell], eng.N) for p in range(2)])
    if pattern == "negated":
        return x, (q - x) % q
    assert pattern == "equal"
    return x, x.copy()


PATTERNS = ("zero", "max", "negated", "equal")


@pytest.mark.parametrize("n_pairs", [1, 3])
@pytest.mark.parametrize("ells", [(2, 2), (5, 5), (5, 2)])
def test_pack_kernel_crafted_residues(bare, orc, ells, n_pairs):
    """out = k0_a a + X^(N/2) k0_b b on the two bottom limbs, read in place from inputs of 2 and 5 limbs; k0 in {2, q_1 - 1, 2^64 - 1}"""
    eng = bare
    q2 = eng.q[:2]
    mono = _mono_i(orc, eng, 2)
    k0s = [2, int(eng.q[1]) - 1, 2 ** 64 - 1]
    for pi, pattern in enumerate(PATTERNS):
        a, b, ka, kb, want = [], [], [], [], []
        for i in range(n_pairs):
            x, _ = _crafted(orc, eng, pattern, 11 + 7 * i, ells[0])
            if pattern in ("zero", "max"):
                y = _crafted(orc, eng, pattern, 0, ells[1])[0]
            else:      # the relation holds on the limbs the kernel reads; the limbs above them are uniform
                y = np.stack([orc.uniform_residues(5 + 13 * i + 1000 * p, eng.q[:ells[1]], eng.N) for p in range(2)])
                qq = np.asarray(q2, dtype=np.uint64)[None, :, None]
                y[:, :2] = (qq - x[:, :2]) % qq if pattern == "negated" else x[:, :2]
            a.append(eng.ct_import(x))
            b.append(eng.ct_import(y))
            ka.append(k0s[(i + pi) % 3])
            kb.append(k0s[(i + pi + 1) % 3])
            sa = np.array([ka[-1] % int(m) for m in q2], dtype=np.uint64)
            sb = np.array([kb[-1] % int(m) for m in q2], dtype=np.uint64)
            want.append(np.stack([orc.add(orc.mul_scalar(x[c, :2], sa, q2), orc.mul(orc.mul_scalar(y[c, :2], sb, q2), mono, q2), q2)
                                  for c in range(2)]))
        got = eng.debug_pair_pack(a, b, ka, kb)
        for i in range(n_pairs):
            assert got[i].info()["ell"] == 2 and got[i].info()["deg"] == 2
            assert np.array_equal(got[i].export(), want[i]), (pattern, ells, i)


@pytest.mark.parametrize("n_pairs", [1, 3])
@pytest.mark.parametrize("ell", [1, 3, 7])
def test_split_kernel_crafted_residues(bare, orc, ell, n_pairs):
    """(w + wc, X^(N/2) (wc - w)) over all limbs, every pair in one launch"""
    eng = bare
    ql = eng.q[:ell]
    mono = _mono_i(orc, eng, ell)
    for pattern in PATTERNS:
        w, wc, want = [], [], []
        for i in range(n_pairs):
            x, y = _crafted(orc, eng, pattern, 21 + 3 * i, ell)
            w.append(eng.ct_import(x))
            wc.append(eng.ct_import(y))
            want.append((np.stack([orc.add(x[c], y[c], ql) for c in range(2)]),
                         np.stack([orc.mul(orc.sub(y[c], x[c], ql), mono, ql) for c in range(2)])))
        got_a, got_b = eng.debug_pair_split(w, wc)
        for i in range(n_pairs):
            assert np.array_equal(got_a[i].export(), want[i][0]), (pattern, ell, i, "a")
            assert np.array_equal(got_b[i].export(), want[i][1]), (pattern, ell, i, "b")
        if pattern == "negated":
            assert not got_a[0].export().any()
        if pattern == "equal":
            assert not got_b[0].export().any()


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------
def _code(fa, fn):
    with pytest.raises(fa.FhelinError) as e:
        fn()
    return e.value.code


def test_pair_refusals(fa, orc, bare, pair10):
    eng, boot, (ca, cb) = pair10["eng"], pair10["boot"], pair10["ct"]
    m = np.random.default_rng(1).uniform(-1, 1, boot.n // 2)
    half = eng.encrypt(m, level=eng.n_q - 3, slots=boot.n // 2)
    assert _code(fa, lambda: eng.bootstrap_pair(ca, half)) == ERR_ARG              # unequal slot counts
    one = eng.level_reduce(ca, 1)
    assert _code(fa, lambda: eng.bootstrap_pair(cb, one)) == ERR_STATE             # fewer than two limbs
    assert _code(fa, lambda: eng.bootstrap_pair_partial(ca, cb, 4)) == ERR_ARG
    # unequal slot counts in a batch are not an error: both run as singles
    before = eng.stats()["bootstrap"]
    outs = eng.bootstrap_paired_batch([ca, half])
    assert eng.stats()["bootstrap"] - before == 2
    assert np.array_equal(outs[0].export(), eng.bootstrap(ca).export())
    # bootstrapping not set up
    x = np.stack([orc.uniform_residues(3 + 1000 * p, bare.q[:3], bare.N) for p in range(2)])
    u, v = bare.ct_import(x), bare.ct_import(x)
    assert _code(fa, lambda: bare.bootstrap_pair(u, v)) == ERR_STATE
    assert _code(fa, lambda: bare.bootstrap_paired_batch([u, v])) == ERR_STATE
    # correction 0 leaves no bit for the split's 1/2
    e0 = fa.Engine("boot12", seed=77, log_slots=10)
    try:
        e0.keygen()
        e0.gen_relin_key()
        e0.bootstrap_config(correction=0)
        e0.bootstrap_setup(3, 3, 1 << 10)
        mm = np.random.default_rng(2).uniform(-1, 1, 1 << 10)
        p, q = e0.encrypt(mm, level=e0.n_q - 3), e0.encrypt(mm, level=e0.n_q - 3)
        assert _code(fa, lambda: e0.bootstrap_pair(p, q)) == ERR_STATE
    finally:
        e0.close()
