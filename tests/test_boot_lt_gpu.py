"""Bootstrap linear stages on the linear-transform engine (include/fhelin.h "Bootstrap linear stages"): with
Engine.set_bootstrap_lt on, every CoeffsToSlots / SlotsToCoeffs stage is ONE Evaluator::linear_transform_rows call, and the bootstrap must
equal - residues, limbs, noise degree, 80-bit scale - the stage-by-stage oracle (oracle/residue_boot.py) with its `apply` replaced by the
composition fhelin_lt_apply is pinned to:  rotate_each_sum([hoisted_dot(x, V_{g,.}, baby[1:]) for g in giant], giant), the plaintexts
over the full key basis at the stage's scale (the level's own, or the override after a ModRaise to fewer limbs).  Off is the parent's path."""
import numpy as np
import pytest

from test_boot_residue_gpu import _boot_input, _rev, _same

pytestmark = pytest.mark.gpu
LD = np.longdouble
ERR_ARG, ERR_STATE, ERR_KEY = 1, 4, 5
ABS_BOUND = 2e-4          # what tests/test_boot_residue_gpu.py asserts at N=2^12
HEADLINE_BOUND = 6.3e-5   # tests/test_bootstrap_gpu.py test_bootstrap_precision_at_the_headline_ring, the default path's bound at N=2^16


def _lt_bootstrapper(orc):
    from oracle.residue_boot import ResidueBootstrapper
    from oracle.residue_eval import RCt

    class LtResidueBootstrapper(ResidueBootstrapper):
        """Bootstrapper::apply with the knob on.  enc(pt)(ell, scale) must give the encoding over the FULL key basis (ell = n_q + n_p)."""

        def apply(self, stage, xin, ns):
            rev = self.rev
            x = rev.rescale(xin) if xin.deg >= 2 else xin
            lvl = rev.level(x)
            sf = rev.sf[lvl]
            if x.ell >= 2 and abs(x.scale / rev.sf[lvl] - LD(1)) > LD(1e-12):
                sf = rev.sf[lvl + 1] * LD(int(rev.q[x.ell - 1])) / x.scale      # the scale override (first stage after a ModRaise to fewer limbs)
            terms = stage["terms"]
            babies = sorted({b for (_, b, _) in terms} - {0})                    # the rotated baby steps that carry a term
            giants = sorted({g for (g, _, _) in terms})
            nl = len(rev.q) + len(rev.p)
            n_dig = -(-len(rev.q) // rev.alpha)
            evks = np.stack([rev.keys[b] for b in babies]) if babies else np.zeros((0, n_dig, 2, nl, self.N), dtype=np.uint64)
            gs = [orc.galois(rev.log_n, b) for b in babies]
            zero = np.zeros((nl, self.N), dtype=np.uint64)
            inner = []
            for g in giants:                                                     # ascending: the unrotated group first
                row = {b: pt for (gg, b, pt) in terms if gg == g}
                pts = np.stack([self.enc(row[b])(nl, sf) if b in row else zero for b in [0] + babies])
                d = orc.hoisted_dot(x.d, evks, gs, pts, rev.alpha, rev.q, rev.p, rev.psi_q, rev.psi_p)
                inner.append(RCt(d, x.deg + 1, x.scale * sf))
            del evks
            return self._rotate_each_sum(inner, giants, ns)

    return LtResidueBootstrapper


def _setup(fa, orc, preset, log_slots, knob=(True, 0), oracle=True, **over):
    """engine with real keys and bootstrapping set up under `knob` (None: never touched); the oracle-side bootstrapper (the subclass
    when the knob is on, the parent's otherwise)"""
    from oracle.residue_boot import ResidueBootstrapper
    eng = fa.Engine(preset, seed=77, log_slots=log_slots, **over)
    eng.keygen()
    eng.gen_relin_key()
    if knob is not None:
        eng.set_bootstrap_lt(*knob)
    eng.bootstrap_setup(3, 3, 1 << log_slots)
    desc = eng.bootstrap_describe()
    if not oracle:
        return eng, desc
    keys = {"relin": eng.key_export(0), "conj": eng.key_export(2)}
    for r in _key_list(eng, desc):
        keys[r] = eng.key_export(1, r)
    cls = _lt_bootstrapper(orc) if desc["lt"] else ResidueBootstrapper
    return eng, cls(_rev(eng, keys), desc, lambda pt: (lambda ell, sc: eng.pt_export(pt, ell, sc)))


def _key_list(eng, desc):
    """the rotation indices the bootstrap needs: every stage term's giant and baby step, and SubSum's"""
    need = set()
    for st in desc["c2s"] + desc["s2c"]:
        for (g, b, _) in st["terms"]:
            need.update((g, b))
    j = 1
    while j < (eng.N // 2) // desc["slots"]:
        need.add(desc["slots"] * j)
        j <<= 1
    return sorted(need - {0})


def _split(desc):
    return [(st["n1"], st["n2"]) for st in desc["c2s"] + desc["s2c"]]


@pytest.fixture(scope="module")
def boots(fa, orc):
    """(engine, oracle bootstrapper) with the knob on and the planner's split, per log_slots, made once for the module"""
    made = {}

    def get(log_slots):
        if log_slots not in made:
            made[log_slots] = _setup(fa, orc, "boot12", log_slots)
        return made[log_slots]

    yield get
    for eng, _ in made.values():
        eng.close()


# ---- 1. stage by stage, bit for bit ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log_slots", [10, 11])     # 10: sparse packing (SubSum, packed last C2S / first S2C over 2n slots); 11: full
def test_bootstrap_lt_bit_exact_stage_by_stage(boots, fa, orc, log_slots):
    eng, boot = boots(log_slots)
    assert boot.desc["lt"] and boot.desc["lt_n1"] == 0 and eng.bootstrap_lt() == (True, 0)
    assert boot.desc["packed"] == (log_slots == 10)
    for st in boot.desc["c2s"] + boot.desc["s2c"]:
        assert 1 <= st["n1"] <= 32 and st["n2"] == len({g for (g, _, _) in st["terms"]})
    m, ct, r = _boot_input(eng, boot)
    for stage in (1, 2, 3):
        got, want = eng.bootstrap_partial(ct, stage), boot.run(r, stop_after=stage)
        assert np.array_equal(got.export(), want.d), ("stage", stage)
        if stage == 2:
            c2s_on = want.d
    out, want = eng.bootstrap(ct), boot.run(r)
    _same(out, want, "bootstrap, linear stages on the engine")
    err = np.max(np.abs(eng.decrypt(out) - m))
    print(f"log_slots {log_slots}: knob-on bootstrap max error {err:.3e}")
    assert err < ABS_BOUND
    if log_slots == 10:
        # not vacuous: the default path's composition (products after the baby steps' ModDowns) on the SAME split and keys gives other
        # residues - the knob changes roundings, and the subclass is what pins them
        from oracle.residue_boot import ResidueBootstrapper
        parent = ResidueBootstrapper(boot.rev, boot.desc, boot.enc)
        other = parent.run(r, stop_after=2)
        assert other.d.shape == c2s_on.shape and not np.array_equal(other.d, c2s_on)


# ---- 2. every kernel shape, through CoeffsToSlots -------------------------------------------------------------------------------------
# forced n1 at 1024 slots -> (n1, n2) of the three CoeffsToSlots stages (8, 15 and 31 diagonals; the first stage's indices are the 8
# multiples of 128, which caps its n1), as tools/boot_lt_split_check.cpp prints them:
#   4: ks_inner_dot_kernel<2>, <4>, and two launches of <4>; 16 and 32: <1> and <2>, with 15 and 30 rotated baby steps in one launch;
#   2 (beyond the three above): 16 groups = four launches of <4>, and 15 rotated giant steps = three shared ModDowns
C2S_SPLITS = {
    2: [(2, 4), (2, 8), (2, 16)],
    4: [(4, 2), (4, 4), (4, 8)],
    16: [(8, 1), (16, 2), (16, 2)],
    32: [(8, 1), (32, 2), (32, 2)],
}


@pytest.mark.parametrize("n1", [4, 16, 32, 2])
def test_every_kernel_shape_through_coeffs_to_slots(fa, orc, n1):
    eng, boot = _setup(fa, orc, "boot12", 10, knob=(True, n1))
    try:
        assert boot.desc["lt_n1"] == n1 and eng.bootstrap_lt() == (True, n1)
        assert _split(boot.desc)[:3] == C2S_SPLITS[n1], _split(boot.desc)
        if n1 == 32:     # 15 + 15 rotated baby steps in the packed stage's one launch
            assert len({b for (_, b, _) in boot.desc["c2s"][2]["terms"]} - {0}) == 30
        m, ct, r = _boot_input(eng, boot)
        got, want = eng.bootstrap_partial(ct, 2), boot.run(r, stop_after=2)
        assert np.array_equal(got.export(), want.d), n1
    finally:
        eng.close()


# ---- 3. drop and level plan: the scale override ----------------------------------------------------------------------------------------
def test_bootstrap_lt_to_fewer_limbs_bit_exact(boots):
    eng, boot = boots(10)
    m, ct, r = _boot_input(eng, boot, ell_left=2, seed=5)
    full = eng.n_q - boot.desc["depth"]
    for drop in (2, 4):
        want = boot.run(r, drop=drop)
        assert want.ell == full - drop
        _same(eng.bootstrap_drop(ct, drop), want, ("drop", drop))
    eng.set_level_plan([full - 4])
    eng.level_plan_begin("apply")
    try:
        out = eng.bootstrap(ct)
    finally:
        eng.level_plan_begin("off")
    _same(out, want, "planned bootstrap")
    assert np.max(np.abs(eng.decrypt(out) - m)) < ABS_BOUND


# ---- 4. batch, pair, iterative ----------------------------------------------------------------------------------------------------------
def test_batch_pair_and_iterative_with_the_knob_on(boots):
    eng, boot = boots(10)
    ins = [_boot_input(eng, boot, ell_left=k, seed=20 + k) for k in (3, 4, 2)]
    singles = [eng.bootstrap(c) for _, c, _ in ins]
    for s, b in zip(singles, eng.bootstrap_batch([c for _, c, _ in ins])):
        assert np.array_equal(s.export(), b.export()) and s.info() == b.info() and s.scale_parts() == b.scale_parts()
    # a pair through one pipeline: the batch entry equals the single pair call, and both halves decrypt
    (ma, ca, _), (mb, cb, _) = ins[0], ins[1]
    pa, pb = eng.bootstrap_pair(ca, cb)
    out = eng.bootstrap_paired_batch([ca, cb])
    for o, p in zip(out, (pa, pb)):
        assert np.array_equal(o.export(), p.export()) and o.info() == p.info() and o.scale_parts() == p.scale_parts()
    ea, eb = np.max(np.abs(eng.decrypt(out[0]) - ma)), np.max(np.abs(eng.decrypt(out[1]) - mb))
    print(f"knob-on pair error a {ea:.3e} b {eb:.3e}")
    assert ea < ABS_BOUND and eb < ABS_BOUND
    # iterative: the batch equals the singles; it decrypts within the single bootstrap's bound
    it = [eng.bootstrap_iter(c, 12) for _, c, _ in ins[:2]]
    for s, b in zip(it, eng.bootstrap_iter_batch([c for _, c, _ in ins[:2]], 12)):
        assert np.array_equal(s.export(), b.export()) and s.info() == b.info() and s.scale_parts() == b.scale_parts()
    ei = np.max(np.abs(eng.decrypt(it[0]) - ma))
    print(f"knob-on iterative error {ei:.3e}")
    assert ei < ABS_BOUND


# ---- 5. off is the parent ---------------------------------------------------------------------------------------------------------------
def test_off_is_the_default_path(boots, fa, orc):
    from test_evalkeys_gpu import move
    never, boot_never = _setup(fa, orc, "boot12", 10, knob=None)
    off, d_off = _setup(fa, orc, "boot12", 10, knob=(False, 0), oracle=False)
    try:
        d_never = boot_never.desc
        assert never.bootstrap_lt() == off.bootstrap_lt() == (False, 0)
        plain = lambda d: {k: ([dict(slots=s["slots"], terms=[t[:2] for t in s["terms"]]) for s in v] if k in ("c2s", "s2c") else v)
                           for k, v in d.items()}
        assert plain(d_never) == plain(d_off) and not d_never["lt"] and "n1" not in d_never["c2s"][0] and "encoding_bytes" not in d_never
        assert _key_list(never, d_never) == _key_list(off, d_off)
        m, ct, r = _boot_input(never, boot_never)
        a = never.bootstrap(ct)
        b = off.bootstrap(move(ct, off))                     # the same test seed: the two contexts hold the same keys
        assert np.array_equal(a.export(), b.export()) and a.info() == b.info() and a.scale_parts() == b.scale_parts()
        _same(a, boot_never.run(r), "the default path is the oracle's default composition")
        # the knob-on key list is another list: the planner's 8 baby steps per stage against the default 4 / 8 x 4
        on_eng, on_boot = boots(10)
        on_keys = _key_list(on_eng, on_boot.desc)
        assert on_keys != _key_list(never, d_never)
        assert _split(on_boot.desc) == [(8, 1), (8, 2), (8, 4), (8, 4), (8, 2), (8, 2)]
        assert set(_key_list(never, d_never)) - set(on_keys), "the default split needs no key the engine's split lacks"
    finally:
        never.close()
        off.close()


# ---- 6. keys and refusals ---------------------------------------------------------------------------------------------------------------
def test_evaluation_context_keys_and_refusals(boots, fa, orc, tmp_path, monkeypatch):
    from test_evalkeys_gpu import _code, move
    from test_keycaps_gpu import _g
    monkeypatch.delenv("FHELIN_BOOT_LT", raising=False)
    monkeypatch.delenv("FHELIN_BOOT_LT_N1", raising=False)
    eng, boot = boots(10)
    path = str(tmp_path / "lt.evk")
    eng.save_eval_keys(path)
    m, ct, r = _boot_input(eng, boot)
    want = eng.bootstrap(ct)
    # the same set under the default split misses a key of that split: named at bootstrap_setup
    code, msg = _code(fa, fa.Engine.from_eval_keys, path, 0, 4)
    assert code == ERR_KEY and "rotation key for index" in msg
    monkeypatch.setenv("FHELIN_BOOT_LT", "1")
    ev = fa.Engine.from_eval_keys(path, seed=4)
    monkeypatch.delenv("FHELIN_BOOT_LT")
    try:
        assert ev.bootstrap_lt() == (True, 0) and _split(ev.bootstrap_describe()) == _split(boot.desc)
        got = ev.bootstrap(move(ct, ev))
        assert np.array_equal(got.export(), want.export()) and got.scale_parts() == want.scale_parts()
        # the knob binds at setup; a bad n1 is refused whenever it is asked
        assert _code(fa, ev.set_bootstrap_lt, False)[0] == ERR_STATE
        assert _code(fa, eng.set_bootstrap_lt, True, 4)[0] == ERR_STATE
        assert ev.bootstrap_lt() == (True, 0)
    finally:
        ev.close()
    fresh = fa.Engine("boot12", seed=1, log_slots=10)
    try:
        for bad in (-1, 33):
            assert _code(fa, fresh.set_bootstrap_lt, True, bad)[0] == ERR_ARG
        assert fresh.bootstrap_lt() == (False, 0)
    finally:
        fresh.close()
    # a rotation key capped below the limbs of the stage that uses it: refused by name before the stage launches anything
    capped = fa.Engine("boot12", seed=77, log_slots=10)
    try:
        idx = boot.desc["c2s"][0]["terms"][1][1]          # the first rotated baby step of the first CoeffsToSlots stage
        assert idx > 0
        capped.set_key_caps([(2, _g(capped, idx), 5)])
        capped.keygen()
        capped.gen_relin_key()
        capped.set_bootstrap_lt(True)
        capped.bootstrap_setup(3, 3, 1 << 10)
        x = capped.encrypt(m, level=capped.n_q - 3)
        before = capped.stats()["keyswitch"]
        code, msg = _code(fa, capped.bootstrap_drop, x, 0)     # the immediate entry point: fhelin_bootstrap may defer, and refuse at the read
        assert code == ERR_KEY and "capped at 5 limbs" in msg and f"index {idx} (Galois element {_g(capped, idx)})" in msg, msg
        assert capped.stats()["keyswitch"] - before == 1   # SubSum's one rotation ran; the stage did not start
    finally:
        capped.close()


# ---- 7. limb-sliced encodings -----------------------------------------------------------------------------------------------------------
def test_stage_encodings_are_limb_sliced(fa, orc):
    eng, desc = _setup(fa, orc, "boot12", 10, oracle=False)
    try:
        assert desc["encoding_bytes"] == 0
        m = np.random.default_rng(3).uniform(-1, 1, 1 << 10)
        eng.bootstrap_drop(eng.encrypt(m, level=eng.n_q - 3), 0)     # the immediate entry point (fhelin_bootstrap may defer until read)
        k, N, n_q = eng.n_p, eng.N, eng.n_q
        # one (limbs, scale) per stage so far: CoeffsToSlots from the top of the chain, one limb per stage; SlotsToCoeffs after EvalMod
        depth = desc["depth"]
        ells = [n_q, n_q - 1, n_q - 2] + [n_q - depth + 3 - i for i in range(3)]
        want = sum(len(st["terms"]) * (ell + k) * N * 8 for st, ell in zip(desc["c2s"] + desc["s2c"], ells))
        got = eng.bootstrap_describe()["encoding_bytes"]
        n_terms = sum(len(st["terms"]) for st in desc["c2s"] + desc["s2c"])
        print(f"stage encodings: {got} bytes sliced, {n_terms * (n_q + k) * N * 8} over the full basis")
        assert got == want
        assert got < n_terms * (n_q + k) * N * 8
        # a second bootstrap to fewer limbs applies every term at another (limbs, scale): as many encodings again, each 2 rows shorter
        eng.bootstrap_drop(eng.encrypt(m, level=eng.n_q - 3), 2)
        want2 = want + sum(len(st["terms"]) * (ell - 2 + k) * N * 8 for st, ell in zip(desc["c2s"] + desc["s2c"], ells))
        assert eng.bootstrap_describe()["encoding_bytes"] == want2
    finally:
        eng.close()


def test_plan_encoding_bytes(engine_factory, orc):
    from test_default_path_gpu import _ct
    from test_linear_transform_gpu import _oracle_keys, _terms
    eng = engine_factory("toy13")
    n1, n2 = 4, 2
    baby, giant = list(range(n1)), [0, n1]
    _oracle_keys(orc, eng, baby[1:] + giant[1:])
    pts, _ = _terms(eng, n1, n2, {(1, 2)}, seed=5)
    lt = eng.lt_create_pts(pts, baby, giant)
    assert lt.encoding_bytes() == 0
    terms, k, N = n1 * n2 - 1, eng.n_p, eng.N
    for i, ell in enumerate((7, 4)):
        eng.lt_apply(lt, [eng.ct_import(_ct(orc, eng, 50 + ell, ell))])
        eng.lt_apply(lt, [eng.ct_import(_ct(orc, eng, 60 + ell, ell))])     # the same (limbs, scale) again: nothing new
        assert lt.encoding_bytes() == terms * N * 8 * sum(e + k for e in (7, 4)[:i + 1])
    assert lt.encoding_bytes() < 2 * terms * (eng.n_q + k) * N * 8


# ---- 8. the headline ring ---------------------------------------------------------------------------------------------------------------
def test_bootstrap_lt_bit_exact_headline_ring_under_a_level_plan(fa, orc):
    """N=2^16, 28+7 limbs, alpha=7, 16384 slots (sparse packing), drop 4, planner split - the chain and the drop of the forward pass's GELU
    bootstraps.  Measured maximum decryption error: see DESIGN.md 7t."""
    eng, boot = _setup(fa, orc, "bench", 14, n_q=28, n_p=-1)
    try:
        assert boot.desc["packed"] and boot.desc["lt"] and eng.alpha == 7 and eng.n_p == 7
        print("headline split (n1, n2) per stage:", _split(boot.desc))
        m, ct, r = _boot_input(eng, boot, ell_left=2)
        out, want = eng.bootstrap_drop(ct, 4), boot.run(r, drop=4)
        assert want.ell == 28 - boot.desc["depth"] - 4 == 9
        _same(out, want, "bootstrap on the engine, headline ring, drop 4")
        err = np.max(np.abs(eng.decrypt(out) - m))
        print(f"knob-on bootstrap max error at N=2^16, 28+7 limbs, drop 4: {err:.3e} (asserted < {HEADLINE_BOUND})")
        assert err < HEADLINE_BOUND
    finally:
        eng.close()
