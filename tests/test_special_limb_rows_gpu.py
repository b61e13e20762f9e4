"""Special-limb inner products formed in the inverse NTT's row pass (FHELIN_FUSE_ACCP_ROWS): the inner-product launches of
a key switch cover the Q limbs only, ntt_rows_product_kernel forms the special-limb sums in its load stage and the ModDown starts at the
column pass.  Residues do not change, so every check is an equality, taken two ways: against the oracle, and against an engine created
with FHELIN_FUSE_ACCP_ROWS=0 (the separate launches) that holds the same keys.

Shapes: N = 2^12 (one row tile per vector) and 2^13 (two: every stream's tile offset counts), one case at N = 2^16 for the A = 8 column
pass; ell = 1, 2, alpha, alpha + 1 and the full chain (one digit, a short last digit, two digits with a one-limb second one); a 52-bit
special-prime chain for the lazy butterfly class.  The crafted cases reach the kernel's operands directly (fhelin_debug_ks_accp): every
digit and key residue at its maximum, so that the 128-bit sums stand at their fold bound, an all-zero digit under a maximal key, and
uniform digits against sums formed by the oracle's dyadic functions."""
import numpy as np
import pytest

from test_default_path_gpu import _ct, _evk, _imp, _rev, _same

pytestmark = pytest.mark.gpu
LD = np.longdouble
KNOB = "FHELIN_FUSE_ACCP_ROWS"
ROTS = [1, 2, 3, 4, 5, 6, 7, 64, 128, 192, -1, -2]     # 64 k: every 512-coefficient tile stays in place at both small rings
# name -> (preset, overrides, levels): alpha = 2 / 3 / 3 / 2
RINGS = {"n12": ("toy", {}, [1, 2, 3, 6]),
         "n13": ("toy13", {}, [1, 2, 3, 4, 7]),
         "n13_lazy": ("toy13", {"special_bits": 52}, [2, 4, 7]),
         "n16": ("bench", {"n_q": 4, "n_p": 2, "dnum": 2}, [2])}
_PAIRS = {}


def _engine(fa, on, preset, **kw):
    """on: every operand form through the row pass (2: the merged sums too, which the default leaves on their own kernel)"""
    mp = pytest.MonkeyPatch()
    try:
        mp.setenv(KNOB, "2" if on else "0")
        mp.setenv("FHELIN_ACCP_ROWS_MIN_VECS", "0")
        return fa.Engine(preset, **kw)
    finally:
        mp.undo()


@pytest.fixture(scope="module")
def pairs(fa, orc):
    """get(name) -> (engine with the fused row pass, engine with the separate launches, rotation keys, relinearisation key, ResidueEvaluator):
    the same uniform 'keys' in both (parity of integer functions needs no real keys), made once per ring"""
    def get(name):
        if name not in _PAIRS:
            preset, over, _ = RINGS[name]
            on, off = _engine(fa, True, preset, **over), _engine(fa, False, preset, **over)
            idx = ROTS if name != "n16" else [1, 2, 3]
            keys = {r: _evk(orc, on, 9000 + 17 * (r % 100003)) for r in idx}
            relin = _evk(orc, on, 31)
            for e in (on, off):
                e.key_import(0, 0, relin)
                for r, k in keys.items():
                    e.key_import(1, r, k)
            _PAIRS[name] = (on, off, keys, relin, _rev(orc, on, keys))
        return _PAIRS[name]
    yield get
    for on, off, *_ in _PAIRS.values():
        on.close()
        off.close()
    _PAIRS.clear()


def _eq(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes(), what


def _cases(names):
    return [(n, ell) for n in names for ell in RINGS[n][2]]


def _limb_transforms(e, fn):
    e.stats(reset=True)
    fn()
    e.sync()
    return e.stats()["limb_ntt"]


@pytest.mark.parametrize("name,ell", _cases(["n12", "n13", "n13_lazy", "n16"]))
def test_relinearisation(pairs, orc, name, ell):
    """the identity form (ks_inner_kernel<false>'s operands: keys as stored, digits times 2^64), one ciphertext and a batch of three"""
    on, off, keys, relin, rev = pairs(name)
    a = [_ct(orc, on, 900 + 7 * i + ell, ell) for i in range(3)]
    b = [_ct(orc, on, 950 + 7 * i + ell, ell) for i in range(3)]
    want = [orc.mult_relin(x, y, relin, on.alpha, on.q, on.p, on.psi_q, on.psi_p) for x, y in zip(a, b)]
    for e in (on, off):
        _eq(e.raw_mult_relin(e.ct_import(a[0]), e.ct_import(b[0])).export(), want[0], (name, ell, e is on, "one"))
        got = e.mult_batch([_imp(e, rev, x)[0] for x in a], [_imp(e, rev, y)[0] for y in b])
        for i, g in enumerate(got):
            _eq(g.export(), want[i], (name, ell, e is on, "batch of 3", i))
    # the counters keep their meaning: the fused row pass still counts its limb transforms
    n_on = _limb_transforms(on, lambda: on.raw_mult_relin(on.ct_import(a[0]), on.ct_import(b[0])))
    n_off = _limb_transforms(off, lambda: off.raw_mult_relin(off.ct_import(a[0]), off.ct_import(b[0])))
    assert n_on == n_off and n_on > 0, (n_on, n_off)


@pytest.mark.parametrize("name,ell", _cases(["n12", "n13", "n13_lazy", "n16"]))
def test_plain_rotations(pairs, orc, name, ell):
    """gathered (ks_inner_kernel<true>'s operands: the row's map, the permuted pre-split key): an index that moves the 512-coefficient
    tiles, one that keeps them in place, a negative one; one ciphertext and a batch of three"""
    on, off, keys, relin, rev = pairs(name)
    rots = [1, 64, -1] if name != "n16" else [1]
    xs = [_ct(orc, on, 300 + 7 * i + ell, ell) for i in range(3)]
    for r in rots:
        want = [orc.rotate(x, keys[r], orc.galois(on.log_n, r), on.alpha, on.q, on.p, on.psi_q, on.psi_p) for x in xs]
        for e in (on, off):
            _eq(e.raw_rotate(e.ct_import(xs[0]), r).export(), want[0], (name, ell, r, e is on, "one"))
            for i, g in enumerate(e.rotate_batch([e.ct_import(x) for x in xs], r)):
                _eq(g.export(), want[i], (name, ell, r, e is on, "batch of 3", i))


@pytest.mark.parametrize("name,ell", _cases(["n12", "n13"]))
def test_rows_with_their_own_keys(pairs, orc, name, ell):
    """per-row keys and maps over a shared input: rotate_many with 1, 2 and 7 indices, and two inputs in one launch (row_mod)"""
    on, off, keys, relin, rev = pairs(name)
    xs = [_ct(orc, on, 410 + 3 * i + ell, ell) for i in range(2)]
    want = {(i, r): orc.rotate(xs[i], keys[r], orc.galois(on.log_n, r), on.alpha, on.q, on.p, on.psi_q, on.psi_p)
            for i in range(2) for r in range(1, 8) if i == 0 or r in (2, 5)}
    for e in (on, off):
        for idx in ([3], [1, 2], [1, 2, 3, 4, 5, 6, 7]):
            for r, g in zip(idx, e.rotate_many(e.ct_import(xs[0]), idx)):
                _eq(g.export(), want[0, r], (name, ell, e is on, "rotate_many", len(idx), r))
        cs = [_imp(e, rev, x)[0] for x in xs]
        for i, outs in enumerate(e.debug_rotate_many_batch(cs, [2, 5])):
            for r, g in zip([2, 5], outs):
                _eq(g.export(), want[i, r], (name, ell, e is on, "two inputs", i, r))


MERGED = {"R1": [-2], "R3": [1, 2, 3], "R3_in_place": [64, 128, 192], "R7": [1, 2, 3, 4, 5, 6, 7]}


@pytest.mark.parametrize("name,ell,rots", [(n, ell, k) for n, ell in _cases(["n12", "n13"]) + [("n13_lazy", 7)] for k in MERGED]
                         + [("n16", 2, "R3")])
def test_merged_rotation_sums(pairs, orc, name, ell, rots):
    """ks_inner_multi_kernel's operands: 1, 3 and 7 merged rotations with and without the LDS digit stage on the Q side, 1, 2 and 3 rows
    (an odd count leaves the row-pair kernel's partner switched off while the product pass still takes every row)"""
    on, off, keys, relin, rev = pairs(name)
    idx = MERGED[rots]
    evks = np.stack([keys[r] for r in idx])
    gs = [orc.galois(on.log_n, r) for r in idx]
    xs = [_ct(orc, on, 300 + 7 * i + ell, ell) for i in range(3)]
    want = [orc.rotate_sum(x, evks, gs, on.alpha, on.q, on.p, on.psi_q, on.psi_p) for x in xs]
    for e in (on, off):
        for rows in (1, 2, 3):
            for i, g in enumerate(e.rotate_sum([e.ct_import(x) for x in xs[:rows]], idx)):
                _eq(g.export(), want[i], (name, ell, idx, e is on, rows, i))


@pytest.mark.parametrize("name,ell", [("n12", 3), ("n13", 4), ("n13", 7)])
def test_sums_of_rotations_of_different_inputs(pairs, orc, name, ell):
    """rotate_each_sum: every rotation on its own input (rot_ext_stride / rot_input_stride), 2 and 7 terms"""
    on, off, keys, relin, rev = pairs(name)
    for idx in ([1, 2], [1, 2, 3, 4, 5, 6, 7]):
        xs = [_ct(orc, on, 800 + 3 * i + ell, ell) for i in range(len(idx))]
        want = rev.rotate_each_sum([_imp(on, rev, x)[1] for x in xs], idx)
        for e in (on, off):
            _same(e.rotate_each_sum([_imp(e, rev, x)[0] for x in xs], idx), want, (name, ell, len(idx), e is on))


@pytest.mark.parametrize("name,ell", [("n12", 3), ("n12", 6), ("n13", 4), ("n13", 7)])
def test_merged_moddown_and_rescale(pairs, orc, name, ell):
    """hoisted_dot: folded keys in the merged form; rescale=True ends in moddown_rescale, whose special limbs arrive row-transformed too"""
    on, off, keys, relin, rev = pairs(name)
    idx = [1, 2, 3]
    rng = np.random.default_rng(77)
    vals = [rng.uniform(-1, 1, 1 << on.params.log_slots) for _ in range(len(idx) + 1)]
    pts0 = [on.encode(v) for v in vals]
    encs = [(lambda p: (lambda l, sc: on.pt_export(p, l, sc)))(p) for p in pts0]
    xs = [_ct(orc, on, 500 + 7 * i + ell, ell) for i in range(2)]
    for rescale in (False, True):
        want = [rev.hoisted_dot(_imp(on, rev, x)[1], encs, idx, rescale=rescale) for x in xs]
        for e in (on, off):
            pts = [e.encode(v) for v in vals]
            for g, w in zip(e.hoisted_dot([_imp(e, rev, x)[0] for x in xs], pts, idx, rescale=rescale), want):
                _same(g, w, (name, ell, rescale, e is on))


# ------------------------------------------------------------------------------------------------ crafted operands, at the kernel
def _accp_want(orc, e, ell, digits, key_sets, gs):
    """INTT over the special limbs of sum_r sigma_r(sum_j d_j * key_{r,j,c}) from the oracle's dyadic functions (canonical digits);
    gs = None: the identity form over one key, whose sum comes times 2^-64"""
    K, L1 = e.n_p, e.n_q
    p = [int(v) for v in e.p]
    out = np.empty((digits.shape[0], 2, K, e.N), dtype=np.uint64)
    for b in range(digits.shape[0]):
        for c in range(2):
            acc = np.zeros((K, e.N), dtype=np.uint64)
            for r, key in enumerate(key_sets):
                beta = digits.shape[1]
                s = orc.dot([digits[b, j, ell:] for j in range(beta)], [key[j, c, L1:] for j in range(beta)], p)
                if gs is not None:
                    s = np.stack([orc.automorph_ntt(s[i], gs[r]) for i in range(K)])
                acc = orc.add(acc, s, p)
            if gs is None:
                acc = orc.mul_scalar(acc, np.array([pow(1 << 64, -1, m) for m in p], dtype=np.uint64), p)
            out[b, c] = orc.ntt_batch(acc, p, e.psi_p, inverse=True)
    return out


@pytest.mark.parametrize("name,ell,idx,batch", [
    ("n12", 6, [], 1), ("n12", 3, [], 2), ("n13", 7, [], 1), ("n13", 4, [1, 64, -1], 2), ("n13", 7, [1, 2, 3, 4, 5, 6, 7], 3),
    ("n13_lazy", 7, [], 1), ("n13_lazy", 7, [1, 2, 3, 4, 5, 6, 7], 1), ("n16", 2, [], 1), ("n16", 2, [1, 2, 3], 1)])
def test_uniform_digits_at_the_kernel(pairs, orc, name, ell, idx, batch):
    """the product pass on digits of the caller's choice: uniform canonical digits against the oracle's sums, both forms"""
    on, off, keys, relin, rev = pairs(name)
    beta, nt = -(-ell // on.alpha), ell + on.n_p
    mods = np.concatenate([np.asarray(on.q[:ell], dtype=np.uint64), np.asarray(on.p, dtype=np.uint64)])
    d = np.stack([orc.uniform_residues(5000 + 13 * i, mods, on.N) for i in range(batch * beta)]).reshape(batch, beta, nt, on.N)
    want = _accp_want(orc, on, ell, d, [keys[r] for r in idx] if idx else [relin], [orc.galois(on.log_n, r) for r in idx] if idx else None)
    for e in (on, off):
        _eq(e.debug_ks_accp(d, ell, idx), want, (name, ell, idx, e is on))


@pytest.mark.parametrize("name,ell,idx", [("n13", 7, []), ("n13", 7, [1, 2, 3, 4, 5, 6, 7]), ("n13", 1, [1, 2, 3, 4, 5, 6, 7]),
                                          ("n13_lazy", 7, []), ("n13_lazy", 7, [1, 2, 3, 4, 5, 6, 7]), ("n12", 6, [1, 2, 3])])
def test_maximal_operands_reach_the_fold_bound(fa, orc, pairs, name, ell, idx):
    """every key residue m - 1 on every limb and every digit at the largest value its class hands over: q - 1, or 86q - 1 where the lazy
    forward transform leaves digits unreduced (q < 2^53).  3, 7, 9 and 21 terms: below the flush at 8, past it, and past the fold at 16.
    Then the all-zero digit under the same maximal key.  Expected: the constant vector n_terms * d * (m - 1) [* 2^-64] mod m, transformed."""
    preset, over, _ = RINGS[name]
    on, off = _engine(fa, True, preset, **over), _engine(fa, False, preset, **over)
    try:
        beta, nt = -(-ell // on.alpha), ell + on.n_p
        mods = [int(v) for v in on.moduli]
        top = np.stack([np.full(on.N, m - 1, dtype=np.uint64) for m in mods])
        key = np.broadcast_to(top, (on.dnum_digits, 2) + top.shape).copy()
        for e in (on, off):
            e.key_import(0, 0, key)
            for r in idx:
                e.key_import(1, r, key)
        p = [int(v) for v in on.p]
        dmax = [(86 * m if m < (1 << 53) else m) - 1 for m in p]
        terms = beta * max(1, len(idx))
        for zero in (False, True):
            d = np.zeros((1, beta, nt, on.N), dtype=np.uint64)
            if not zero:
                for i, v in enumerate(dmax):
                    d[:, :, ell + i, :] = v
            const = [0 if zero else terms * dmax[i] * (m - 1) * (1 if idx else pow(1 << 64, -1, m)) % m for i, m in enumerate(p)]
            eva = np.stack([np.full(on.N, v, dtype=np.uint64) for v in const])
            want = orc.ntt_batch(eva, p, on.psi_p, inverse=True)
            for e in (on, off):
                got = e.debug_ks_accp(d, ell, idx)
                for c in range(2):
                    _eq(got[0, c], want, (name, ell, idx, zero, e is on, c))
    finally:
        on.close()
        off.close()


# ------------------------------------------------------------------------------------------------ what pool memory held before
@pytest.fixture(scope="module")
def trios(fa):
    import stale_memory
    mp = pytest.MonkeyPatch()
    mp.setenv(KNOB, "2")
    mp.setenv("FHELIN_ACCP_ROWS_MIN_VECS", "0")
    try:
        yield from stale_memory.make_trios(fa)
    finally:
        mp.undo()


def test_no_result_depends_on_stale_memory(trios, orc):
    """the pool's fill knob off, 1 and 2: the product pass writes every word of accP that the column pass reads (two row tiles, a
    relinearisation, a gathered rotation, a merged sum of an odd row count)"""
    from stale_memory import keys_for, relin_for, run

    def scen(s):
        eng = s.eng
        keys = keys_for(s, [1, 2, 3], 9000)
        relin = relin_for(s)
        rev = s.rev(keys)
        ell = 4
        a, b = _ct(s.orc, eng, s.seed(900), ell), _ct(s.orc, eng, s.seed(950), ell)
        s.out("mult", eng.mult(s.operand(eng.ct_import(a)), s.operand(eng.ct_import(b))),
              lambda: s.orc.mult_relin(a, b, relin, eng.alpha, eng.q, eng.p, eng.psi_q, eng.psi_p))
        c, x = s.imp(rev, _ct(s.orc, eng, s.seed(300), ell))
        s.out("rotate", eng.rotate(c, 1), lambda: rev.rotate(x, 1))
        xs = [_ct(s.orc, eng, s.seed(310 + 7 * i), ell) for i in range(3)]
        evks = np.stack([keys[r] for r in (1, 2, 3)])
        gs = [s.orc.galois(eng.log_n, r) for r in (1, 2, 3)]
        for i, (xx, g) in enumerate(zip(xs, eng.rotate_sum([s.operand(eng.ct_import(v)) for v in xs], [1, 2, 3]))):
            s.out(f"rotate_sum row {i}", g, lambda xx=xx: s.orc.rotate_sum(xx, evks, gs, eng.alpha, eng.q, eng.p, eng.psi_q, eng.psi_p))
    run(trios("toy13"), orc, scen)


# ------------------------------------------------------------------------------------------------ the conjugation key, through a bootstrap
def test_bootstrap_agrees_with_the_separate_launches(fa):
    """one bootstrap at N = 2^12 with real keys: baby steps (rows with their own keys), giant steps (merged sums over their own inputs),
    the conjugation key's gathered switch, EvalMod's relinearisations with both tails - byte for byte on both engines"""
    es = []
    try:
        for on in (True, False):
            e = _engine(fa, on, "boot12", seed=99, log_slots=10)
            e.keygen()
            e.gen_relin_key()
            e.bootstrap_setup(3, 3, 1 << 10)
            es.append(e)
        e0 = es[0]
        m = np.random.default_rng(3).uniform(-1, 1, 1 << 10)
        ct = e0.encrypt(m, level=e0.n_q - 3)
        x, inf, (hi, lo) = ct.export(), ct.info(), ct.scale_parts()
        outs = [e.bootstrap(e.ct_import(x, deg=inf["deg"], scale=float(LD(hi) + LD(lo)))) for e in es]
        _eq(outs[0].export(), outs[1].export(), "bootstrap")
        assert np.max(np.abs(e0.decrypt(outs[0]) - m)) < 2e-4
    finally:
        for e in es:
            e.close()
