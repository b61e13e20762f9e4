"""The kernels added since tests/test_param_corners_gpu.py, at the parameter corners Context accepts - byte for byte against the oracle
(oracle/fhe_oracle.c through oracle/residue_eval.py), and where the library has two paths, both against the oracle and each other.

  1. ks_inner_dot_kernel<1 / 2 / 4> (fhelin_lt_apply): its Acc30 sums are flushed per group of 8 digits and its group sums hold up to 32
     products.  Corners with alpha = 1..16, beta = 1..16, k = 1..16 and 24..60-bit primes; then 32 steps over 60-bit residues and 16
     digits at their maximum.
  2. moddown_rescale_exact_conv_kernel<1..8, 16> and affine_acc_items_kernel (the exact merged tail of mult_affine_batch): one
     instantiation per k, a guarded body for k = 9..15, the centring comparison of x_top and the lift through qlm where q_top >= 2 q_t.
     Three ways: the library as built, the library with FHELIN_EXACT_PRODUCTS=0, the oracle.
  3. product_sums<4, false, OWN> (kernels_ntt.hip): the row-pass product stages for sums of more than 8 terms - a flush every 8 terms, a
     fold every 16 - on the Q-limb side (OWN) and on the special-limb side with a single key as stored (khi = 30), and the 8-term SHORT
     variant holding eight products of 60-bit residues.  Engines with FHELIN_FUSE_ACCP_ROWS=2 / FHELIN_FUSE_ACCQ_ROWS=2 against engines
     with both at 0 and against the oracle.  At knob 2 neither Evaluator::accp_in_rows nor accq_in_rows bounds beta, so every single-key
     switch of these engines runs the row-pass kernels (DESIGN.md 6k lists the kernels of one traced case).

Chains that test_param_corners_gpu.py does not have are in NEW.  Two linear-transform shapes need a word: _absent(2, 1) removes both
terms of a 2 x 1 transform, which lt_create_pts refuses, so that shape keeps its rotated term; the 3 x 5 transform takes the giant steps
[0, 1, 3, 6, 9] (giant step 1 shares the key of baby step 1), so that no case needs more than four rotation keys (19 MB each at
beta = 16)."""
import numpy as np
import pytest

from test_exact_products_gpu import _round, _run_lib, _run_oracle, _same as _same_exact, _same_ct
from test_linear_transform_gpu import _absent, _modup_constant, _oracle, _same_scale, _terms
from test_param_corners_gpu import CORNERS, _ct, _ells, _engine, _evk, _extreme, _imp, _max_evk, _rev, _same
from test_q_limb_rows_gpu import _accq_want, _pinv
from test_special_limb_rows_gpu import _accp_want, _eq, _limb_transforms

pytestmark = pytest.mark.gpu
LD = np.longdouble
ERR_STATE = 4

# chain -> (preset, overrides, the branch it is there for)
NEW = {
    "p60_b16": ("toy", dict(n_q=16, dnum=16, first_bits=60, scale_bits=59), "16 digit products of 59/60-bit residues"),
    "a2_b10": ("toy", dict(n_q=20, dnum=10), "more than 8 digits with alpha > 1: own = t / alpha, a short last digit at ell = 19"),
    "p60_b8": ("toy", dict(n_q=8, dnum=8, first_bits=60, scale_bits=59), "the SHORT variant at its eight-product capacity"),
    "k8": ("toy", dict(n_p=8), "moddown_rescale_exact_conv_kernel<8>: the last full-body instantiation below <16>"),
    "toy13": ("toy13", {}, "the preset of tests/test_exact_products_gpu.py, k = 3"),
}
CHAINS = dict(CORNERS, **NEW)
VARIANTS = {
    "default": {},
    "sequence": {"FHELIN_EXACT_PRODUCTS": "0"},
    "max": {},                                        # a context of its own: its keys are the crafted ones
    "max_sequence": {"FHELIN_EXACT_PRODUCTS": "0"},
    "rows": {"FHELIN_FUSE_ACCP_ROWS": "2", "FHELIN_FUSE_ACCQ_ROWS": "2", "FHELIN_ACCP_ROWS_MIN_VECS": "0", "FHELIN_ACCQ_ROWS_MIN_VECS": "0"},
    "launches": {"FHELIN_FUSE_ACCP_ROWS": "0", "FHELIN_FUSE_ACCQ_ROWS": "0"},
}
VARIANTS.update(rows_max=VARIANTS["rows"], launches_max=VARIANTS["launches"])
_ENGINES = {}
_KEYS = {}


def _make(fa, chain, env):
    """a context of the chain created with the given knobs (they are read when the context is created)"""
    if not env and chain in CORNERS:
        return _engine(fa, chain)
    preset, over, _ = CHAINS[chain]
    mp = pytest.MonkeyPatch()
    try:
        for k, v in env.items():
            mp.setenv(k, v)
        return fa.Engine(preset, device=0, seed=1, **over)
    finally:
        mp.undo()


@pytest.fixture(scope="module")
def engines(fa):
    def get(chain, variant="default"):
        if (chain, variant) not in _ENGINES:
            _ENGINES[(chain, variant)] = _make(fa, chain, VARIANTS[variant])
        return _ENGINES[(chain, variant)]
    yield get
    for e in _ENGINES.values():
        e.close()
    _ENGINES.clear()
    _KEYS.clear()


def _uniform_keys(orc, engs, chain, indices, relin=False):
    """uniform 'keys' of the chain (parity of integer functions needs no real ones), made once and imported once per engine:
    {index: key}, and under "relin" the relinearisation key"""
    made = _KEYS.setdefault(chain, {})
    out = {}
    for r in list(indices) + (["relin"] if relin else []):
        if r not in made:
            made[r] = (_evk(orc, engs[0], 4242 if r == "relin" else 7300 + 17 * (r % 100003)), set())
        key, holders = made[r]
        for e in engs:
            if id(e) not in holders:
                e.key_import(0, 0, key) if r == "relin" else e.key_import(1, r, key)
                holders.add(id(e))
        out[r] = key
    return out


# ================================================================================================ 1. linear transforms
LT_CORNERS = ["a1_b16", "a16_k16", "a9", "a5_k5", "k1", "k9", "p53", "p57", "p60", "p60_a1", "p24", "lift", "p60_b16"]
# (baby, giant): G = 1; G = 2; a launch of four groups and a launch of one
LT_SHAPES = [([0, 1], [0]), ([0, 1, 2, 3], [0, 4]), ([0, 1, 2], [0, 1, 3, 6, 9])]


def _lt_absent(n1, n2):
    a = _absent(n1, n2)
    return a if len(a) < n1 * n2 else {(0, 0)}


@pytest.mark.parametrize("corner", LT_CORNERS)
def test_linear_transforms_at_the_corners(engines, orc, corner):
    """lt_apply against rotate_each_sum over hoisted_dot at the levels n_q, alpha + 1, alpha (and 2), with absent terms, for 1 and 3
    rows and once with rescale=True"""
    eng = engines(corner)
    keys = _uniform_keys(orc, [eng], corner, [1, 2, 3, 4, 6, 9])
    rev = _rev(eng, keys)
    for baby, giant in LT_SHAPES:
        n1, n2 = len(baby), len(giant)
        absent = _lt_absent(n1, n2)
        pts, encs = _terms(eng, n1, n2, absent, seed=11 * n1 + n2)
        lt = eng.lt_create_pts(pts, baby, giant)
        assert lt.info()["n_terms"] == n1 * n2 - len(absent)
        for li, ell in enumerate(_ells(eng)):
            what = (corner, n1, n2, ell)
            pairs = [_imp(eng, rev, _ct(orc, eng, 600 + 7 * i + ell, ell)) for i in range(3)]
            want = [_oracle(rev, r, encs, baby, giant) for _, r in pairs]
            for rows in (1, 3):
                got = eng.lt_apply(lt, [p[0] for p in pairs[:rows]])
                assert len(got) == rows
                for g, w in zip(got, want):
                    _same(g, w, what + (rows,))
                    _same_scale(g, w)
            if li == 0 and n2 == 2 and ell >= 2:
                g = eng.lt_apply(lt, [pairs[0][0]], rescale=True)[0]
                w = rev.rescale(want[0])
                _same(g, w, what + ("rescale",))
                _same_scale(g, w)


@pytest.mark.parametrize("corner,full", [("p60", True), ("p60", False), ("p60_a1", True), ("p60_a1", False)])
def test_lt_32_steps_of_sixty_bit_residues(engines, orc, corner, full):
    """test_boundary_residues of tests/test_linear_transform_gpu.py on the 60-bit chains: every key word m - 1, c1 = q - 1 everywhere, 32
    steps; plaintexts made residue by residue over the full key basis, holding q - 1, 2^30 - 1, 1 and 0 at coefficients 0, 255, 256,
    N/2 - 1, N/2, N - 1 and uniform words elsewhere - the group sums' 2^125 bound where the residues really are near 2^60.  The whole
    result equals the oracle composition; at the six coefficients the oracle's words are re-summed with Python integers (the closed form
    of that test, alpha and the chain as variables)."""
    eng = engines(corner, "max")
    N, nq, n1 = eng.N, eng.n_q, 32
    ell = nq if full else 1
    baby, giant = list(range(n1)), [0]
    mx_key = np.stack([np.full(N, int(m) - 1, dtype=np.uint64) for m in eng.moduli])
    mx_key = np.ascontiguousarray(np.broadcast_to(mx_key, (eng.dnum_digits, 2) + mx_key.shape))
    for r in baby[1:]:
        eng.key_import(1, r, mx_key)
    rev = _rev(eng, {r: mx_key for r in baby[1:]})
    x = _ct(orc, eng, 4242, ell)
    x[1] = np.stack([np.full(N, int(m) - 1, dtype=np.uint64) for m in eng.q[:ell]])
    c, r = _imp(eng, rev, x)
    sf = rev.sf[rev.level(r)]
    spots = [0, 255, 256, N // 2 - 1, N // 2, N - 1]
    fullv, blank = [], []
    for b in range(n1):
        v = orc.uniform_residues(31000 + b, eng.moduli, N)
        for k, n in enumerate(spots):
            for t, m in enumerate(eng.moduli):
                v[t, n] = [int(m) - 1, (1 << 30) - 1, 1, 0][(k + b + t) % 4]
        z = v.copy()
        z[:nq, spots] = 0
        fullv.append(v)
        blank.append(z)
    assert int(eng.q[0]).bit_length() == 60 and max(int(v[0, 0]) for v in fullv) == int(eng.q[0]) - 1
    pts = [[eng.debug_pt_from_residues_full(v, sf) for v in fullv]]
    want = _oracle(rev, r, [[(lambda v: (lambda e, sc: v[:e]))(v) for v in fullv]], baby, giant)
    base = _oracle(rev, r, [[(lambda v: (lambda e, sc: v[:e]))(v) for v in blank]], baby, giant)
    D = _modup_constant(eng, ell)
    P = 1
    for m in eng.p:
        P *= int(m)
    maps = {b: orc.automorph_ntt(np.arange(N, dtype=np.uint64), orc.galois(eng.log_n, b)) for b in baby[1:]}   # sigma_b(c)[n] = c[maps[b][n]]
    for t in range(ell):
        m = int(eng.q[t])
        W = (m - 1) * sum(Dj[t] for Dj in D) % m          # sum_j D[j][t] * (q_t - 1)
        wp = W * pow(P % m, -1, m) % m
        for n in spots:
            e0, e1 = int(x[0, t, n]) * int(fullv[0][t, n]), int(x[1, t, n]) * int(fullv[0][t, n])
            for b in baby[1:]:
                mp = int(maps[b][n])
                e0 += int(fullv[b][t, n]) * (wp + int(x[0, t, mp]))
                e1 += int(fullv[b][t, n]) * wp
            assert int(want.d[0, t, n]) == (int(base.d[0, t, n]) + e0) % m, (t, n)
            assert int(want.d[1, t, n]) == (int(base.d[1, t, n]) + e1) % m, (t, n)
    got = eng.lt_apply(eng.lt_create_pts(pts, baby, giant), [c])[0]
    _same(got, want, (corner, "32 steps", ell))
    _same_scale(got, want)


@pytest.mark.parametrize("corner", ["a1_b16", "p60_b16"])
@pytest.mark.parametrize("form", ["plain", "montgomery"])
def test_lt_16_digits_at_their_maximum(engines, orc, corner, form):
    """near-maximal keys in both forms (this kernel reads EvalKey::d_perm, stored times 2^64: "montgomery" is its maximal form) and
    ciphertext limbs at min(q_j, target) - 1: at alpha = 1 the ModUp hands every digit its largest value, and at ell = 16 both flush
    groups of eight digits are full, at ell = 9 the second holds one"""
    eng = engines(corner, "max")
    assert eng.alpha == 1 and eng.dnum_digits == 16
    mx = _max_evk(eng, form)
    baby, giant = [0, 1, 2], [0]
    for r in baby[1:]:
        eng.key_import(1, r, mx)
    rev = _rev(eng, {r: mx for r in baby[1:]})
    pts, encs = _terms(eng, 3, 1, set(), seed=34)
    lt = eng.lt_create_pts(pts, baby, giant)
    for target in sorted({int(max(eng.moduli)), int(min(eng.p)), int(eng.q[0])}):
        for ell in (eng.n_q, 9):
            x = np.ascontiguousarray(_extreme(eng, orc, target)[:, :ell])
            c, r = _imp(eng, rev, x)
            got = eng.lt_apply(lt, [c])[0]
            want = _oracle(rev, r, encs, baby, giant)
            _same(got, want, (corner, form, hex(target), ell))
            _same_scale(got, want)


# ================================================================================================ 2. the exact merged tail
# p24 gives k = 2, so no chain is added for it
TAIL_CORNERS = ["k1", "a5_k5", "k8", "k9", "k15", "a1_b16", "p53", "p57", "p60", "p60_a1", "lift", "p24"]
COUNTERS = ["limb_ntt", "keyswitch", "keyswitch_limbs", "rescale", "ct_pt_mult", "bootstrap", "encode", "rescale_limbs", "ct_pt_limbs"]


def _trio(engines, orc, chain):
    """(the library as built, the library with FHELIN_EXACT_PRODUCTS=0, the oracle) over one uniform relinearisation key"""
    e1, e0 = engines(chain), engines(chain, "sequence")
    relin = _uniform_keys(orc, [e1, e0], chain, [], relin=True)["relin"]
    return e1, e0, _rev(e1, {"relin": relin})


def _product_limbs(eng):
    """product limb counts n_q - 1, alpha + 1 and 2 that leave a limb to drop and a level above for T1"""
    return sorted({e for e in (eng.n_q - 1, eng.alpha + 1, 2) if e >= 2 and e + 1 <= eng.n_q}, reverse=True)


def _three_ways(e1, e0, items, want, what):
    got1, got0 = _run_lib(e1, items), _run_lib(e0, items)
    assert len(got1) == len(got0) == len(want) == len(items)
    for k, (g1, g0, w) in enumerate(zip(got1, got0, want)):
        assert w.deg == 1
        _same_exact(g1, w, ("as built vs oracle",) + what + (k,))
        _same_exact(g0, w, ("sequence vs oracle",) + what + (k,))
        _same_ct(g1, g0, ("as built vs sequence",) + what + (k,))


@pytest.mark.parametrize("corner", TAIL_CORNERS)
def test_exact_tail_mixed_round(engines, orc, corner):
    """the mixed round of tests/test_exact_products_gpu.py (even and odd powers, a degree-2 operand, factor 1 with an addend, constant and
    subtrahend together) for 3 rows and for 1 (the first row's items in a call of their own)"""
    e1, e0, rev = _trio(engines, orc, corner)
    assert 1 <= e1.n_p <= 15
    for ell in _product_limbs(e1):
        items = _round(orc, e1, rev, ell, 3, 7000 + 10 * ell)
        want = _run_oracle(rev, items)
        assert all(w.ell == ell - 1 for w in want)
        for rows in (3, 1):
            _three_ways(e1, e0, items[:4 * rows], want[:4 * rows], (corner, ell, rows))


def test_k16_runs_the_sequence(engines, orc):
    """a16_k16: K + 1 > 16 sources do not fit the merged tail, so the call runs the sequence: the oracle's bytes, the knob-0 engine's
    bytes, and the knob-0 engine's counters"""
    e1, e0, rev = _trio(engines, orc, "a16_k16")
    assert e1.n_p + 1 > 16
    for ell in _product_limbs(e1):
        items = _round(orc, e1, rev, ell, 3, 7100 + 10 * ell)
        want = _run_oracle(rev, items)
        for e in (e1, e0):
            e.sync()
            e.stats(reset=True)
        _three_ways(e1, e0, items, want, ("a16_k16", ell))
        for e in (e1, e0):
            e.sync()
        s1, s0 = e1.stats(), e0.stats()
        assert s1["keyswitch"] > 0 and s1["limb_ntt"] > 0
        assert {k: s1[k] for k in COUNTERS} == {k: s0[k] for k in COUNTERS}, ell


def test_k0_refuses_mult_affine_batch(engines, orc, fa):
    """n_p = 0: no key switch, with the exact tail or without it"""
    for variant in ("default", "sequence"):
        eng = engines("k0", variant)
        eng.key_import(0, 0, _evk(orc, eng, 4))
        rev = _rev(eng, {})
        items = _round(orc, eng, rev, 3, 1, 7200)
        with pytest.raises(fa.FhelinError) as ei:
            _run_lib(eng, items)
        assert ei.value.code == ERR_STATE, str(ei.value)


def _oracle_sum(rev, item):
    """f a b + constant +- addend before its rescale, as _run_oracle composes it"""
    from oracle.residue_eval import RCt
    a, b, f, cadd, ad, neg = item
    ra = RCt(*a)
    t = rev.mult(ra, ra if b is a else RCt(*b))
    if f == 2:
        t = rev.add(t, t)
    if cadd != 0.0:
        t = rev.add_real(t, cadd)
    if ad is not None:
        t = rev.sub(t, RCt(*ad)) if neg else rev.add(t, RCt(*ad))
    return t


def _threshold_spots(eng, q, p):
    """coefficient -> value: 0, floor(q/2), floor(q/2) + 1 and q - 1 where _with_thresholds of tests/test_param_corners_gpu.py plants
    them (later entries replace earlier ones, as there): spread over the ring and, at 4..11, on both lanes of a coefficient pair"""
    vals = [0, q // 2, q // 2 + 1, q - 1]
    where = {}
    for j, v in enumerate(vals):
        for base in (0, 1, 515, eng.N // 2 + 6, eng.N - 8):
            where[(base + 2 * j + p) % eng.N] = v
    for n, v in zip(range(4, 12), vals + vals[::-1]):
        where[n] = v
    return where


def _planted_item(orc, eng, rev, item):
    """the item with the top limb of its degree-2 addend A rebuilt so that the top limb of f a b + constant + A holds the centring
    boundaries in coefficient form: A enters that sum additively and exactly, so A_top = boundary - (sum with A_top = 0)"""
    a, b, f, cadd, A, neg = item
    assert not neg and A[1] == 2 and A[0].shape == a[0].shape
    top = A[0].shape[1] - 1
    q, psi = int(eng.q[top]), eng.psi_q[top]
    zeroed = A[0].copy()
    zeroed[:, top] = 0
    t0 = _oracle_sum(rev, (a, b, f, cadd, (zeroed, A[1], A[2]), neg))
    planted = A[0].copy()
    for p in range(2):
        c0 = orc.ntt_inverse(t0.d[p, top], q, psi)
        ca = orc.ntt_inverse(A[0][p, top], q, psi)
        for n, v in _threshold_spots(eng, q, p).items():
            ca[n] = (v - int(c0[n])) % q
        planted[p, top] = orc.ntt_forward(ca, q, psi)
    return (a, b, f, cadd, (planted, A[1], A[2]), neg)


@pytest.mark.parametrize("corner", ["toy13", "p60", "lift", "k9"])
def test_exact_tail_centring_thresholds(engines, orc, corner):
    """x_top, the top-limb coefficient of the unmerged result before its rescale, at 0, floor(q/2) (stays positive), floor(q/2) + 1 (turns
    negative) and q - 1: for a factor-1 and a factor-2 item (f2 doubles the conversion), with and without a constant, at 2 product limbs
    and at n_q - 1.  lift: q_top >= 2 q_t, the qlm branch on a 40-bit target.  Expected: the oracle's rescale of the planted sum."""
    e1, e0, rev = _trio(engines, orc, corner)
    n_q = e1.n_q
    for ell in (n_q - 1, 2):
        sc = LD(float(rev.sf[n_q - ell]))
        t2 = (_ct(orc, e1, 8100 + ell, ell), 1, sc)
        items = []
        for i, (f, cadd) in enumerate([(1, 0.0), (2, 0.0), (1, -1.0), (2, -1.0)]):
            A = (_ct(orc, e1, 8200 + 10 * i + ell, ell), 2, LD(float(sc * sc)))
            items.append(_planted_item(orc, e1, rev, (t2, t2, f, cadd, A, False)))
        top = ell - 1
        q, psi = int(e1.q[top]), e1.psi_q[top]
        want = []
        for it in items:
            t = _oracle_sum(rev, it)
            seen = set()
            for p in range(2):
                co = orc.ntt_inverse(t.d[p, top], q, psi)
                for n, v in _threshold_spots(e1, q, p).items():
                    assert int(co[n]) == v, (corner, ell, p, n)
                    seen.add((v, n & 1))
            assert seen == {(v, lane) for v in (0, q // 2, q // 2 + 1, q - 1) for lane in (0, 1)}
            want.append(rev.rescale(t))
        for w, w2 in zip(want, _run_oracle(rev, items)):
            assert w.d.tobytes() == w2.d.tobytes() and w.scale == w2.scale
        _three_ways(e1, e0, items, want, (corner, ell, "thresholds"))
        _three_ways(e1, e0, items[1:2], want[1:2], (corner, ell, "thresholds, one item"))


@pytest.mark.parametrize("corner", ["k15", "p60", "a1_b16"])
def test_exact_tail_maximal_operands(engines, orc, corner):
    """a near-maximal relinearisation key ("plain" is the maximal form for ks_inner_kernel) and operands at min(q_j, target) - 1, factor 2,
    a constant and a subtrahend together: 16 sources at k = 15, 60-bit limbs, both flush groups of 16 digits"""
    e1, e0 = engines(corner, "max"), engines(corner, "max_sequence")
    mx = _max_evk(e1, "plain")
    for e in (e1, e0):
        e.key_import(0, 0, mx)
    rev = _rev(e1, {"relin": mx})
    n_q = e1.n_q
    for target in sorted({int(max(e1.moduli)), int(min(e1.p)), int(e1.q[0])}):
        ex = _extreme(e1, orc, target)
        for ell in (n_q - 1, 2):
            x = np.ascontiguousarray(ex[:, :ell])
            y = x.copy()
            y[1] = 1                                       # the relinearised component a1 * b1 = q - 1 as well
            val = lambda d: (d, 1, LD(float(rev.sf[n_q - d.shape[1]])))
            a, b, t1 = val(x), val(y), val(np.ascontiguousarray(ex[:, :ell + 1]))
            items = [(a, b, 2, -1.0, t1, True), (a, a, 2, -1.0, t1, True)]
            _three_ways(e1, e0, items, _run_oracle(rev, items), (corner, hex(target), ell))


# ================================================================================================ 3. row-pass product stages
# ring -> levels: n_q, 9 alpha (one term past the flush), 8 alpha (the SHORT border), alpha + 1 and 1; a2_b10 also 19 (a one-limb last digit)
ROW_RINGS = ["a1_b16", "a2_b10", "p60_b16", "p60_b8", "p53", "p57"]
ROW_SHAPE = {"a1_b16": (16, 1), "a2_b10": (20, 2), "p60_b16": (16, 1), "p60_b8": (8, 1), "p53": (12, 4), "p57": (12, 4)}   # n_q, alpha


def _row_levels(ring):
    n_q, a = ROW_SHAPE[ring]
    s = {n_q, 9 * a, 8 * a, a + 1, 1} | ({19} if ring == "a2_b10" else set())
    return sorted((e for e in s if e <= n_q), reverse=True)


ROW_CASES = [(r, ell) for r in ROW_RINGS for ell in _row_levels(r)]


def _row_pair(engines, orc, ring, indices=(), relin=False):
    """(engine whose row passes form the sums, engine with the separate launches, keys) over the same uniform keys"""
    on, off = engines(ring, "rows"), engines(ring, "launches")
    assert (on.n_q, on.alpha) == ROW_SHAPE[ring]
    return on, off, _uniform_keys(orc, [on, off], ring, indices, relin=relin)


def _max_row_pair(engines, ring):
    """such a pair in contexts of their own that hold every key word at m - 1 (relinearisation key and rotation 1), imported once"""
    on, off = engines(ring, "rows_max"), engines(ring, "launches_max")
    if ("max", ring) not in _KEYS:
        top = np.stack([np.full(on.N, int(m) - 1, dtype=np.uint64) for m in on.moduli])
        key = np.broadcast_to(top, (on.dnum_digits, 2) + top.shape).copy()
        for e in (on, off):
            e.key_import(0, 0, key)
            e.key_import(1, 1, key)
        _KEYS[("max", ring)] = True
    return on, off


def _args(e):
    return (e.alpha, e.q, e.p, e.psi_q, e.psi_p)


@pytest.mark.parametrize("ring,ell", ROW_CASES)
def test_rows_relinearisation(engines, orc, ring, ell):
    """the identity form (keys as stored, khi = 30; the own limb through its Montgomery factor): raw_mult_relin and mult_batch of 3;
    limb_ntt equal with the knobs on and off"""
    on, off, keys = _row_pair(engines, orc, ring, relin=True)
    rev = _rev(on, {})
    a = [_ct(orc, on, 900 + 7 * i + ell, ell) for i in range(3)]
    b = [_ct(orc, on, 950 + 7 * i + ell, ell) for i in range(3)]
    want = [orc.mult_relin(x, y, keys["relin"], *_args(on)) for x, y in zip(a, b)]
    for e in (on, off):
        _eq(e.raw_mult_relin(e.ct_import(a[0]), e.ct_import(b[0])).export(), want[0], (ring, ell, e is on, "one"))
        got = e.mult_batch([_imp(e, rev, x)[0] for x in a], [_imp(e, rev, y)[0] for y in b])
        for i, g in enumerate(got):
            _eq(g.export(), want[i], (ring, ell, e is on, "batch of 3", i))
    n_on = _limb_transforms(on, lambda: on.raw_mult_relin(on.ct_import(a[0]), on.ct_import(b[0])))
    n_off = _limb_transforms(off, lambda: off.raw_mult_relin(off.ct_import(a[0]), off.ct_import(b[0])))
    assert n_on == n_off and n_on > 0, (n_on, n_off)


@pytest.mark.parametrize("ring", ["p60_b16", "a2_b10"])
def test_rows_relinearisation_on_the_fused_engine_alone(engines, orc, ring):
    """the top level on the engine with the knobs at 2 and on no other: the case to run under a kernel trace, which then lists
    ntt_rows_product_kernel and ntt_rows_epilogue_product_kernel and no ks_inner_kernel"""
    on = engines(ring, "rows")
    relin = _uniform_keys(orc, [on], ring, [], relin=True)["relin"]
    ell = on.n_q
    a, b = _ct(orc, on, 900 + ell, ell), _ct(orc, on, 950 + ell, ell)
    _eq(on.raw_mult_relin(on.ct_import(a), on.ct_import(b)).export(), orc.mult_relin(a, b, relin, *_args(on)), (ring, ell))


@pytest.mark.parametrize("ring,ell", ROW_CASES)
def test_rows_plain_rotations(engines, orc, ring, ell):
    """the gathered form: raw_rotate by 1 (moves the 512-coefficient tiles), 64 (keeps them in place) and -1, rotate_batch of 3; limb_ntt
    equal with the knobs on and off"""
    on, off, keys = _row_pair(engines, orc, ring, [1, 64, -1])
    xs = [_ct(orc, on, 300 + 7 * i + ell, ell) for i in range(3)]
    rot = lambda x, r: orc.rotate(x, keys[r], orc.galois(on.log_n, r), *_args(on))
    for r in (1, 64, -1):
        want = [rot(x, r) for x in (xs if r == 1 else xs[:1])]
        for e in (on, off):
            _eq(e.raw_rotate(e.ct_import(xs[0]), r).export(), want[0], (ring, ell, r, e is on, "one"))
            if r == 1:
                for i, g in enumerate(e.rotate_batch([e.ct_import(x) for x in xs], r)):
                    _eq(g.export(), want[i], (ring, ell, r, e is on, "batch of 3", i))
    n_on = _limb_transforms(on, lambda: on.raw_rotate(on.ct_import(xs[0]), 1))
    n_off = _limb_transforms(off, lambda: off.raw_rotate(off.ct_import(xs[0]), 1))
    assert n_on == n_off and n_on > 0, (n_on, n_off)


@pytest.mark.parametrize("ring,ell", ROW_CASES)
def test_rows_with_their_own_keys(engines, orc, ring, ell):
    """per-row keys and maps: rotate_many over [1, 2, 3] (a shared input), rotate_each (rows with their own inputs) and two inputs in one
    launch (row_mod)"""
    on, off, keys = _row_pair(engines, orc, ring, [1, 2, 3])
    rev = _rev(on, keys)
    xs = [_ct(orc, on, 410 + 3 * i + ell, ell) for i in range(3)]
    rot = lambda x, r: orc.rotate(x, keys[r], orc.galois(on.log_n, r), *_args(on))
    want = {(i, r): rot(xs[i], r) for i, r in [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (1, 1), (2, 2)]}
    for e in (on, off):
        for r, g in zip([1, 2, 3], e.rotate_many(e.ct_import(xs[0]), [1, 2, 3])):
            _eq(g.export(), want[0, r], (ring, ell, e is on, "rotate_many", r))
        for i, (r, g) in enumerate(zip([3, 1, 2], e.rotate_each([e.ct_import(x) for x in xs], [3, 1, 2]))):
            _eq(g.export(), want[i, r], (ring, ell, e is on, "rotate_each", i))
        cs = [_imp(e, rev, x)[0] for x in xs[:2]]
        for i, outs in enumerate(e.debug_rotate_many_batch(cs, [2, 3])):
            for r, g in zip([2, 3], outs):
                _eq(g.export(), want[i, r], (ring, ell, e is on, "two inputs", i, r))


# ---- crafted operands, at the kernel (fhelin_debug_ks_accq / fhelin_debug_ks_accp)
def _kernel_levels(ring):
    """the levels with beta = 8, 9, 10 and 16 where the ring has them (a2_b10: also the short last digit), else the full chain"""
    n_q, a = ROW_SHAPE[ring]
    s = {b * a for b in (8, 9, 10, 16) if b * a <= n_q} | ({19} if ring == "a2_b10" else set())
    return sorted(s or {n_q}, reverse=True)


KERNEL_CASES = [(r, ell, index) for r in ROW_RINGS for ell in _kernel_levels(r) for index in (0, 1)]


@pytest.mark.parametrize("ring,ell,index", KERNEL_CASES)
def test_rows_uniform_operands_at_the_kernel(engines, orc, ring, ell, index):
    """uniform canonical digits, own limb and conv against sums formed by the oracle's dyadic functions: index 0 is the identity form over
    the key as stored (khi = 30), index 1 the gathered form; two batch rows at the top level"""
    on, off, keys = _row_pair(engines, orc, ring, [1], relin=True)
    batch = 2 if ell == on.n_q else 1
    beta, nt = -(-ell // on.alpha), ell + on.n_p
    mods = np.concatenate([np.asarray(on.q[:ell], dtype=np.uint64), np.asarray(on.p, dtype=np.uint64)])
    d = np.stack([orc.uniform_residues(5000 + 13 * i, mods, on.N) for i in range(batch * beta)]).reshape(batch, beta, nt, on.N)
    own = np.stack([orc.uniform_residues(6000 + 13 * i, on.q[:ell], on.N) for i in range(batch)])
    conv = np.stack([orc.uniform_residues(7000 + 13 * i, on.q[:ell], on.N) for i in range(2 * batch)]).reshape(batch, 2, ell, on.N)
    key = keys[1] if index else keys["relin"]
    g = orc.galois(on.log_n, index) if index else None
    want_q = _accq_want(orc, on, ell, d, own, conv, key, g)
    want_p = _accp_want(orc, on, ell, d, [key], [g] if index else None)
    for e in (on, off):
        _eq(e.debug_ks_accq(d, own, conv, ell, index), want_q, (ring, ell, index, e is on, "Q limbs"))
        _eq(e.debug_ks_accp(d, ell, [index] if index else []), want_p, (ring, ell, index, e is on, "special limbs"))


@pytest.mark.parametrize("ring,ell,index", KERNEL_CASES)
def test_rows_maximal_operands_at_the_kernel(engines, orc, ring, ell, index):
    """test_maximal_operands (Q limbs) and test_maximal_operands_reach_the_fold_bound (special limbs) with beta as a variable: every key
    residue m - 1, the own limb q - 1 and every digit at the largest value its class hands over - q - 1, or 86q - 1 where the lazy
    forward transform leaves digits unreduced (q < 2^53); conv = 0 and every coefficient of conv at q - 1; then all-zero digits and an
    all-zero own limb under the same key.  Expected: the constant vectors of the sums in closed form."""
    on, off = _max_row_pair(engines, ring)
    beta, nt = -(-ell // on.alpha), ell + on.n_p
    q = [int(v) for v in on.q[:ell]]
    p = [int(v) for v in on.p]
    big = lambda m: (86 * m if m < (1 << 53) else m) - 1
    r2 = lambda m: 1 if index else pow(1 << 64, -1, m)
    for zero in (False, True):
        d = np.zeros((1, beta, nt, on.N), dtype=np.uint64)
        own = np.zeros((1, ell, on.N), dtype=np.uint64)
        if not zero:
            for t, m in enumerate(q):
                d[:, :, t, :] = big(m)
                own[:, t, :] = m - 1
            for i, m in enumerate(p):
                d[:, :, ell + i, :] = big(m)
        cq = [0 if zero else ((beta - 1) * big(m) * (m - 1) * r2(m) + (m - 1) * (m - 1)) % m for m in q]
        cp = [0 if zero else beta * big(m) * (m - 1) * r2(m) % m for m in p]
        acc = np.stack([np.full(on.N, v, dtype=np.uint64) for v in cq])
        want_p = orc.ntt_batch(np.stack([np.full(on.N, v, dtype=np.uint64) for v in cp]), p, on.psi_p, inverse=True)
        for e in (on, off):
            got = e.debug_ks_accp(d, ell, [index] if index else [])
            for c in range(2):
                _eq(got[0, c], want_p, (ring, ell, index, zero, e is on, c, "special limbs"))
        for conv_max in (False, True):
            cv = np.stack([np.full(on.N, m - 1 if conv_max else 0, dtype=np.uint64) for m in q])
            want_q = orc.mul_scalar(orc.sub(acc, orc.ntt_batch(cv, q, on.psi_q[:ell]), q), _pinv(on, ell), q)
            conv = np.broadcast_to(cv, (1, 2) + cv.shape).copy()
            for e in (on, off):
                got = e.debug_ks_accq(d, own, conv, ell, index)
                for c in range(2):
                    _eq(got[0, c], want_q, (ring, ell, index, zero, conv_max, e is on, c, "Q limbs"))

