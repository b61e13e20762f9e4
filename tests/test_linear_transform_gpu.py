"""Linear transforms (include/fhelin.h "Linear transforms"): fhelin_lt_apply, the baby-step/giant-step matrix x ciphertext product whose
baby steps share one ModUp and whose key products are multiplied into all giant-step groups' sums by ks_inner_dot_kernel, against its
defining composition  rotate_each_sum([hoisted_dot(x, V_g, baby[1:]) for g], giant)  of oracle/residue_eval.py - bit for bit, limbs,
noise degree and 80-bit scale included - and against the existing entry points, crafted boundary residues, real keys and refusals."""
import numpy as np
import pytest

from test_default_path_gpu import _ct, _evk, _imp, _keys, _rev, _same
from test_evalkeys_gpu import move

pytestmark = pytest.mark.gpu
LD = np.longdouble
ERR_ARG, ERR_STATE, ERR_KEY = 1, 4, 5


def _zeros(eng):
    return lambda ell, sc: np.zeros((ell, eng.N), dtype=np.uint64)


def _export_enc(eng, p):
    return lambda ell, sc: eng.pt_export(p, ell, sc)


def _terms(eng, n1, n2, absent, seed):
    """pts [n2][n1] of engine plaintexts (None where absent) and the oracle-side encoders (zeros where absent)"""
    rng = np.random.default_rng(seed)
    ns = 1 << eng.params.log_slots
    pts = [[None if (g, b) in absent else eng.encode(rng.uniform(-1, 1, ns)) for b in range(n1)] for g in range(n2)]
    encs = [[_zeros(eng) if p is None else _export_enc(eng, p) for p in row] for row in pts]
    return pts, encs


def _oracle(rev, r, encs, baby, giant, rescale=False):
    """the defining composition on one row"""
    inner = [rev.hoisted_dot(r, e, baby[1:]) for e in encs]
    out = rev.rotate_each_sum(inner, giant)
    return rev.rescale(out) if rescale else out


def _same_scale(ct, r):
    hi, lo = ct.scale_parts()
    assert LD(hi) + LD(lo) == r.scale


def _oracle_keys(orc, eng, indices, skip=(), seed=7300):
    """uniform 'keys' for every index on the oracle's side; the engine gets all but `skip` (indices whose key it must not need)"""
    keys = {}
    for r in indices:
        keys[r] = _evk(orc, eng, seed + 17 * (r % 100003))
        if r not in skip:
            eng.key_import(1, r, keys[r])
    return keys


# absent terms of every shape: the (g = 0, b = 0) term, one whole baby column (the last), and one more where the shape has room
def _absent(n1, n2):
    a = {(0, 0)} | {(g, n1 - 1) for g in range(n2)}
    if n1 > 2 and n2 > 1:
        a.add((n2 - 1, 1))
    return a


@pytest.mark.parametrize("preset,ells,n1,n2,rows,variants", [
    ("toy", [6, 5, 3, 2], 4, 2, 2, [(1, False)]),                        # alpha = 2: full, partial and single digit
    ("toy13", [7, 4], 8, 3, 3, [(1, False), (1, True), (2, False), (2, True)]),   # an odd row count; degree 2 is rescaled first
    ("toy13", [6], 16, 2, 1, [(1, False)]),                              # past hoisted_dot's 7 rotations
    ("toy13", [6], 32, 1, 1, [(1, False)]),                              # the kernel's maximum of 32 steps
    ("toy", [4], 2, 9, 2, [(1, False)]),                                 # more groups than one launch holds (4) and than one shared ModDown (7)
    ("toy", [4], 3, 9, 1, [(1, False)]),                                 # the same with a rotated baby step in every launch
    ("reference", [9], 4, 2, 1, [(1, False)]),                           # N = 2^15, alpha = 7: four imported keys
])
def test_lt_apply_bit_exact(engine_factory, orc, preset, ells, n1, n2, rows, variants):
    eng = engine_factory(preset)
    baby = list(range(n1))
    giant = [g * n1 for g in range(n2)]
    absent = _absent(n1, n2)
    keys = _oracle_keys(orc, eng, baby[1:] + giant[1:], skip={baby[-1]} if n1 > 1 else ())
    rev = _rev(orc, eng, keys)
    pts, encs = _terms(eng, n1, n2, absent, seed=11 * n1 + n2)
    lt = eng.lt_create_pts(pts, baby, giant)
    assert lt.info() == dict(n1=n1, n2=n2, n_terms=n1 * n2 - len(absent), slots=1 << eng.params.log_slots)
    assert sorted(lt.rotations()) == sorted(set(baby[1:-1]) | set(giant[1:]))
    for ell in ells:
        for deg, rescale in variants:
            pairs = [_imp(eng, rev, _ct(orc, eng, 600 + 7 * i + ell, ell), deg=deg) for i in range(rows)]
            got = eng.lt_apply(lt, [p[0] for p in pairs], rescale=rescale)
            assert len(got) == rows
            for (c, r), g in zip(pairs, got):
                want = _oracle(rev, r, encs, baby, giant, rescale)
                _same(g, want, (preset, ell, deg, rescale))
                _same_scale(g, want)
    del keys


def test_single_diagonal_at_index_zero_needs_no_key(fa, orc):
    """one diagonal at index 0: n1 = n2 = 1, no rotation, no key switch - on a context that holds no key at all"""
    eng = fa.Engine("toy13", seed=5)
    try:
        rev = _rev(orc, eng, {})
        ns = 1 << eng.params.log_slots
        diag = np.random.default_rng(1).uniform(-1, 1, ns)
        lt = eng.lt_create([diag], [0])
        assert lt.info()["n1"] == 1 and lt.info()["n2"] == 1 and lt.rotations() == []
        before = eng.stats()
        c, r = _imp(eng, rev, _ct(orc, eng, 77, 5))
        got = eng.lt_apply(lt, [c])[0]
        assert eng.stats()["keyswitch"] == before["keyswitch"]
        sf = rev.sf[rev.level(r)]
        full = eng.pt_export(eng.encode(diag), eng.n_q + eng.n_p, sf)[None]
        evks = np.zeros((0, eng.dnum_digits, 2, eng.n_limbs, eng.N), dtype=np.uint64)
        want = orc.hoisted_dot(r.d, evks, np.zeros(0, dtype=np.uint64), full, eng.alpha, eng.q, eng.p, eng.psi_q, eng.psi_p)
        inf = got.info()
        assert (inf["npoly"], inf["ell"], inf["deg"]) == (2, 5, 2)
        assert np.array_equal(got.export(), want)
        hi, lo = got.scale_parts()
        assert LD(hi) + LD(lo) == r.scale * sf
    finally:
        eng.close()


def test_single_diagonal_off_the_baby_grid(engine_factory, orc):
    """one diagonal at index 5 with n1 = 4: b = 1, g = 4, the plaintext is rot(diag, -4)"""
    eng = engine_factory("toy13")
    keys = _keys(orc, eng, [1, 4], seed=5100)
    rev = _rev(orc, eng, keys)
    ns = 1 << eng.params.log_slots
    diag = np.random.default_rng(2).uniform(-1, 1, ns)
    lt = eng.lt_create([diag], [5], n1=4)
    assert lt.info() == dict(n1=4, n2=1, n_terms=1, slots=ns) and sorted(lt.rotations()) == [1, 4]
    v = eng.encode(np.roll(diag, 4))
    c, r = _imp(eng, rev, _ct(orc, eng, 88, 6))
    got = eng.lt_apply(lt, [c])[0]
    want = _oracle(rev, r, [[_zeros(eng), _export_enc(eng, v)]], [0, 1], [4])
    _same(got, want, "index 5")
    _same_scale(got, want)
    del keys


@pytest.mark.parametrize("baby,giant", [
    ([0, 64, 128, 192], [0, 256, 512]),                                  # multiples of 64: the rotations that keep 512-coefficient tiles in place
    ([0, 1, 3, 5, 7, 9, 11, 13], [0, 17, 35]),                           # odd amounts, n1 = 8
])
def test_equal_to_the_existing_entry_points(engine_factory, orc, baby, giant):
    """for n1 <= 8 the same composition runs through the C ABI: fhelin_rotate_each_sum over fhelin_hoisted_dot, export for export"""
    eng = engine_factory("toy13")
    _keys(orc, eng, baby[1:] + giant[1:], seed=8200)
    pts, _ = _terms(eng, len(baby), len(giant), set(), seed=3)
    lt = eng.lt_create_pts(pts, baby, giant)
    for ell in (7, 4):
        xs = [eng.ct_import(_ct(orc, eng, 900 + 5 * i + ell, ell)) for i in range(3)]
        got = eng.lt_apply(lt, xs)
        for x, g in zip(xs, got):
            want = eng.rotate_each_sum([eng.hoisted_dot([x], row, baby[1:])[0] for row in pts], giant)
            assert g.info() == want.info()
            assert np.array_equal(g.export(), want.export())
            assert g.scale_parts() == want.scale_parts()


def _modup_constant(eng, ell):
    """Python integers: the ModUp digits D[j][t] of the polynomial whose NTT form is q_i - 1 everywhere (the constant q_i - 1: its
    only nonzero coefficient is the first, and the forward transform of a constant is that constant at every point), over the targets
    t = q_0..q_{ell-1}, p_0..p_{k-1}:  D[j][t] = sum_{i in digit j} [(q_i - 1) (Q_j/q_i)^-1]_{q_i} (Q_j/q_i) mod t, the own digit's limbs as they are"""
    q = [int(v) for v in eng.q[:ell]]
    mods = q + [int(v) for v in eng.p]
    a = eng.alpha
    D = []
    for lo in range(0, ell, a):
        dig = list(range(lo, min(ell, lo + a)))
        row = []
        for t, m in enumerate(mods):
            if t in dig:
                row.append(m - 1)
                continue
            s = 0
            for i in dig:
                hat = 1
                for i2 in dig:
                    if i2 != i:
                        hat *= q[i2]
                s += ((q[i] - 1) * pow(hat % q[i], -1, q[i]) % q[i]) * hat
            row.append(s % m)
        D.append(row)
    return D


@pytest.mark.parametrize("ell", [6, 1])
def test_boundary_residues(engine_factory, orc, ell):
    """every key word q - 1, c1 = q - 1 everywhere, 32 steps; plaintexts made residue by residue over the full key basis, holding q - 1,
    the all-ones low half, 1 and 0 at coefficients 0, 255, 256, N/2 - 1, N/2, N - 1 and uniform words elsewhere.  The whole result equals the
    oracle composition; at the six coefficients the oracle's words are re-summed here with Python integers: with the key products
    W[t] = -(sum_j D[j][t]) (constant, _modup_constant) the planted Q-limb words contribute
        sum_b V_b[t][n] (W[t] P^-1 + sigma_b(c0)[t][n])  (+ V_0[t][n] c[t][n])      mod q_t
    on top of the oracle's result for the same plaintexts with zeros planted there (same special limbs: same conversion)."""
    eng = engine_factory("toy")
    N, nq, n1 = eng.N, eng.n_q, 32
    baby, giant = list(range(n1)), [0]
    mx_key = np.stack([np.full(N, int(m) - 1, dtype=np.uint64) for m in eng.moduli])
    mx_key = np.ascontiguousarray(np.broadcast_to(mx_key, (eng.dnum_digits, 2) + mx_key.shape))
    for r in baby[1:]:
        eng.key_import(1, r, mx_key)
    rev = _rev(orc, eng, {r: mx_key for r in baby[1:]})
    x = _ct(orc, eng, 4242, ell)
    x[1] = np.stack([np.full(N, int(m) - 1, dtype=np.uint64) for m in eng.q[:ell]])
    c, r = _imp(eng, rev, x)
    sf = rev.sf[rev.level(r)]
    spots = [0, 255, 256, N // 2 - 1, N // 2, N - 1]
    full, blank = [], []
    for b in range(n1):
        v = orc.uniform_residues(31000 + b, eng.moduli, N)
        for k, n in enumerate(spots):
            for t, m in enumerate(eng.moduli):
                v[t, n] = [int(m) - 1, (1 << 30) - 1, 1, 0][(k + b + t) % 4]
        z = v.copy()
        z[:nq, spots] = 0
        full.append(v)
        blank.append(z)
    pts = [[eng.debug_pt_from_residues_full(v, sf) for v in full]]
    want = _oracle(rev, r, [[(lambda v: (lambda e, sc: v[:e]))(v) for v in full]], baby, giant)
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
            e0, e1 = int(x[0, t, n]) * int(full[0][t, n]), int(x[1, t, n]) * int(full[0][t, n])
            for b in baby[1:]:
                mp = int(maps[b][n])
                e0 += int(full[b][t, n]) * (wp + int(x[0, t, mp]))
                e1 += int(full[b][t, n]) * wp
            assert int(want.d[0, t, n]) == (int(base.d[0, t, n]) + e0) % m, (t, n)
            assert int(want.d[1, t, n]) == (int(base.d[1, t, n]) + e1) % m, (t, n)
    got = eng.lt_apply(eng.lt_create_pts(pts, baby, giant), [c])[0]
    _same(got, want, ("boundary", ell))
    _same_scale(got, want)


# 16 diagonals: negative indices, multiples of 128 as the drivers rotate by, and neighbours of both
DIAG_IDX = [0, 1, 2, 3, -1, -2, -3, 5, 128, 256, 384, -128, 130, 257, 1024, -1023]


def _semantics(ns):
    rng = np.random.default_rng(9)
    diags = rng.uniform(-1, 1, (len(DIAG_IDX), ns))
    xs = [rng.uniform(-1, 1, ns) for _ in range(2)]
    wants = [sum(d * np.roll(x, -i) for d, i in zip(diags, DIAG_IDX)) for x in xs]
    return diags, xs, wants


def test_semantics_with_real_keys(fa, tmp_path):
    """decrypt(lt_apply(x)) = sum_d diag_d * roll(x, -d) with the keys fhelin_lt_rotations lists - on the client's context and on an
    evaluation context loaded from the saved key set.  Bound: the 1e-6 of test_hoisted_dot_is_the_sum_of_rotated_products, which the
    mult_plain + rotate + add form on the same inputs must meet too (asserted, so that the bound is known to be this form's class)."""
    cl = fa.Engine("toy13", seed=31)
    path = str(tmp_path / "lt.evk")
    try:
        cl.keygen()
        ns = 1 << cl.params.log_slots
        diags, xs, wants = _semantics(ns)
        lt = cl.lt_create(diags, DIAG_IDX)
        inf = lt.info()
        assert inf["n_terms"] == len(DIAG_IDX) and inf["slots"] == ns and 1 <= inf["n1"] <= 32
        need = lt.rotations()
        cl.gen_rotation_keys(need)
        cts = [cl.encrypt(x) for x in xs]
        outs = cl.lt_apply(lt, cts)
        for o, w in zip(outs, wants):
            assert o.info()["deg"] == 2
            err = np.max(np.abs(cl.decrypt(o)[:ns] - w))
            print("lt_apply max error", err)
            assert err < 1e-6
        for o, w in zip(cl.lt_apply(lt, cts, rescale=True), wants):
            assert o.info()["deg"] == 1 and o.info()["ell"] == cts[0].info()["ell"] - 1
            assert np.max(np.abs(cl.decrypt(o)[:ns] - w)) < 1e-6
        # the same through an evaluation context that never held the secret
        cl.save_eval_keys(path)
        ev = fa.Engine.from_eval_keys(path, seed=4)
        try:
            lt_ev = ev.lt_create(diags, DIAG_IDX)
            assert lt_ev.info() == inf and lt_ev.rotations() == need
            for c, o, w in zip(cts, outs, wants):
                o_ev = ev.lt_apply(lt_ev, [move(c, ev)])[0]
                assert np.array_equal(o_ev.export(), o.export())
                assert np.max(np.abs(cl.decrypt(move(o_ev, cl))[:ns] - w)) < 1e-6
        finally:
            ev.close()
        # the products-then-sum form on the same inputs: rot(x, d) * diag_d, added up
        cl.gen_rotation_keys([d for d in DIAG_IDX if d])
        acc = None
        for d, i in zip(diags, DIAG_IDX):
            t = cl.mult(cl.rotate(cts[0], i) if i else cts[0], cl.encode(d))
            acc = t if acc is None else cl.add(acc, t)
        ref_err = np.max(np.abs(cl.decrypt(acc)[:ns] - wants[0]))
        print("mult_plain + rotate + add max error", ref_err)
        assert ref_err < 1e-6
    finally:
        cl.close()


def test_refusals(fa, orc):
    eng = fa.Engine("toy13", seed=8)
    try:
        ns = 1 << eng.params.log_slots
        rng = np.random.default_rng(4)
        diags = rng.uniform(-1, 1, (3, ns))
        # creation: the encoder's domain rule, duplicates (mod slots), an empty list, another packing
        bad = diags.copy()
        bad[1, 7] = float("nan")
        for fn in (lambda: eng.lt_create(bad, [0, 1, 2]), lambda: eng.lt_create(diags, [1, 2, 1 + ns]), lambda: eng.lt_create(diags, [1, 2, 1]),
                   lambda: eng.lt_create([], []), lambda: eng.lt_create(diags[:, :ns // 2], [0, 1, 2], slots=ns // 2),
                   lambda: eng.lt_create(diags, [0, 1, 2], n1=33)):
            with pytest.raises(fa.FhelinError) as ei:
                fn()
            assert ei.value.code == ERR_ARG
        # a missing key: named, no handle, the level plan's source counter where it was
        lt = eng.lt_create(diags, [0, 1, 6], n1=4)
        assert sorted(lt.rotations()) == [1, 2, 4]
        _keys(orc, eng, [1, 4], seed=10)
        x = eng.ct_import(_ct(orc, eng, 5, 4))
        source = eng.level_plan_tell()[1]
        with pytest.raises(fa.FhelinError) as ei:
            eng.lt_apply(lt, [x, x])
        assert ei.value.code == ERR_KEY and "index 2" in str(ei.value)
        assert eng.level_plan_tell()[1] == source
        _keys(orc, eng, [2], seed=10)
        assert len(eng.lt_apply(lt, [x, x])) == 2 and eng.level_plan_tell()[1] == source
    finally:
        eng.close()
    # interleaved samples are out of scope
    il = fa.Engine("toy13", seed=8, interleave=2, log_slots=11)      # two samples of 2048 slots in the 4096 physical slots
    try:
        with pytest.raises(fa.FhelinError) as ei:
            il.lt_create(np.ones((1, 1 << il.params.log_slots)), [0])
        assert ei.value.code == ERR_STATE
    finally:
        il.close()
