"""The kernels at every parameter corner Context accepts, bit for bit against the oracle.  The kernels choose their code by the digit
size alpha (modup_conv_kernel<1..8> / <16>), the number of special primes k (moddown_conv_kernel<1..8> / <16>, the merged ModDown +
rescale with k + 1 <= 16 sources), the digit count beta (ks_inner_kernel's Acc30 flush per 8 digits, ks_inner_multi_kernel's fold
every 16 products) and the size of the primes (lazy / semi-lazy / classic NTT butterflies around 2^53 and 2^57, the fused or separate
centred lift of a rescale).  The presets reach only alpha, k in {2..8}, beta <= 4 and 52-55-bit Q primes; the corners below reach the
rest.  Every corner runs the leaf operations at the levels n_q, alpha + 1, alpha (and 2) - full, partial and single digits - with
uniform random keys, then the accumulation bounds with crafted operands (near-maximal keys, maximal as each kernel multiplies them,
ciphertext limbs at their maximum), and
the centring thresholds of the rescale and ModRaise lifts (coefficients 0, q/2, q/2 + 1, q - 1 planted in coefficient form)."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
LD = np.longdouble
IDX = [1, 2, 3, 4, 5, 6, 7]          # rotate_sum with 7 indices: the kernel's maximum of merged rotations

# corner -> (preset, overrides, the branch it is there for)
CORNERS = {
    "a1_b16": ("toy", dict(n_q=16, dnum=16),
               "modup_conv_kernel<1>; beta = 16: both Acc30 flush groups of ks_inner_kernel, long fold chains in ks_inner_multi_kernel"),
    "a16_k16": ("toy", dict(n_q=16, dnum=1, n_p=16),
                "modup_conv_kernel<16> and moddown_conv_kernel<16> full bodies; k = 16: ModDown then rescale in place of the merged form"),
    "a9": ("toy13", dict(n_q=17, dnum=2), "modup_conv_kernel<16> guarded body (digits of 9 and 8 limbs)"),
    "a5_k5": ("toy13", dict(n_q=10, dnum=2, n_p=5), "modup_conv_kernel<5>, moddown_conv_kernel<5>"),
    "k1": ("toy", dict(n_p=1), "moddown_conv_kernel<1>; the merged ModDown + rescale with 2 sources"),
    "k9": ("toy", dict(n_p=9), "moddown_conv_kernel<16> guarded body (9 sources)"),
    "k15": ("toy", dict(n_q=8, dnum=2, n_p=15), "the merged ModDown + rescale with exactly 16 sources (its MAXS)"),
    "p53": ("toy13", dict(n_q=12, scale_bits=53), "53/54-bit primes: lazy vs semi-lazy inverse butterflies, lazy_out"),
    "p57": ("toy13", dict(n_q=12, scale_bits=57), "57/58-bit primes: lazy vs classic forward butterflies; q_last >= 2 q0: unfused lift"),
    "p60": ("toy", dict(n_q=8, first_bits=60, scale_bits=59),
            "60-bit q0, 59/60-bit scaling primes: the largest accepted primes; ew_lincomb with 32 terms near q^2 each"),
    "p60_a1": ("toy", dict(n_q=4, dnum=4, first_bits=60, scale_bits=59),
               "alpha = 1 on a 60-bit chain: ModUp digits near 2^60 reach ks_inner_multi_kernel unchanged; rotate_sum's 28 products "
               "per output pass m 2^64 without its fold every 16"),
    "lift": ("toy", dict(n_q=8, first_bits=40, scale_bits=50, special_bits=30, n_p=-1),
             "q_last >= 2 q0: rescale_lift_kernel (the lift cannot ride in the NTT); 30-bit special primes, k = 5"),
    "p24": ("toy", dict(n_q=4, n_p=2, dnum=2, first_bits=24, scale_bits=24, special_bits=24),
            "24-bit primes: the small-prime constants of reduce_lazy_2q and the Shoup products"),
    "n17": ("toy", dict(log_n=17, log_slots=16), "the largest ring, N = 2^17: NTT, rescale and one rotation"),
    "k0": ("toy", dict(n_p=0), "no special prime: NTT and rescale run, every key switch is refused with FHELIN_ERR_STATE"),
}
FULL = [c for c in CORNERS if c not in ("n17", "k0")]
KNOBS = {"fused": {"FHELIN_FUSE_FINISH": "1", "FHELIN_FUSE_LIFT": "1"},
         "no_finish": {"FHELIN_FUSE_FINISH": "0", "FHELIN_FUSE_LIFT": "1"},
         "no_lift": {"FHELIN_FUSE_FINISH": "1", "FHELIN_FUSE_LIFT": "0"}}


def _engine(fa, corner, knobs="fused"):
    """a context of the corner created with the given knobs (they are read when the context is created)"""
    preset, over, _ = CORNERS[corner]
    env = KNOBS[knobs]
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return fa.Engine(preset, device=0, seed=1, **over)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


_CACHE = {}


@pytest.fixture(scope="module")
def corner_engine(fa):
    def get(corner, knobs="fused"):
        if (corner, knobs) not in _CACHE:
            _CACHE[(corner, knobs)] = _engine(fa, corner, knobs)
        return _CACHE[(corner, knobs)]
    yield get
    for e in _CACHE.values():
        e.close()
    _CACHE.clear()


def _ct(orc, eng, seed, ell, npoly=2):
    return np.stack([orc.uniform_residues(seed + 1000 * p, eng.q[:ell], eng.N) for p in range(npoly)])


def _evk(orc, eng, seed):
    d = eng.dnum_digits
    k = np.stack([orc.uniform_residues(seed + 50 * j, eng.moduli, eng.N) for j in range(2 * d)])
    return k.reshape(d, 2, eng.n_limbs, eng.N)


def _max_evk(eng, form):
    """a near-maximal key: limb m holds m - 1 - d_n with d_n < 2^16 varying over the slots (so that the low words of the sums, and
    with them the Montgomery reductions' corrections, differ across the ring).  "plain": these values as imported, the operand
    ks_inner_kernel multiplies (there the ModUp digits carry the Montgomery factor 2^64); "montgomery": the values times 2^-64 mod m,
    which ks_inner_multi_kernel stores times 2^64 (EvalKey::d_perm) and so multiplies as m - 1 - d_n.  For m just above a power of
    two, m - 1 stored times 2^64 is small: each kernel sees its maximal key only in its own form."""
    d = np.random.default_rng(5).integers(0, 1 << 16, size=eng.N)
    rows = []
    for m in (int(x) for x in eng.moduli):
        v = [m - 1 - int(t) for t in d]
        if form == "montgomery":
            inv = pow(1 << 64, -1, m)
            v = [x * inv % m for x in v]
        rows.append(np.array(v, dtype=np.uint64))
    k = np.stack(rows)
    return np.ascontiguousarray(np.broadcast_to(k, (eng.dnum_digits, 2) + k.shape))


def _rev(eng, keys):
    from oracle.residue_eval import ResidueEvaluator
    return ResidueEvaluator(eng.q, eng.p, eng.psi_q, eng.psi_p, eng.alpha, eng.log_n, keys, eng.params.log_slots)


def _imp(eng, rev, x, deg=1):
    from oracle.residue_eval import RCt
    sc = float(rev.sf[len(eng.q) - x.shape[1]])
    if deg == 2:
        sc = float(LD(sc) * LD(sc))
    return eng.ct_import(x, deg=deg, scale=sc), RCt(x, deg, LD(sc))


def _same(ct, r, what=""):
    inf = ct.info()
    assert (inf["npoly"], inf["ell"], inf["deg"]) == (r.npoly, r.ell, r.deg), (what, inf)
    assert np.array_equal(ct.export(), r.d), what


def _ells(eng):
    """n_q, alpha + 1, alpha (and 2 when alpha >= 2): full, partial and single digits, highest first"""
    a = eng.alpha
    s = {eng.n_q, a + 1, a} | ({2} if a >= 2 else set())
    return sorted((e for e in s if 1 <= e <= eng.n_q), reverse=True)


def _with_thresholds(orc, eng, x, limb):
    """x with limb `limb` of every component rebuilt in coefficient form to hold the centring boundaries 0, floor(q/2),
    floor(q/2) + 1 and q - 1 (at both lanes of a coefficient pair and spread over the ring), then mapped back with the oracle's NTT"""
    q, psi = int(eng.q[limb]), eng.psi_q[limb]
    x = x.copy()
    vals = [0, q // 2, q // 2 + 1, q - 1]
    for p in range(x.shape[0]):
        co = orc.ntt_inverse(x[p, limb], q, psi)
        for j, v in enumerate(vals):
            for base in (0, 1, 515, eng.N // 2 + 6, eng.N - 8):
                co[(base + 2 * j + p) % eng.N] = v
        co[4:12] = vals + vals[::-1]
        x[p, limb] = orc.ntt_forward(co, q, psi)
    return x


@pytest.fixture(scope="module")
def corner_keys(orc):
    """uniform relinearisation and rotation keys per corner, imported once"""
    cache = {}

    def get(eng, corner):
        if corner not in cache:
            relin = _evk(orc, eng, 4242)
            rots = {r: _evk(orc, eng, 7100 + 17 * r) for r in IDX}
            eng.key_import(0, 0, relin)
            for r, k in rots.items():
                eng.key_import(1, r, k)
            cache[corner] = (relin, rots)
        return cache[corner]
    yield get
    cache.clear()


@pytest.mark.parametrize("corner", list(CORNERS))
def test_ntt_every_limb(corner_engine, orc, corner):
    """forward and inverse NTT over all Q and P limbs: uniform inputs and the maximal / zero patterns of the lazy butterflies"""
    eng = corner_engine(corner)
    n = eng.N
    idx = np.arange(n)
    pats = [np.ones(n, dtype=bool)] + [((idx // s) & 1).astype(bool) for s in (1, 16, 256, 4096, n // 2)]
    groups = [(eng.q, eng.psi_q, 0)] + ([(eng.p, eng.psi_p, eng.n_q)] if eng.n_p else [])
    for mods, psis, first in groups:
        mods = np.asarray(mods, dtype=np.uint64)
        pat = np.stack([np.where(p[None, :], (mods - np.uint64(1))[:, None], np.uint64(0)) for p in pats])
        rnd = np.stack([orc.uniform_residues(31 + s, mods, n) for s in range(2)])
        for x in (rnd, pat):
            for inverse in (False, True):
                buf = eng.upload(x)
                eng.ntt(buf, x.shape[0] * x.shape[1], limb_first=first, limb_count=len(mods), inverse=inverse)
                got = buf.download(x.shape)
                buf.free()
                assert np.array_equal(got, orc.ntt_batch(x, mods, psis, inverse=inverse)), (corner, first, inverse)


@pytest.mark.parametrize("corner", list(CORNERS))
def test_rescale_and_modraise_at_centring_thresholds(corner_engine, orc, corner):
    """raw_rescale with the fused lift, the separate lift (FHELIN_FUSE_LIFT=0) and the separate finishing kernels
    (FHELIN_FUSE_FINISH=0), rescale_batch with 2 and 3 rows, and raw_modraise: the dropped limb (or ModRaise's source limb) holds the
    centring boundaries 0, floor(q/2) (stays positive), floor(q/2) + 1 (turns negative) and q - 1"""
    engs = {k: corner_engine(corner, k) for k in KNOBS}
    eng = engs["fused"]
    rev = _rev(eng, {})
    ells = [e for e in _ells(eng) if e >= 2] if corner != "n17" else [eng.n_q]
    for ell in ells:
        x = _with_thresholds(orc, eng, _ct(orc, eng, 60 + ell, ell), ell - 1)
        want = orc.rescale(x, eng.q[:ell], eng.psi_q[:ell])
        for k, e in engs.items():
            assert np.array_equal(e.raw_rescale(e.ct_import(x)).export(), want), (corner, ell, k)
        if corner == "n17":
            continue
        for rows in (2, 3):
            xs = [_with_thresholds(orc, eng, _ct(orc, eng, 90 + 7 * i + ell, ell), ell - 1) for i in range(rows)]
            for k, e in engs.items():
                pairs = [_imp(e, rev, xi, deg=2) for xi in xs]
                for got, (_, r) in zip(e.rescale_batch([p[0] for p in pairs]), pairs):
                    _same(got, rev.rescale(r), (corner, ell, rows, k, "rescale_batch"))
    src = _with_thresholds(orc, eng, _ct(orc, eng, 123, 1), 0)
    want = orc.modraise(src[:, 0], eng.n_q, eng.q, eng.psi_q)
    assert np.array_equal(eng.raw_modraise(eng.ct_import(src), eng.n_q).export(), want), (corner, "modraise")


@pytest.mark.parametrize("corner", FULL)
def test_key_switching_at_every_digit_shape(corner_engine, corner_keys, orc, corner):
    """raw_rotate, rotate_batch (2 rows: the row-pair kernel; 3 rows: its odd tail), raw_mult_relin, mult_batch, rotate_sum with 7
    indices (ks_inner_multi_kernel), rotate_each_sum and hoisted_dot with and without the merged ModDown + rescale, at the levels
    n_q, alpha + 1, alpha and 2"""
    eng = corner_engine(corner)
    relin, rots = corner_keys(eng, corner)
    rev = _rev(eng, rots)
    ga = lambda r: orc.galois(eng.log_n, r)
    args = (eng.alpha, eng.q, eng.p, eng.psi_q, eng.psi_p)
    evks = np.stack([rots[r] for r in IDX])
    rng = np.random.default_rng(77)
    ns = 1 << eng.params.log_slots
    pts = [eng.encode(rng.uniform(-1, 1, ns)) for _ in range(4)]
    encs = [(lambda p: (lambda ell, sc: eng.pt_export(p, ell, sc)))(p) for p in pts]
    for ell in _ells(eng):
        what = (corner, ell)
        x, y = _ct(orc, eng, 300 + ell, ell), _ct(orc, eng, 400 + ell, ell)
        assert np.array_equal(eng.raw_rotate(eng.ct_import(x), 5).export(), orc.rotate(x, rots[5], ga(5), *args)), what
        want = orc.mult_relin(x, y, relin, *args)
        assert np.array_equal(eng.raw_mult_relin(eng.ct_import(x), eng.ct_import(y)).export(), want), what
        for rows in (2, 3):
            pairs = [_imp(eng, rev, _ct(orc, eng, 500 + 7 * i + ell, ell)) for i in range(rows)]
            cs, rs = [p[0] for p in pairs], [p[1] for p in pairs]
            for got, r in zip(eng.rotate_batch(cs, 3), rs):
                _same(got, rev.rotate(r, 3), what + (rows, "rotate_batch"))
            for got, a, b in zip(eng.mult_batch(cs, cs[1:] + cs[:1]), rs, rs[1:] + rs[:1]):
                assert np.array_equal(got.export(), orc.mult_relin(a.d, b.d, relin, *args)), what + (rows, "mult_batch")
            for got, r in zip(eng.rotate_sum(cs, IDX), rs):
                assert np.array_equal(got.export(), orc.rotate_sum(r.d, evks, [ga(i) for i in IDX], *args)), what + (rows, "rotate_sum")
            for rescale in (False, True):
                if rescale and ell < 2:
                    continue
                for got, r in zip(eng.hoisted_dot(cs, pts, [1, 2, 3], rescale=rescale), rs):
                    if rescale and eng.n_p + 1 > 16:        # k = 16: ModDown, then a separate rescale
                        want = rev.rescale(rev.hoisted_dot(r, encs, [1, 2, 3], rescale=False))
                    else:
                        want = rev.hoisted_dot(r, encs, [1, 2, 3], rescale=rescale)
                    _same(got, want, what + (rows, "hoisted_dot", rescale))
        terms = [_imp(eng, rev, _ct(orc, eng, 800 + 3 * i + ell, ell)) for i in range(4)]
        _same(eng.rotate_each_sum([t[0] for t in terms], [0, 1, 2, 3]), rev.rotate_each_sum([t[1] for t in terms], [0, 1, 2, 3]),
              what + ("rotate_each_sum",))


@pytest.mark.parametrize("corner", FULL)
def test_lincomb_32_terms(corner_engine, orc, corner):
    """fhelin_lincomb with 32 terms (ew_lincomb_kernel: 32 products summed in 128 bits, one reduction) at every prime class"""
    eng = corner_engine(corner)
    rev = _rev(eng, {})
    rng = np.random.default_rng(8)
    for ell in _ells(eng):
        pairs = [_imp(eng, rev, _ct(orc, eng, 700 + i + ell, ell)) for i in range(32)]
        coef = rng.uniform(-2, 2, 32)
        _same(eng.lincomb([p[0] for p in pairs], coef, 0.37), rev.lincomb([p[1] for p in pairs], coef, 0.37), (corner, ell))


def test_n17_rotation(corner_engine, orc):
    """the largest ring (N = 2^17): one rotation at the top level"""
    eng = corner_engine("n17")
    k = _evk(orc, eng, 77)
    eng.key_import(1, 3, k)
    x = _ct(orc, eng, 5, eng.n_q)
    want = orc.rotate(x, k, orc.galois(eng.log_n, 3), eng.alpha, eng.q, eng.p, eng.psi_q, eng.psi_p)
    assert np.array_equal(eng.raw_rotate(eng.ct_import(x), 3).export(), want)


def test_k0_refuses_key_switching(corner_engine, orc, fa):
    """n_p = 0: additions run, every key switch is refused with FHELIN_ERR_STATE (4) and nothing is launched for it"""
    eng = corner_engine("k0")
    rev = _rev(eng, {})
    a, b = (_imp(eng, rev, _ct(orc, eng, s, eng.n_q)) for s in (1, 2))
    _same(eng.add(a[0], b[0]), rev.add(a[1], b[1]), "add")
    eng.key_import(1, 1, _evk(orc, eng, 3))
    eng.key_import(0, 0, _evk(orc, eng, 4))
    for op in (lambda: eng.raw_rotate(a[0], 1), lambda: eng.rotate_sum([a[0]], [1]), lambda: eng.raw_mult_relin(a[0], b[0]),
               lambda: eng.rotate_batch([a[0], b[0]], 1)):
        with pytest.raises(fa.FhelinError) as ei:
            op()
        assert ei.value.code == 4, str(ei.value)


# ---- operands at the accumulation bounds

def _extreme(eng, orc, target):
    """a 2-component ciphertext whose limbs are the constant min(q_j, target) - 1 (a constant in NTT form is a constant polynomial:
    at alpha = 1 the ModUp hands every target limb min(q_j, target) - 1 itself)"""
    v = np.stack([np.full(eng.N, min(int(m), target) - 1, dtype=np.uint64) for m in eng.q])
    return np.stack([v, v])


@pytest.mark.parametrize("corner", ["a1_b16", "a16_k16", "k15", "p60", "p60_a1"])
@pytest.mark.parametrize("form", ["plain", "montgomery"])
def test_extreme_operands(corner_engine, orc, corner, form):
    """near-maximal keys (see _max_evk for which form is maximal in which kernel) and ciphertext limbs at min(q_j, target) - 1:
    the Acc30 flush groups and Montgomery-finished sums of ks_inner (beta = 16), ModDown with 16 sources, the merged ModDown + rescale
    with 16 sources, 60-bit limbs in all of them, and (p60_a1) ks_inner_multi's fold every 16 products: at alpha = 1 every ModUp digit
    for a special target m is the constant min(q_j, m) - 1 itself, and rotate_sum's 7 * 4 products per output sum to about
    1.09 m 2^64, so only the fold keeps the final Montgomery reduction's input below m 2^64"""
    eng = corner_engine(corner, "no_finish")          # a context of its own: its keys are the maximal ones
    mx = _max_evk(eng, form)
    eng.key_import(0, 0, mx)
    for r in IDX:
        eng.key_import(1, r, mx)
    rev = _rev(eng, {r: mx for r in IDX})
    args = (eng.alpha, eng.q, eng.p, eng.psi_q, eng.psi_p)
    ga = lambda r: orc.galois(eng.log_n, r)
    pts = [eng.encode(np.full(1 << eng.params.log_slots, -0.999)) for _ in range(4)]
    encs = [(lambda p: (lambda ell, sc: eng.pt_export(p, ell, sc)))(p) for p in pts]
    for target in sorted({int(max(eng.moduli)), int(min(eng.p)), int(eng.q[0])}):
        for ell in sorted({eng.n_q, 2}, reverse=True):
            what = (corner, form, hex(target), ell)
            x = np.ascontiguousarray(_extreme(eng, orc, target)[:, :ell])
            assert np.array_equal(eng.raw_rotate(eng.ct_import(x), 1).export(), orc.rotate(x, mx, ga(1), *args)), what
            y = x.copy()
            y[1] = 1                                       # the relinearised component a1 * b1 = q - 1 as well
            assert np.array_equal(eng.raw_mult_relin(eng.ct_import(x), eng.ct_import(y)).export(),
                                  orc.mult_relin(x, y, mx, *args)), what
            c, r = _imp(eng, rev, x)
            got = eng.rotate_sum([c, c], IDX)
            want = orc.rotate_sum(x, np.stack([mx] * len(IDX)), [ga(i) for i in IDX], *args)
            for g in got:
                assert np.array_equal(g.export(), want), what + ("rotate_sum",)
            for rescale in (False, True):
                g = eng.hoisted_dot([c], pts, [1, 2, 3], rescale=rescale)[0]
                if rescale and eng.n_p + 1 > 16:
                    want = rev.rescale(rev.hoisted_dot(r, encs, [1, 2, 3], rescale=False))
                else:
                    want = rev.hoisted_dot(r, encs, [1, 2, 3], rescale=rescale)
                _same(g, want, what + ("hoisted_dot", rescale))
    if corner == "p60":
        for ell in (eng.n_q, 3):
            x = np.ascontiguousarray(_extreme(eng, orc, 1 << 62)[:, :ell])
            pairs = [_imp(eng, rev, x) for _ in range(32)]
            coef = np.full(32, -2.0 ** -40)                # per-limb scalars q - round(2^-40 Delta): close to q
            _same(eng.lincomb([p[0] for p in pairs], coef), rev.lincomb([p[1] for p in pairs], coef, 0.0), ("lincomb", ell))


def test_sixty_bit_reference_ring_slot_kernels(fa, orc):
    """the kernels that need a slot layout, on a 60-bit chain at the reference ring (N = 2^15, 16384 slots): wrapUpRepeated over 32
    ciphertexts at q - 1 (ew_dot_kernel: 32 products before one reduction, q - 1 on the ciphertext side, the encoder's block masks on
    the plaintext side) and matmulRElarge with rows at q - 1, read directly and through generate_containers (ew_cyclic_dot_kernel on its
    30-bit split path with NINE of its 32 columns live: no output sums more than nine products, so neither a second flush of eight nor
    the fold after sixteen carries anything here).  The full sums - 32 live columns, plaintext residues at their extremes too - are in
    tests/test_dot_kernels_gpu.py"""
    eng = fa.Engine("reference", seed=3, n_q=6, n_p=2, dnum=3, first_bits=60, scale_bits=59)
    try:
        assert int(eng.q[0]).bit_length() == 60
        rev = _rev(eng, {})
        ns = 1 << eng.params.log_slots
        ell = eng.n_q
        mx = np.ascontiguousarray(_extreme(eng, orc, 1 << 62))
        pairs = [_imp(eng, rev, mx) for _ in range(32)]
        got = eng.wrapUpRepeated([p[0] for p in pairs])
        acc = None
        for i, (_, r) in enumerate(pairs):
            m = np.zeros(ns)
            m[128 * i:128 * (i + 1)] = 1.0
            pt = eng.encode(m)
            t = rev.mult_plain(r, lambda e, sc: eng.pt_export(pt, e, sc))
            acc = t if acc is None else rev.add(acc, t)
        _same(got, acc, "wrapUpRepeated at q - 1")
        need = {128, 256, 384, 8192, 1024, 4096, 12288, 512, 1536, 2048, 3072, 6144, 2560, 3584}
        keys = {r: _evk(orc, eng, 100 + 17 * r) for r in sorted(need)}
        for r, k in keys.items():
            eng.key_import(1, r, k)
        keys[-4096] = keys[12288]
        rev = _rev(eng, keys)
        rng = np.random.default_rng(9)
        pt = lambda v: eng.encode(v)
        enc_of = lambda p: (lambda e, sc: eng.pt_export(p, e, sc))
        wv = [rng.uniform(-1, 1, ns) / 8 for _ in range(4)]
        ws = [pt(v) for v in wv]
        bias_values = rng.uniform(-1, 1, ns)
        bias = pt(bias_values)
        w2 = []
        for t in range(4):
            v = np.zeros(ns)
            for b in range(128):
                v[128 * b:128 * (b + 1)] = wv[(b - t) % 4][128 * b:128 * (b + 1)]
            w2.append(enc_of(pt(np.roll(v, -128 * t))))
        m512 = np.zeros(ns)
        m512[:512] = 0.5
        rows = [_imp(eng, rev, mx) for _ in range(2)]
        for o, r in zip(eng.matmulRElarge([c[0] for c in rows], ws, bias, 0.5),
                        rev.matmulRElarge([c[1] for c in rows], w2, enc_of(bias), enc_of(pt(m512)))):
            _same(o, r, "matmulRElarge at q - 1")
        rows9 = [_imp(eng, rev, mx) for _ in range(9)]
        got = eng.generate_containers(eng.matmulRElarge([c[0] for c in rows9], ws, bias, 0.5))
        assert len(got) == 1
        masks = []
        for j in range(32):
            m = np.zeros(ns)
            m[512 * j:512 * (j + 1)] = 0.5
            masks.append(enc_of(pt(m)))
        tiled = np.zeros(ns)
        for i in range(9):
            tiled += np.roll(bias_values, 512 * i)
        us = [rev.relarge_u(c[1], w2) for c in rows9]
        _same(got[0], rev.relarge_container(us, masks, enc_of(pt(tiled))), "fused containers at q - 1")
    finally:
        eng.close()
