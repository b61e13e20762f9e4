"""Q-limb inner products formed in the ModDown's forward NTT row pass (FHELIN_FUSE_ACCQ_ROWS): for the single-key forms whose
ModDown ends in the row pass of NTT(conv), no inner-product launch runs and accQ is never stored - ntt_rows_epilogue_product_kernel forms
the sums where the epilogue used to read them back.  Residues do not change, so every check is an equality, taken two ways: against the
oracle, and against an engine created with FHELIN_FUSE_ACCQ_ROWS=0 (launch_ks_inner and the accQ round trip) that holds the same keys.

Rings and levels are those of test_special_limb_rows_gpu.py: N = 2^12 (one row tile per vector) and 2^13 (two), one case at N = 2^16;
ell = 1, 2, alpha, alpha + 1 and the full chain (one digit whose own-limb slot is the only term, a short last digit, two digits); a 52-bit
special-prime chain.  The engines with the knob on are created with it at 2 (every class that is built); one case runs at the default 1.
The crafted cases reach the kernel's operands directly (fhelin_debug_ks_accq): every digit, own limb and key residue at its maximum (a
dnum = 7 chain puts seven terms into one sum), an all-zero digit under a maximal key, conv = 0 and conv maximal, and uniform operands
against sums formed by the oracle's dyadic functions."""
import numpy as np
import pytest

from test_default_path_gpu import _ct, _evk, _imp, _rev
from test_special_limb_rows_gpu import RINGS, ROTS, _cases, _eq, _limb_transforms

pytestmark = pytest.mark.gpu
LD = np.longdouble
KNOB = "FHELIN_FUSE_ACCQ_ROWS"
_PAIRS = {}


def _engine(fa, knob, preset, **kw):
    mp = pytest.MonkeyPatch()
    try:
        if knob is not None:
            mp.setenv(KNOB, str(knob))
            mp.setenv("FHELIN_ACCQ_ROWS_MIN_VECS", "0")
        else:
            mp.delenv(KNOB, raising=False)
        return fa.Engine(preset, **kw)
    finally:
        mp.undo()


@pytest.fixture(scope="module")
def pairs(fa, orc):
    """get(name) -> (engine whose row pass forms the Q-limb sums, engine with the separate launches, rotation keys, relinearisation key,
    ResidueEvaluator): the same uniform 'keys' in both (parity of integer functions needs no real keys), made once per ring"""
    def get(name):
        if name not in _PAIRS:
            preset, over, _ = RINGS[name]
            on, off = _engine(fa, 2, preset, **over), _engine(fa, 0, preset, **over)
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


def _rot(orc, e, keys, x, r):
    return orc.rotate(x, keys[r], orc.galois(e.log_n, r), e.alpha, e.q, e.p, e.psi_q, e.psi_p)


@pytest.mark.parametrize("name,ell", _cases(["n12", "n13", "n13_lazy", "n16"]))
def test_relinearisation(pairs, orc, name, ell):
    """the identity form (ks_inner_kernel<false>'s operands: keys as stored, digits times 2^64, the own limb through t.mont), one ciphertext
    and a batch of three; limb_ntt equal with the knob on and off"""
    on, off, keys, relin, rev = pairs(name)
    a = [_ct(orc, on, 900 + 7 * i + ell, ell) for i in range(3)]
    b = [_ct(orc, on, 950 + 7 * i + ell, ell) for i in range(3)]
    want = [orc.mult_relin(x, y, relin, on.alpha, on.q, on.p, on.psi_q, on.psi_p) for x, y in zip(a, b)]
    for e in (on, off):
        _eq(e.raw_mult_relin(e.ct_import(a[0]), e.ct_import(b[0])).export(), want[0], (name, ell, e is on, "one"))
        got = e.mult_batch([_imp(e, rev, x)[0] for x in a], [_imp(e, rev, y)[0] for y in b])
        for i, g in enumerate(got):
            _eq(g.export(), want[i], (name, ell, e is on, "batch of 3", i))
    n_on = _limb_transforms(on, lambda: on.raw_mult_relin(on.ct_import(a[0]), on.ct_import(b[0])))
    n_off = _limb_transforms(off, lambda: off.raw_mult_relin(off.ct_import(a[0]), off.ct_import(b[0])))
    assert n_on == n_off and n_on > 0, (n_on, n_off)


@pytest.mark.parametrize("name,ell", _cases(["n12", "n13", "n13_lazy", "n16"]))
def test_plain_rotations(pairs, orc, name, ell):
    """gathered (ks_inner_kernel<true>'s operands: digits, own limb and c0 through the row's map, the permuted pre-split key, + P * c0): an
    index that moves the 512-coefficient tiles, one that keeps them in place, a negative one; one ciphertext, a batch of three, and
    rotate_add (rotsum over one step: x + rot(x, r)); limb_ntt equal with the knob on and off"""
    on, off, keys, relin, rev = pairs(name)
    rots = [1, 64, -1] if name != "n16" else [1]
    xs = [_ct(orc, on, 300 + 7 * i + ell, ell) for i in range(3)]
    for r in rots:
        want = [_rot(orc, on, keys, x, r) for x in xs]
        for e in (on, off):
            _eq(e.raw_rotate(e.ct_import(xs[0]), r).export(), want[0], (name, ell, r, e is on, "one"))
            for i, g in enumerate(e.rotate_batch([e.ct_import(x) for x in xs], r)):
                _eq(g.export(), want[i], (name, ell, r, e is on, "batch of 3", i))
            if r > 0:
                added = np.stack([orc.add(xs[0][p], want[0][p], on.q[:ell]) for p in range(2)])
                _eq(e.rotsum(e.ct_import(xs[0]), 2, r).export(), added, (name, ell, r, e is on, "rotate_add"))
    n_on = _limb_transforms(on, lambda: on.raw_rotate(on.ct_import(xs[0]), rots[0]))
    n_off = _limb_transforms(off, lambda: off.raw_rotate(off.ct_import(xs[0]), rots[0]))
    assert n_on == n_off and n_on > 0, (n_on, n_off)


@pytest.mark.parametrize("name,ell", _cases(["n12", "n13"]))
def test_rows_with_their_own_keys(pairs, orc, name, ell):
    """per-row keys and maps over a shared input: rotate_many with 1, 2 and 7 indices, rotate_each (rows with their own inputs), and two
    inputs in one launch (row_mod)"""
    on, off, keys, relin, rev = pairs(name)
    xs = [_ct(orc, on, 410 + 3 * i + ell, ell) for i in range(3)]
    want = {(i, r): _rot(orc, on, keys, xs[i], r) for i in range(2) for r in range(1, 8) if i == 0 or r in (2, 5)}
    each = [_rot(orc, on, keys, x, r) for x, r in zip(xs, [64, -1, 3])]
    for e in (on, off):
        for idx in ([3], [1, 2], [1, 2, 3, 4, 5, 6, 7]):
            for r, g in zip(idx, e.rotate_many(e.ct_import(xs[0]), idx)):
                _eq(g.export(), want[0, r], (name, ell, e is on, "rotate_many", len(idx), r))
        for i, g in enumerate(e.rotate_each([e.ct_import(x) for x in xs], [64, -1, 3])):
            _eq(g.export(), each[i], (name, ell, e is on, "rotate_each", i))
        cs = [_imp(e, rev, x)[0] for x in xs[:2]]
        for i, outs in enumerate(e.debug_rotate_many_batch(cs, [2, 5])):
            for r, g in zip([2, 5], outs):
                _eq(g.export(), want[i, r], (name, ell, e is on, "two inputs", i, r))


def test_the_default_knob(fa, orc, pairs):
    """FHELIN_FUSE_ACCQ_ROWS unset (1: the classes of the measured table): a relinearisation, a rotation and rows with their own keys at
    N = 2^13 against the oracle"""
    on, off, keys, relin, rev = pairs("n13")
    e = _engine(fa, None, "toy13")
    try:
        e.key_import(0, 0, relin)
        for r in (1, 2, 3):
            e.key_import(1, r, keys[r])
        for ell in (2, 7):
            a, b = _ct(orc, e, 901 + ell, ell), _ct(orc, e, 951 + ell, ell)
            _eq(e.raw_mult_relin(e.ct_import(a), e.ct_import(b)).export(),
                orc.mult_relin(a, b, relin, e.alpha, e.q, e.p, e.psi_q, e.psi_p), ("relin", ell))
            _eq(e.raw_rotate(e.ct_import(a), 1).export(), _rot(orc, e, keys, a, 1), ("rotate", ell))
            for r, g in zip([1, 2, 3], e.rotate_many(e.ct_import(b), [1, 2, 3])):
                _eq(g.export(), _rot(orc, e, keys, b, r), ("rotate_many", ell, r))
    finally:
        e.close()


# ------------------------------------------------------------------------------------------------ crafted operands, at the kernel
def _pinv(e, ell):
    P = 1
    for m in e.p:
        P *= int(m)
    return np.array([pow(P % int(m), -1, int(m)) for m in e.q[:ell]], dtype=np.uint64)


def _accq_want(orc, e, ell, digits, own, conv, key, g):
    """(acc - NTT(conv)) * P^-1 with acc from the oracle's dyadic functions; g = None: the identity form, whose digit terms come times 2^-64"""
    q = [int(m) for m in e.q[:ell]]
    beta = digits.shape[1]
    r2inv = np.array([pow(1 << 64, -1, m) for m in q], dtype=np.uint64)
    own_key = lambda c: np.stack([key[t // e.alpha, c, t] for t in range(ell)])
    out = np.empty((digits.shape[0], 2, ell, e.N), dtype=np.uint64)
    for b in range(digits.shape[0]):
        d = digits[b, :, :ell].copy()
        for t in range(ell):
            d[t // e.alpha, t] = 0          # the own-digit slot is not read
        for c in range(2):
            s = orc.dot([d[j] for j in range(beta)], [key[j, c, :ell] for j in range(beta)], q)
            if g is None:
                s = orc.mul_scalar(s, r2inv, q)
            s = orc.add(s, orc.mul(own[b], own_key(c), q), q)
            if g is not None:
                s = np.stack([orc.automorph_ntt(s[t], g) for t in range(ell)])
            x = orc.ntt_batch(conv[b, c], q, e.psi_q[:ell])
            out[b, c] = orc.mul_scalar(orc.sub(s, x, q), _pinv(e, ell), q)
    return out


@pytest.mark.parametrize("name,ell,index,batch", [
    ("n12", 6, 0, 1), ("n12", 3, 0, 2), ("n12", 1, 1, 1), ("n13", 7, 0, 1), ("n13", 4, 1, 2), ("n13", 7, 64, 1), ("n13", 4, -1, 3),
    ("n13_lazy", 7, 0, 1), ("n13_lazy", 7, 1, 1), ("n16", 2, 0, 1), ("n16", 2, 1, 1)])
def test_uniform_operands_at_the_kernel(pairs, orc, name, ell, index, batch):
    """the fused row pass on operands of the caller's choice: uniform canonical digits, own limb and conv against the oracle's sums"""
    on, off, keys, relin, rev = pairs(name)
    beta, nt = -(-ell // on.alpha), ell + on.n_p
    mods = np.concatenate([np.asarray(on.q[:ell], dtype=np.uint64), np.asarray(on.p, dtype=np.uint64)])
    d = np.stack([orc.uniform_residues(5000 + 13 * i, mods, on.N) for i in range(batch * beta)]).reshape(batch, beta, nt, on.N)
    own = np.stack([orc.uniform_residues(6000 + 13 * i, on.q[:ell], on.N) for i in range(batch)])
    conv = np.stack([orc.uniform_residues(7000 + 13 * i, on.q[:ell], on.N) for i in range(2 * batch)]).reshape(batch, 2, ell, on.N)
    want = _accq_want(orc, on, ell, d, own, conv, keys[index] if index else relin, orc.galois(on.log_n, index) if index else None)
    for e in (on, off):
        _eq(e.debug_ks_accq(d, own, conv, ell, index), want, (name, ell, index, e is on))


MAXIMAL = dict(RINGS, n13_d7=("toy13", {"dnum": 7}, [7]))     # alpha = 1: seven digits, six digit terms and the own limb in every sum


@pytest.mark.parametrize("name,ell,index", [("n13", 7, 0), ("n13", 7, 1), ("n13", 1, 1), ("n13_lazy", 7, 0), ("n12", 6, 64),
                                            ("n13_d7", 7, 0), ("n13_d7", 7, 1)])
def test_maximal_operands(fa, orc, name, ell, index):
    """every key residue m - 1, the own limb q - 1 and every digit at the largest value its class hands over: q - 1, or 86q - 1 where the
    lazy forward transform leaves digits unreduced (q < 2^53); conv = 0 and every coefficient of conv at q - 1.  Then all-zero digits and
    an all-zero own limb under the same maximal key.  Expected: the constant vector of the sum minus NTT(conv), times P^-1."""
    preset, over, _ = MAXIMAL[name]
    on, off = _engine(fa, 2, preset, **over), _engine(fa, 0, preset, **over)
    try:
        beta, nt = -(-ell // on.alpha), ell + on.n_p
        mods = [int(v) for v in on.moduli]
        top = np.stack([np.full(on.N, m - 1, dtype=np.uint64) for m in mods])
        key = np.broadcast_to(top, (on.dnum_digits, 2) + top.shape).copy()
        for e in (on, off):
            e.key_import(0, 0, key)
            if index:
                e.key_import(1, index, key)
        q = [int(v) for v in on.q[:ell]]
        dmax = [(86 * m if m < (1 << 53) else m) - 1 for m in q]
        for zero in (False, True):
            d = np.zeros((1, beta, nt, on.N), dtype=np.uint64)
            own = np.zeros((1, ell, on.N), dtype=np.uint64)
            if not zero:
                for t in range(ell):
                    d[:, :, t, :] = dmax[t]
                    own[:, t, :] = q[t] - 1
            r2 = lambda m: 1 if index else pow(1 << 64, -1, m)
            const = [0 if zero else ((beta - 1) * dmax[t] * (m - 1) * r2(m) + (m - 1) * (m - 1)) % m for t, m in enumerate(q)]
            acc = np.stack([np.full(on.N, v, dtype=np.uint64) for v in const])
            for conv_max in (False, True):
                cv = np.stack([np.full(on.N, m - 1 if conv_max else 0, dtype=np.uint64) for m in q])
                want = orc.mul_scalar(orc.sub(acc, orc.ntt_batch(cv, q, on.psi_q[:ell]), q), _pinv(on, ell), q)
                conv = np.broadcast_to(cv, (1, 2) + cv.shape).copy()
                for e in (on, off):
                    got = e.debug_ks_accq(d, own, conv, ell, index)
                    for c in range(2):
                        _eq(got[0, c], want, (name, ell, index, zero, conv_max, e is on, c))
    finally:
        on.close()
        off.close()


# ------------------------------------------------------------------------------------------------ the conjugation key, through a bootstrap
def test_bootstrap_agrees_with_the_separate_launches(fa):
    """one bootstrap at N = 2^12 with real keys: baby steps (rows with their own keys in one launch), the conjugation key's gathered switch,
    EvalMod's relinearisations - byte for byte on both engines"""
    es = []
    try:
        for knob in (2, 0):
            e = _engine(fa, knob, "boot12", seed=99, log_slots=10)
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
