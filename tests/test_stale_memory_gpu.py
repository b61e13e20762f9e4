"""No result may depend on what pool memory held before the call (DESIGN.md "Pool fill").

All device memory comes from DevicePool, which recycles ranges in stream order and never clears them; every accumulator, conversion buffer
and digit block has to be written by a kernel before anything reads it.  Under FHELIN_POOL_FILL=<w> the pool hands out every block with w
in each 32-bit word, so a kernel that consumes memory nobody wrote computes from w.  Every scenario here runs on THREE engines of equal
arguments and seed - knob off, w = 1, w = 2 - with identical inputs, and

  * every array it returns (exported residues, ciphertext shape and scale parts, decrypted doubles as raw bytes, file bytes) is equal on
    the three engines, byte for byte,
  * where the oracle defines the result, engine 1's arrays equal the oracle's residue for residue,
  * every operand exports after the scenario what it exported before - ciphertext handles, the plaintext encodings an operation reads
    and the evaluation keys it uses (no kernel used an input block as scratch),
  * the pool's fill counters rose on engines 2 and 3 during the scenario and are 0 on engine 1 (the knob was really on / off),

and then runs again on the same engines with other input seeds, when the pool's ranges have been used once and are being recycled.
No tolerance is involved in any of these comparisons.  What the method cannot see is listed in DESIGN.md."""
import numpy as np
import pytest

from stale_memory import LD, WORDS, keys_for, make_trios, relin_for, run
from test_default_path_gpu import _ct, _imp
from test_linear_transform_gpu import _absent, _oracle as _lt_oracle, _terms

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def trios(fa):
    """(preset, overrides) -> [engine with the knob off, with w = 1, with w = 2]: the same arguments and the same non-zero seed"""
    yield from make_trios(fa)


# ------------------------------------------------------------------------------------------------ the knob itself, on the device
def test_a_handed_out_block_reads_back_as_w(trios, fa):
    """fhelin_dev_alloc -> DevicePool::alloc: every word of a fresh block is w (one block of each granule class, an odd size, and a block
    that re-uses a range a kernel-free upload has just written and freed)"""
    for w, eng in zip(WORDS, trios("toy")):
        before = eng.pool_fill_stats()
        for nbytes in (256, 4 * 1000, 8 * eng.N, (64 << 10) + 4096 * 3):
            buf = eng.buf(nbytes)
            if w:
                got = buf.download((nbytes // 4,), dtype=np.uint32)
                assert np.array_equal(got, np.full(nbytes // 4, w, dtype=np.uint32)), (w, nbytes)
            buf.upload(np.full(nbytes // 4, 0xDEADBEEF, dtype=np.uint32))
            buf.free()
            again = eng.buf(nbytes)                         # best fit hands the same range out again
            if w:
                got = again.download((nbytes // 4,), dtype=np.uint32)
                assert np.array_equal(got, np.full(nbytes // 4, w, dtype=np.uint32)), ("recycled", w, nbytes)
            again.free()
        after = eng.pool_fill_stats()
        if w:
            assert after[0] - before[0] == 8
            assert after[1] - before[1] == 2 * (256 + 4096 + 8 * eng.N + (64 << 10) + 4096 * 3)     # rounded: 4000 -> 4096
        else:
            assert before == after == (0, 0)


# ------------------------------------------------------------------------------------------------ evaluator scenarios (oracle-anchored)
@pytest.mark.parametrize("ell", [6, 5, 3, 2])
def test_plain_rotation(trios, orc, ell):
    """toy, alpha = 2: a full digit, a short last digit, a single digit - both bodies of modup_body and the gather path"""
    def scen(s):
        keys = keys_for(s, [1, 3], 9000)
        rev = s.rev(keys)
        for i, r in enumerate((1, 3)):
            c, x = s.imp(rev, _ct(s.orc, s.eng, s.seed(300 + 7 * i + ell), ell))
            s.out(f"rotate {r}", s.eng.rotate(c, r), lambda: rev.rotate(x, r))
    run(trios("toy"), orc, scen)


def test_hoisted_rotations_past_one_launch(trios, orc):
    """toy13, ell 5, 18 hoisted indices - more than KsShape::MAX_ROWS - of 2 inputs behind one ModUp (Evaluator::rotate_many_batch through
    its test hook: per input and per chunk of 16 rows, accQ / accP / conv / ext offset by row and input); 3 indices of the 2 inputs in one
    launch (row_mod), index 0 handing the input itself back; and the 18 of one input alone (rotate_many's own chunks)"""
    idx = list(range(1, 19))

    def scen(s):
        keys = keys_for(s, idx, 9100, watch=(1, 16, 17, 18))          # the keys at the chunk boundary
        rev = s.rev(keys)
        pairs = [s.imp(rev, _ct(s.orc, s.eng, s.seed(410 + 3 * i), 5)) for i in range(2)]
        cs = [c for c, _ in pairs]
        made = {}

        def want(i, r):                                               # every index is anchored; the oracle rotates once per (input, index)
            if (i, r) not in made:
                made[(i, r)] = rev.rotate(pairs[i][1], r)
            return made[(i, r)]
        for i, outs in enumerate(s.eng.debug_rotate_many_batch(cs, idx)):
            for r, o in zip(idx, outs):
                s.out(f"batch of 2, input {i} rotation {r}", o, lambda i=i, r=r: want(i, r))
        for i, outs in enumerate(s.eng.debug_rotate_many_batch(cs, [0, 2, 5])):
            for r, o in zip([0, 2, 5], outs):
                s.out(f"one launch, input {i} rotation {r}", o, (lambda i=i, r=r: want(i, r)) if r else pairs[i][1])
        for r, o in zip(idx, s.eng.rotate_many(cs[1], idx)):
            s.out(f"one input, rotation {r}", o, lambda r=r: want(1, r))
    run(trios("toy13"), orc, scen)


@pytest.mark.parametrize("idx,rows", [
    ([-2], 1),                               # a single merged term
    ([1, 2], 3),                             # an odd row count: the switched-off partner of the ROWS = 2 kernel
    ([1, 2, 3, 4, 5, 6, 7], 2),              # the kernel's maximum
    ([64, 128, 192], 3),                     # every 512-coefficient tile stays in place: digit tiles staged in LDS
    ([1, 2, 3], 1),                          # ... and one that moves them
])
def test_merged_rotation_sum(trios, orc, idx, rows):
    def scen(s):
        keys = keys_for(s, idx, 9000)
        eng = s.eng
        evks = np.stack([keys[r] for r in idx])
        gs = [s.orc.galois(eng.log_n, r) for r in idx]
        for ell in (5, 2):
            xs = [_ct(s.orc, eng, s.seed(300 + 7 * i + ell), ell) for i in range(rows)]
            cs = [s.operand(eng.ct_import(x)) for x in xs]
            for i, (x, g) in enumerate(zip(xs, eng.rotate_sum(cs, idx))):
                s.out(f"ell {ell} row {i}", g, lambda x=x: s.orc.rotate_sum(x, evks, gs, eng.alpha, eng.q, eng.p, eng.psi_q, eng.psi_p))
    run(trios("toy13"), orc, scen)


@pytest.mark.parametrize("ell,idx", [
    (7, [1, 2, 0, 4, 8, 16, 32, 64]),        # an unrotated addend + exactly 7 rotated terms
    (5, [1, 2, 4, 8, 16, 32, 64, 128]),      # 8 terms: a group of 7 and one leftover through a plain rotation
    (3, [1, 2]),
])
def test_rotate_each_sum(trios, orc, ell, idx):
    def scen(s):
        keys = keys_for(s, [r for r in idx if r], 4000)
        rev = s.rev(keys)
        pairs = [s.imp(rev, _ct(s.orc, s.eng, s.seed(800 + 3 * i), ell)) for i in range(len(idx))]
        s.out("rotate_each_sum", s.eng.rotate_each_sum([p[0] for p in pairs], idx), lambda: rev.rotate_each_sum([p[1] for p in pairs], idx))
    run(trios("toy13"), orc, scen)


@pytest.mark.parametrize("deg", [1, 2])
def test_hoisted_dot(trios, orc, deg):
    """fold_key, hoist_addends with and without an accumulator, the ModDown merged with the rescale"""
    idx = [1, 2, 3]

    def scen(s):
        eng = s.eng
        keys = keys_for(s, idx, 6100)
        rev = s.rev(keys)
        rng = np.random.default_rng(s.seed(77))
        ns = 1 << eng.params.log_slots
        pts = [eng.encode(rng.uniform(-1, 1, ns)) for _ in range(len(idx) + 1)]
        encs = [(lambda p: (lambda ell, sc: eng.pt_export(p, ell, sc)))(p) for p in pts]
        for ell in (6, 3):
            at = ell - (deg - 1)                                # a degree-2 operand is rescaled first
            s.plain(pts[0], [(at, 0.0)], "unrotated term's plaintext")
            for r, p in zip(idx, pts[1:]):                      # folded into the key: over the full key basis at that level's scale
                s.plain(p, [(eng.n_q + eng.n_p, rev.sf[eng.n_q - at])], f"plaintext of rotation {r}")
            pairs = [s.imp(rev, _ct(s.orc, eng, s.seed(500 + 7 * i + ell), ell), deg=deg) for i in range(2)]
            for rescale in (False, True):
                got = eng.hoisted_dot([p[0] for p in pairs], pts, idx, rescale=rescale)
                for i, ((c, r), g) in enumerate(zip(pairs, got)):
                    s.out(f"ell {ell} rescale {rescale} row {i}", g, lambda r=r: rev.hoisted_dot(r, encs, idx, rescale=rescale))
    run(trios("toy"), orc, scen)


@pytest.mark.parametrize("ell", [6, 3, 1])
def test_mult_relin(trios, orc, ell):
    def scen(s):
        eng = s.eng
        relin = relin_for(s)
        a = _ct(s.orc, eng, s.seed(900 + ell), ell)
        b = _ct(s.orc, eng, s.seed(950 + ell), ell)
        ca, cb = s.operand(eng.ct_import(a)), s.operand(eng.ct_import(b))
        s.out("mult", eng.mult(ca, cb), lambda: s.orc.mult_relin(a, b, relin, eng.alpha, eng.q, eng.p, eng.psi_q, eng.psi_p))
    run(trios("toy"), orc, scen)


def test_mult_affine_batch_exact_tail(trios, orc):
    """the exact merged tail (AffineItems, accp_limbs = k + 1): items that differ in factor, constant, addend and sign"""
    from oracle.residue_eval import RCt

    def scen(s):
        eng = s.eng
        relin = relin_for(s)
        rev = s.rev({"relin": relin})
        n_q, ell = len(eng.q), 3

        def val(sd, limbs, deg=1):
            sc = LD(float(rev.sf[n_q - limbs]))
            if deg == 2:
                sc = LD(float(sc * sc))
            x = _ct(s.orc, eng, s.seed(7000 + sd), limbs)
            return s.operand(eng.ct_import(x, deg=deg, scale=float(sc))), RCt(x, deg, sc)
        t1, t2, aa = val(1, ell + 1), val(2, ell), val(4, ell, 2)
        items = [(t2, t2, 2, -1.0, None, False), (t1, t2, 2, 0.0, t1, True), (t2, t2, 1, 0.0, aa, False)]
        got = eng.mult_affine_batch([i[0][0] for i in items], [i[1][0] for i in items], [i[2] for i in items], [i[3] for i in items],
                                    [i[4][0] if i[4] else None for i in items], [i[5] for i in items])

        def want(a, b, f, cadd, ad, neg):
            t = rev.mult(a[1], b[1])
            if f == 2:
                t = rev.add(t, t)
            if cadd != 0.0:
                t = rev.add_real(t, cadd)
            if ad is not None:
                t = rev.sub(t, ad[1]) if neg else rev.add(t, ad[1])
            return rev.rescale(t)
        for k, (it, g) in enumerate(zip(items, got)):
            s.out(f"item {k}", g, lambda it=it: want(*it))
    run(trios("toy13"), orc, scen)


def test_rescale(trios, orc):
    """2 and 3 components, ell = 2 -> 1 included"""
    def scen(s):
        eng = s.eng
        rev = s.rev({})
        for ell, npoly in ((6, 2), (2, 2), (4, 3), (2, 3)):
            x = _ct(s.orc, eng, s.seed(40 + 10 * ell + npoly), ell, npoly)
            c = s.operand(eng.ct_import(x))
            s.out(f"raw_rescale ell {ell} npoly {npoly}", eng.raw_rescale(c), lambda: s.orc.rescale(x, eng.q[:ell], eng.psi_q[:ell]))
        xs = [_imp(eng, rev, _ct(s.orc, eng, s.seed(60 + i), 5), deg=2) for i in range(3)]
        for c, _ in xs:
            s.operand(c)
        for i, (g, (_, r)) in enumerate(zip(eng.rescale_batch([c for c, _ in xs]), xs)):
            s.out(f"rescale_batch row {i}", g, lambda r=r: rev.rescale(r))
    run(trios("toy"), orc, scen)


def test_smaller_ops(trios, orc):
    """batched level and degree adjustment (ew_scalar_items), real-constant ops, lincomb with n = 5 and n = 1, ModRaise 3 -> 7"""
    def scen(s):
        eng = s.eng
        rev = s.rev({})
        L1 = len(eng.q)
        a, ra = s.imp(rev, _ct(s.orc, eng, s.seed(1), L1))
        b, rb = s.imp(rev, _ct(s.orc, eng, s.seed(2), L1 - 2))
        c2, rc2 = s.imp(rev, _ct(s.orc, eng, s.seed(3), L1 - 4), deg=2)
        d2, rd2 = s.imp(rev, _ct(s.orc, eng, s.seed(4), L1), deg=2)
        s.out("add two levels apart", eng.add(a, b), lambda: rev.add(ra, rb))
        s.out("sub swapped", eng.sub(b, a), lambda: rev.sub(rb, ra))
        s.out("deg1 + deeper deg2", eng.add(a, c2), lambda: rev.add(ra, rc2))
        s.out("deg2 with more limbs", eng.add(d2, b), lambda: rev.add(rd2, rb))
        pairs = [(a, b), (b, a), (a, c2), (d2, b), (a, d2)]
        wants = [(ra, rb), (rb, ra), (ra, rc2), (rd2, rb), (ra, rd2)]
        for k, (g, (x, y)) in enumerate(zip(eng.add_batch([p[0] for p in pairs], [p[1] for p in pairs]), wants)):
            s.out(f"add_batch {k}", g, lambda x=x, y=y: rev.add(x, y))
        for cst in (0.7310585786300049, -1.25e-3):
            s.out(f"mult_real {cst}", eng.mult_real(b, cst), lambda: rev.mult_real(rb, cst))
            s.out(f"add_real {cst}", eng.add_real(b, cst), lambda: rev.add_real(rb, cst))
        rng = np.random.default_rng(s.seed(8))
        for n in (5, 1):
            terms = [s.imp(rev, _ct(s.orc, eng, s.seed(700 + i), 6)) for i in range(n)]
            coef = rng.uniform(-2, 2, n)
            if n > 3:
                coef[2] = 0.0
            s.out(f"lincomb {n}", eng.lincomb([t[0] for t in terms], coef, 0.37), lambda: rev.lincomb([t[1] for t in terms], coef, 0.37))
        x = _ct(s.orc, eng, s.seed(77), 1)
        c = s.operand(eng.ct_import(x))
        s.out("modraise 1 -> 7", eng.raw_modraise(c, 7), lambda: s.orc.modraise(x[:, 0], 7, eng.q[:7], eng.psi_q[:7]))
        s.out("modraise 1 -> 3", eng.raw_modraise(c, 3), lambda: s.orc.modraise(x[:, 0], 3, eng.q[:3], eng.psi_q[:3]))
    run(trios("toy13"), orc, scen)


@pytest.mark.parametrize("ells,n1,n2,rows", [
    ([6, 3], 4, 2, 2),                       # alpha = 2: full and partial digits; absent terms of every shape
    ([4], 2, 9, 2),                          # more groups than one launch holds (4) and than one shared ModDown (7)
])
def test_lt_apply(trios, orc, ells, n1, n2, rows):
    baby = list(range(n1))
    giant = [g * n1 for g in range(n2)]
    absent = _absent(n1, n2)

    def scen(s):
        eng = s.eng
        keys = keys_for(s, baby[1:] + giant[1:], 7300)
        rev = s.rev(keys)
        pts, encs = _terms(eng, n1, n2, absent, seed=s.seed(11 * n1 + n2))
        lt = eng.lt_create_pts(pts, baby, giant)
        for g, row in enumerate(pts):                           # the diagonals: over the full key basis at each level's scale
            for b, p in enumerate(row):
                if p is not None:
                    s.plain(p, [(eng.n_q + eng.n_p, rev.sf[eng.n_q - ell]) for ell in ells], f"diagonal {g}, {b}")
        for ell in ells:
            pairs = [s.imp(rev, _ct(s.orc, eng, s.seed(600 + 7 * i + ell), ell)) for i in range(rows)]
            got = eng.lt_apply(lt, [p[0] for p in pairs])
            for i, ((c, r), g) in enumerate(zip(pairs, got)):
                s.out(f"ell {ell} row {i}", g, lambda r=r: _lt_oracle(rev, r, encs, baby, giant))
    run(trios("toy"), orc, scen)


# ------------------------------------------------------------------------------------------------ the dot kernels, through their test hooks
class DotOps:
    """uniform ciphertexts and plaintext residues of one (engine, round), with the oracle's sums"""

    def __init__(self, s, ell, n_ct, n_pt):
        self.s, self.ell = s, ell
        eng, orc = s.eng, s.orc
        self.q = eng.q[:ell]
        self.q2 = np.concatenate([self.q, self.q])
        self.ct = [np.stack([orc.uniform_residues(s.seed(11 + 1000 * i + 400 * c), self.q, eng.N) for c in range(2)]) for i in range(n_ct)]
        self.pt = [orc.uniform_residues(s.seed(200003 + 1000 * i), self.q, eng.N) for i in range(n_pt)]
        self.hct = [s.operand(eng.ct_import(x), f"ct {i}") for i, x in enumerate(self.ct)]
        self.hpt = [s.plain(eng.debug_pt_from_residues(x), [(ell, 0.0)], f"pt {i}") for i, x in enumerate(self.pt)]

    def want(self, terms, base=None):
        shape = (2, self.ell, self.s.eng.N)
        out = np.zeros(shape, dtype=np.uint64)
        if terms:
            out = self.s.orc.dot([self.ct[i].reshape(-1, shape[2]) for i, _ in terms], [np.concatenate([self.pt[k], self.pt[k]]) for _, k in terms],
                                 self.q2).reshape(shape)
        if base is not None:
            out = self.s.orc.add(out.reshape(-1, shape[2]), base.reshape(-1, shape[2]), self.q2).reshape(shape)
        return out


def test_dot_plain_two_chunks(trios, orc):
    """33 terms: a chunk of 32 and an accumulating chunk of one"""
    def scen(s):
        o = DotOps(s, 3, 33, 33)
        terms = [(i, (7 * i + 3) % 33) for i in range(33)]
        got = s.eng.debug_dot_plain([o.hct[i] for i, _ in terms], [o.hpt[k] for _, k in terms])
        s.out("dot_plain 33", got, lambda: o.want(terms))
    run(trios("toy"), orc, scen)


@pytest.mark.parametrize("nb", [1, 2])
def test_dot_groups_padded_columns(trios, orc, nb):
    """na = 9: the 16-wide instantiation with 7 padded columns; ng = 3 with absent terms (term (0, 0), a whole column, a one-term group)"""
    na, ng = 9, 3
    gone = {(0, 0)} | {(g, 5) for g in range(ng)} | {(ng - 1, b) for b in range(na) if b != 4}

    def scen(s):
        o = DotOps(s, 3, nb * na, ng * na)
        cts = [[o.hct[x * na + b] for b in range(na)] for x in range(nb)]
        pts = [[None if (g, b) in gone else o.hpt[g * na + b] for b in range(na)] for g in range(ng)]
        outs = s.eng.debug_dot_groups(cts, pts)
        for x in range(nb):
            for g in range(ng):
                terms = [(x * na + b, g * na + b) for b in range(na) if (g, b) not in gone]
                s.out(f"batch {x} group {g}", outs[x][g], lambda terms=terms: o.want(terms))
    run(trios("toy"), orc, scen)


def test_dot_cyclic_padded_entries(trios, orc):
    """n = 5 live columns, 27 padded entries dropped by the wave-uniform select"""
    def scen(s):
        o = DotOps(s, 2, 5, 32)
        row = [(5 * j + 2) % 32 for j in range(32)]
        outs = s.eng.debug_dot_cyclic(o.hct, [o.hpt[k] for k in row])
        for k in range(32):
            s.out(f"output {k}", outs[k], (lambda k=k: o.want([(i, row[(i + k) % 32]) for i in range(5)])) if k in (0, 1, 27, 28, 31) else None)
    run(trios("toy"), orc, scen)


def test_dot_window_then_accumulate(trios, orc):
    """sparse cur / prev masks; accumulate = 0 into fresh destinations (whatever they held must be gone), then accumulate = 1 on top"""
    cm, pm = 0x90020401, 0x00810012
    cm2, pm2 = 0x00000105, 0x80000000

    def scen(s):
        eng = s.eng
        o = DotOps(s, 2, 64, 32)
        row = [(11 * k + 5) % 32 for k in range(32)]
        pts = [o.hpt[k] for k in row]
        dst = [np.stack([s.orc.uniform_residues(s.seed(700001 + 1000 * i + 400 * c), o.q, eng.N) for c in range(2)]) for i in range(32)]
        dest = [eng.ct_import(x) for x in dst]

        def terms(t, cmask, pmask):
            return [(j, row[(t - j) % 32]) for j in range(32) if j <= t and cmask >> j & 1] + \
                   [(32 + j, row[(t - j) % 32]) for j in range(32) if j > t and pmask >> j & 1]
        cur = [o.hct[j] if cm >> j & 1 else None for j in range(32)]
        prev = [o.hct[32 + j] if pm >> j & 1 else None for j in range(32)]
        eng.debug_dot_window(cur, prev, pts, dest, accumulate=False)
        first = {}
        for t in range(32):
            first[t] = dest[t].export()
            s.out(f"window output {t}", dest[t], (lambda t=t: o.want(terms(t, cm, pm))) if t in (0, 1, 10, 31) else None)
        cur = [o.hct[j] if cm2 >> j & 1 else None for j in range(32)]
        prev = [o.hct[32 + j] if pm2 >> j & 1 else None for j in range(32)]
        eng.debug_dot_window(cur, prev, pts, dest, accumulate=True)
        for t in range(32):
            s.out(f"accumulated output {t}", dest[t], (lambda t=t: o.want(terms(t, cm2, pm2), base=first[t])) if t in (0, 2, 8, 31) else None)
    run(trios("toy"), orc, scen)
