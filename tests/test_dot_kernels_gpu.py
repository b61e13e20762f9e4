"""The five ciphertext x plaintext inner-sum kernels of kernels_elem.hip, each reached directly (include/fhelin.h "test hooks") and pinned
bit for bit against the oracle on operands chosen residue by residue:

    ew_dot_kernel              out   = sum_i a_i * b_i                                               (fhelin_debug_dot_plain)
    ew_dot_groups_kernel<8|16> out_g = sum_b a_b * p_{g,b}, absent terms, batches                    (fhelin_debug_dot_groups)
    ew_cyclic_dot_kernel       out_k = sum_{i<n} a_i * m_{(i + k) mod 32}                            (fhelin_debug_dot_cyclic)
    ew_window_dot_kernel<G>    out_t (+)= sum_j (j <= t ? cur_j : prev_j) * m_{(t - j) mod 32}       (fhelin_debug_dot_window)

(the formulas of the header comments in kernels_elem.h).  The composites that otherwise reach these kernels build their own plaintexts -
encodings of 0/1 block masks - and never fill the cyclic kernel's 32 columns; here every ciphertext and every plaintext is uniform with a
seed of its own, so that any mis-pairing of a column with a mask row changes the result, and at the coefficients PLANT every operand of a
launch holds an extreme value at the same place: q - 1, the value with an all-ones low half, the one with a zero low half and a maximal
high half, 1 and 0, cycled per limb.  There the sums are recomputed with Python integers, independent of the oracle's own modular
multiply; the first two values are where Acc30::s1 comes closest to 2^64 and the 128-bit sums are largest.

Every output, component, limb and coefficient is compared with np.array_equal."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

# chain -> (overrides of "toy", N = 2^12; the branch it is there for)
CHAINS = {
    "toy": (dict(), "55-bit q0 (split at 30 bits) and 52/53-bit scaling primes below 2^53 (split at 27): both bodies in one launch"),
    "p53": (dict(n_q=4, scale_bits=53), "54-bit and 53-bit scaling primes: both sides of the (q >> 53) == 0 dispatch"),
    "p60": (dict(n_q=4, first_bits=60, scale_bits=59), "60-bit q0, 59/60-bit scaling primes: Acc30::s1 and the 128-bit sums at their bounds"),
    "p24": (dict(n_q=4, n_p=2, dnum=2, first_bits=24, scale_bits=24, special_bits=24), "24/25-bit primes: the high halves are zero"),
}
ELLS = {"full": "ell = n_q", "one": "ell = 1: a single limb, grid.y = 1"}
N_CT, N_PT = 64, 128                 # operands per (chain, ell): 2 x 32 window columns / 3 x 16 batch columns; 8 x 16 group terms
FULL = (1 << 32) - 1


def plant_coeffs(n):
    """first and last lane of a workgroup, and both halves of the u64x2 pairs of the N/512-grid kernels"""
    return [0, 255, 256, n // 2 - 1, n // 2, n - 1]


def extremes(q):
    sh = 27 if q < 2 ** 53 else 30
    return [q - 1, (((q >> sh) << sh) - 1) % q, ((q - 1) >> sh) << sh, 1, 0]     # below 2^27 the second is q - 1 again, the third 0


def plant(x, q, shift):
    """x [ell][N]: limb l, planted coefficient i <- extremes(q_l)[(i + l + shift) mod 5]"""
    for l, ql in enumerate(int(v) for v in q):
        ext = extremes(ql)
        for i, n in enumerate(plant_coeffs(x.shape[-1])):
            x[l, n] = ext[(i + l + shift) % 5]
    return x


class Operands:
    """the operands of one (chain, ell): numpy arrays and their imported handles.  Plaintexts and component 0 of every ciphertext hold the
    same kind of extreme at a planted coefficient (the maximal products), component 1 the next kind (the mixed ones)."""

    def __init__(self, orc, eng, ell):
        self.orc, self.eng, self.ell = orc, eng, ell
        self.q = eng.q[:ell]
        self.ct = [np.stack([plant(orc.uniform_residues(11 + 1000 * i + 400 * c, self.q, eng.N), self.q, c) for c in range(2)]) for i in range(N_CT)]
        self.pt = [plant(orc.uniform_residues(200003 + 1000 * i, self.q, eng.N), self.q, 0) for i in range(N_PT)]
        self.pt2 = [np.concatenate([x, x]) for x in self.pt]
        self.q2 = np.concatenate([self.q, self.q])
        self.dst = [np.stack([orc.uniform_residues(700001 + 1000 * i + 400 * c, self.q, eng.N) for c in range(2)]) for i in range(64)]
        # the planted columns as Python integers: [2][ell][6] per ciphertext, [ell][6] per plaintext
        self.at = plant_coeffs(eng.N)
        self.ct_int = [x[..., self.at].astype(object) for x in self.ct]
        self.pt_int = [x[..., self.at].astype(object) for x in self.pt]
        self.q_int = np.array([int(v) for v in self.q], dtype=object)[:, None]
        self.hct = [eng.ct_import(x) for x in self.ct]
        self.hpt = [eng.debug_pt_from_residues(x) for x in self.pt]

    def want(self, terms, base=None):
        """[2][ell][N]: sum of ct[i] * pt[k] over terms = [(i, k)], plus base - orc.dot per component, orc.add of the earlier sum"""
        shape = (2, self.ell, self.eng.N)
        out = np.zeros(shape, dtype=np.uint64)
        if terms:      # both components in one call: [2 ell][N] operands over the limbs (q, q)
            out = self.orc.dot([self.ct[i].reshape(-1, shape[2]) for i, _ in terms], [self.pt2[k] for _, k in terms], self.q2).reshape(shape)
        if base is not None:
            out = self.orc.add(out.reshape(-1, shape[2]), base.reshape(-1, shape[2]), self.q2).reshape(shape)
        return out

    def check(self, got, terms, what, base=None):
        want = self.want(terms, base)
        assert got.shape == want.shape, what
        # the planted columns again, with Python integers (object arrays: exact products and sums of any size)
        s = sum((self.ct_int[i] * self.pt_int[k] for i, k in terms), np.zeros((2, self.ell, len(self.at)), dtype=object))
        if base is not None:
            s = s + base[..., self.at].astype(object)
        s = s % self.q_int
        assert np.array_equal(want[..., self.at].astype(object), s), ("oracle vs integers", what)
        bad = np.argwhere(got[..., self.at].astype(object) != s)
        assert not len(bad), ("planted", what, "(component, limb, planted coefficient):", [(c, l, self.at[n]) for c, l, n in bad[:4].tolist()])
        assert np.array_equal(got, want), (what, "first mismatches (component, limb, coefficient):", np.argwhere(got != want)[:4].tolist())
        return want


_ENG, _OPS = {}, {}


def engine(fa, chain):
    if chain not in _ENG:
        _ENG[chain] = fa.Engine("toy", device=0, seed=1, **CHAINS[chain][0])
    return _ENG[chain]


def operands(fa, orc, chain, ell_kind):
    if (chain, ell_kind) not in _OPS:
        eng = engine(fa, chain)
        _OPS[(chain, ell_kind)] = Operands(orc, eng, eng.n_q if ell_kind == "full" else 1)
    return _OPS[(chain, ell_kind)]


def close_all():
    _OPS.clear()
    for e in _ENG.values():
        e.close()
    _ENG.clear()


@pytest.fixture(scope="module")
def ops(fa, orc):
    yield lambda chain, ell_kind: operands(fa, orc, chain, ell_kind)
    close_all()


BOTH = [pytest.param(c, e, id=f"{c}-{e}") for c in CHAINS for e in ELLS]


def test_chains_are_what_they_are_there_for(fa):
    bits = {c: [int(v).bit_length() for v in engine(fa, c).q] for c in CHAINS}
    assert all(engine(fa, c).N == 1 << 12 for c in CHAINS)
    assert bits["toy"][0] == 55 and max(bits["toy"][1:]) <= 53 and all(int(v) < 2 ** 53 for v in engine(fa, "toy").q[1:])
    assert {int(v) >> 53 == 0 for v in engine(fa, "p53").q[1:]} == {True, False}
    assert bits["p60"][0] == 60 and min(bits["p60"]) >= 59
    assert max(bits["p24"]) <= 25


# ------------------------------------------------------------------------------------------------ the plaintext import itself
def test_pt_from_residues_is_its_one_encoding_and_stays_out_of_the_cache(fa, ops):
    o = ops("toy", "full")
    eng, ell = o.eng, o.ell
    before = eng.cache_stats()
    p = eng.debug_pt_from_residues(o.pt[3])
    assert np.array_equal(eng.pt_export(p, ell), o.pt[3])            # Plaintext::at(ell, Delta of that limb count) returns it
    got = eng.debug_dot_plain(o.hct[:2], [p, o.hpt[1]]).export()
    o.check(got, [(0, 3), (1, 1)], "fresh import")
    after = eng.cache_stats()
    assert (after["pt_cache_entries"], after["pt_cache_bytes"]) == (before["pt_cache_entries"], before["pt_cache_bytes"])
    for use in (lambda: eng.pt_export(p, ell - 1),                                    # another limb count
                lambda: eng.pt_export(p, ell, 2.0 ** 40),                             # another scale
                lambda: eng.debug_dot_plain(ops("toy", "one").hct[:2], [p, p])):      # one-limb ciphertexts ask for a one-limb encoding
        with pytest.raises(fa.FhelinError) as ei:
            use()
        assert ei.value.code == 4, ei.value                                           # FHELIN_ERR_STATE, not an encoding of nothing
    bad = o.pt[3].copy()
    bad[ell - 1, 77] = eng.q[ell - 1]
    with pytest.raises(fa.FhelinError) as ei:
        eng.debug_pt_from_residues(bad)
    assert ei.value.code == 1                                                         # FHELIN_ERR_ARG


# ------------------------------------------------------------------------------------------------ ew_dot_kernel
DOT_N = {2: "the shortest sum the kernel takes (one term is a plain product)",
         16: "the sixteen products the Acc128 comment used to promise",
         17: "one more",
         32: "EwItems::MAX_ITEMS, one launch: at the planted maximum 32 (q - 1)^2 reaches barrett_reduce128 with hi >= q on a 60-bit limb"}


@pytest.mark.parametrize("chain,ell_kind", BOTH)
def test_dot_plain(ops, chain, ell_kind):
    o = ops(chain, ell_kind)
    for n in DOT_N:
        # the plaintexts in another order than the ciphertexts: a kernel that paired them by anything but position would differ
        terms = [(i, (7 * i + 3) % N_PT) for i in range(n)]
        got = o.eng.debug_dot_plain([o.hct[i] for i, _ in terms], [o.hpt[k] for _, k in terms]).export()
        o.check(got, terms, f"dot_plain n={n}")
    if chain == "p60":      # the case the 32-term launch is there for: the sum's high word is not below q
        q0, n0 = int(o.q[0]), plant_coeffs(o.eng.N)[0]
        s = sum(int(o.ct[i][0, 0, n0]) * int(o.pt[k][0, n0]) for i, k in terms)
        assert s == 32 * (q0 - 1) ** 2 and (s >> 64) >= q0


# ------------------------------------------------------------------------------------------------ ew_dot_groups_kernel<8>, <16>
def _absent(kind, na, ng):
    if kind == "column":            # a whole column absent: its bit is clear in every group's mask
        b0 = na - 4 if na > 4 else 0
        return {(g, b0) for g in range(ng)}
    if kind == "first":             # term (0, 0) absent: the launcher's search for a readable dummy pointer walks on
        return {(0, 0)}
    if kind == "one":               # a whole group with one term, its last: term (0, 0) absent as well, and the search walks the whole row
        return {(0, b) for b in range(na - 1)} | {(ng - 1, b) for b in range(na) if b != na // 2}
    return set()


# case -> (na, ng, nb, absent terms, the branch it reaches)
GROUP_CASES = {
    "na1_ng1": (1, 1, 1, "none", "<8>, one live column and seven padded ones; one group: the prefetch re-reads it (gn == g)"),
    "na1_ng8_nb3": (1, 8, 3, "none", "<8>, batch stride with a single column"),
    "na8_ng1_nb3": (8, 1, 3, "first", "<8> at full width over a batch of three; with one column less in group 0"),
    "na8_ng8_column": (8, 8, 1, "column", "<8> at full width, next group's plaintexts in flight; a whole column absent"),
    "na8_ng8_nb3_one": (8, 8, 3, "one", "<8>: groups of a single term, batch element fastest after the component"),
    "na9_ng1": (9, 1, 1, "none", "<16> with one live column in the second batch of eight"),
    "na9_ng8_first": (9, 8, 1, "first", "<16>: term (0, 0) absent, the dummy pointer comes from (0, 1)"),
    "na16_ng1_nb3": (16, 1, 3, "none", "<16> at full width over a batch of three"),
    "na16_ng8_column": (16, 8, 1, "column", "<16>: a column of the second batch of eight absent in every group"),
    "na16_ng8_nb3_one": (16, 8, 3, "one", "<16>: groups of a single term (in the second batch of eight), batch of three"),
}


@pytest.mark.parametrize("case", list(GROUP_CASES))
@pytest.mark.parametrize("chain,ell_kind", BOTH)
def test_dot_groups(ops, chain, ell_kind, case):
    o = ops(chain, ell_kind)
    na, ng, nb, kind, _ = GROUP_CASES[case]
    gone = _absent(kind, na, ng)
    ct_of = lambda x, b: (x * 16 + b * 5) % N_CT if nb == 1 else x * 16 + (b * 5) % 16      # distinct over (x, b): 5 is odd
    pt_of = lambda g, b: (g * 16 + b * 3 + 1) % N_PT if (g, b) not in gone else None          # distinct over (g, b)
    cts = [[o.hct[ct_of(x, b)] for b in range(na)] for x in range(nb)]
    pts = [[(o.hpt[pt_of(g, b)] if pt_of(g, b) is not None else None) for b in range(na)] for g in range(ng)]
    outs = o.eng.debug_dot_groups(cts, pts)
    assert len(outs) == nb and all(len(r) == ng for r in outs)
    for x in range(nb):             # every batch element against ITS ciphertexts' sums
        for g in range(ng):
            terms = [(ct_of(x, b), pt_of(g, b)) for b in range(na) if (g, b) not in gone]
            assert terms
            o.check(outs[x][g].export(), terms, f"dot_groups {case} batch {x} group {g}")


# ------------------------------------------------------------------------------------------------ ew_cyclic_dot_kernel
CYCLIC_N = {1: "one live column, 31 dropped by the wave-uniform select",
            9: "the nine live columns the composites pass",
            31: "one dropped column",
            32: "every column live: four full flushes of eight per output on the 30-bit path, the fold after sixteen products"}


@pytest.mark.parametrize("n", list(CYCLIC_N))
@pytest.mark.parametrize("chain,ell_kind", BOTH)
def test_dot_cyclic(ops, chain, ell_kind, n):
    o = ops(chain, ell_kind)
    col = [(3 * i + n) % N_CT for i in range(n)]          # distinct (3 is odd): not the ciphertexts the other lengths use at the same column
    row = [(5 * j + 2) % 32 + 32 for j in range(32)]      # 32 distinct plaintexts
    outs = o.eng.debug_dot_cyclic([o.hct[i] for i in col], [o.hpt[k] for k in row])
    assert len(outs) == 32
    for k in range(32):
        o.check(outs[k].export(), [(col[i], row[(i + k) % 32]) for i in range(n)], f"dot_cyclic n={n} output {k}")


# ------------------------------------------------------------------------------------------------ ew_window_dot_kernel<G>
_rng = np.random.default_rng(20240607)
WINDOW_MASKS = {       # pattern -> (cur_mask, prev_mask, what it reaches)
    "all": (FULL, FULL, "every column of both windows: each output takes cur up to its own column and prev beyond"),
    "prev_absent": (FULL, 0, "the first block of a row: nothing before the window"),
    "cur_absent": (0, FULL, "the block past the end: only the previous window"),
    "bit0": (1, 1, "cur_0 meets every output, prev_0 none"),
    "bit31": (1 << 31, 1 << 31, "cur_31 meets output 31 only, prev_31 every other one"),
    "sparse_a": (int(_rng.integers(1, 1 << 32)), int(_rng.integers(1, 1 << 32)), "a random sparse pattern"),
    "sparse_b": (int(_rng.integers(1, 1 << 32)) & int(_rng.integers(1, 1 << 32)), int(_rng.integers(1, 1 << 32)) & int(_rng.integers(1, 1 << 32)),
                 "a sparser one"),
}
CHAIN_OF_THREE = ["all", "sparse_a", "sparse_b"]     # accumulate on: three tap chunks into the same dest


def check_window(o):
    """every mask pattern with accumulate off (dest holds other values beforehand: they must be gone), then three accumulating calls
    into the same dest, which starts as a uniform ciphertext"""
    eng = o.eng
    cur_i, prev_i = list(range(32)), list(range(32, 64))
    row = [(11 * k + 5) % 32 + 64 for k in range(32)]     # 32 distinct plaintexts, another set than the cyclic test's
    pts = [o.hpt[k] for k in row]
    dest = [eng.ct_import(x) for x in o.dst[:32]]
    sums = {}
    for name, (cm, pm, _) in WINDOW_MASKS.items():
        cur = [o.hct[cur_i[j]] if cm >> j & 1 else None for j in range(32)]
        prev = [o.hct[prev_i[j]] if pm >> j & 1 else None for j in range(32)]
        eng.debug_dot_window(cur, prev, pts, dest, accumulate=False)
        sums[name] = []
        for t in range(32):
            terms = [(cur_i[j], row[(t - j) % 32]) for j in range(32) if j <= t and cm >> j & 1]
            terms += [(prev_i[j], row[(t - j) % 32]) for j in range(32) if j > t and pm >> j & 1]
            sums[name].append((terms, o.check(dest[t].export(), terms, f"dot_window {name} output {t}")))
    acc = [eng.ct_import(x) for x in o.dst[32:64]]
    run = [x.copy() for x in o.dst[32:64]]
    for step, name in enumerate(CHAIN_OF_THREE):
        cm, pm, _ = WINDOW_MASKS[name]
        cur = [o.hct[cur_i[j]] if cm >> j & 1 else None for j in range(32)]
        prev = [o.hct[prev_i[j]] if pm >> j & 1 else None for j in range(32)]
        eng.debug_dot_window(cur, prev, pts, acc, accumulate=True)
        for t in range(32):
            run[t] = o.check(acc[t].export(), sums[name][t][0], f"dot_window accumulate step {step} ({name}) output {t}", base=run[t])


@pytest.mark.parametrize("chain,ell_kind", BOTH)
def test_dot_window_default_group(ops, chain, ell_kind):
    assert "FHELIN_WINDOW_GROUP" not in os.environ
    check_window(ops(chain, ell_kind))


@pytest.mark.parametrize("group", [1, 4])
def test_dot_window_other_groups_in_a_fresh_process(group):
    """FHELIN_WINDOW_GROUP is read once per process: ew_window_dot_kernel<1> and <4> run the same checker in a child of their own, on the
    27/30-bit mix of plain toy and on the 60-bit chain"""
    env = dict(os.environ, FHELIN_WINDOW_GROUP=str(group))
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.abspath(__file__), "window", str(group), "toy", "p60"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=240, cwd=ROOT)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert f"window ok: group {group}, chains toy p60" in r.stdout
    assert "FHELIN_WINDOW_GROUP" not in os.environ or os.environ["FHELIN_WINDOW_GROUP"] != str(group)


if __name__ == "__main__":
    assert sys.argv[1] == "window" and os.environ["FHELIN_WINDOW_GROUP"] == sys.argv[2]
    import fhe_linformer_amd
    import oracle
    oracle.lib()
    oracle.set_threads(min(16, len(os.sched_getaffinity(0))))
    for ch in sys.argv[3:]:
        for kind in ELLS:
            check_window(operands(fhe_linformer_amd, oracle, ch, kind))
    close_all()
    print(f"window ok: group {sys.argv[2]}, chains {' '.join(sys.argv[3:])}")
