"""CKKS bootstrapping on the GPU, checked by decryption.
Stated tolerance: 2e-4 absolute for |m| <= 1 — the sine approximation of the modular reduction contributes
(2 pi 2^-c |mu|)^2 / 6 relative (c = 10: 6e-6), the degree-47 cosine fit ~1e-10 * 4^R * 2^c = 7e-6, CKKS noise
of ~25 multiplicative levels the rest."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _engine(fa, log_slots):
    e = fa.Engine("boot12", seed=77, log_slots=log_slots)
    e.keygen()
    e.gen_relin_key()
    e.bootstrap_setup(3, 3, 1 << log_slots)
    return e


def _coeffs(m):
    """unscaled plaintext coefficients (mu_lo + i mu_hi) of the slot vector m: w = U^H m / n, U_jk = zeta_j^k"""
    n = len(m)
    j = np.arange(n)
    e5 = np.array([pow(5, int(t), 4 * n) for t in j])
    U = np.exp(2j * np.pi * np.outer(e5, np.arange(n)) / (4 * n))
    return U.conj().T @ m / n


@pytest.mark.parametrize("log_slots", [10, 11])     # 10: sparse packing (N/4 slots, SubSum path); 11: full packing
def test_bootstrap_refreshes_levels_and_keeps_message(fa, log_slots):
    eng = _engine(fa, log_slots)
    try:
        n = 1 << log_slots
        m = np.random.default_rng(3).uniform(-1, 1, n)
        ct = eng.encrypt(m, level=eng.n_q - 3)               # 3 limbs left: nearly exhausted
        assert ct.info()["ell"] == 3
        # stage 2: slots hold t_k / (q0 K) (bit-reversed order) with t = Delta' mu + q0 I
        a = eng.decrypt(eng.bootstrap_partial(ct, 2))
        frac = a * 28 - np.round(a * 28)
        w = _coeffs(m)
        if len(a) == 2 * n:                                   # sparse packing: [t_k | t_{k+n}] share one ciphertext (2n slots)
            assert np.max(np.abs(np.sort(frac[:n] * 2 ** 10) - np.sort(w.real))) < 1e-3
            assert np.max(np.abs(np.sort(frac[n:] * 2 ** 10) - np.sort(w.imag))) < 1e-3
        else:
            assert len(a) == n
            assert np.max(np.abs(np.sort(frac * 2 ** 10) - np.sort(w.real))) < 1e-3
        out = eng.bootstrap(ct)
        info = out.info()
        assert info["ell"] >= 4, info                         # strictly more limbs than before
        err = np.max(np.abs(eng.decrypt(out) - m))
        assert err < 2e-4, err
        # the refreshed ciphertext is usable: one more multiplication
        sq = eng.mult(out, out)
        assert np.max(np.abs(eng.decrypt(sq) - m * m)) < 1e-3
    finally:
        eng.close()


def test_bootstrap_requires_setup_and_two_limbs(fa):
    e = fa.Engine("boot12", seed=1)
    e.keygen()
    ct = e.encrypt(np.zeros(4), level=e.n_q - 2)
    with pytest.raises(fa.FhelinError) as ei:
        e.bootstrap(ct)
    assert ei.value.code == 4                                 # EvalBootstrapSetup has not been called
    e.close()


def test_async_heavy_ops_match_the_synchronous_path(fa, monkeypatch):
    """Heavy ops issued back to back run on alternating worker lanes and are joined when their results are used
    (deferred.h run_heavy).  The residues must not depend on that: the same call sequence with FHELIN_ASYNC=0
    (everything on the main stream) has to export bit-identical ciphertexts — chains on one ciphertext (polynomial then
    bootstrap), independent ciphertexts interleaved, results consumed in the opposite order, and an input freed by the
    host while its consumer may still be running."""
    cheb = [0.0, 1.0, 0.0, -0.25, 0.0, 0.05, 0.0, -0.01]

    def run(mode):
        # "lanes": at the call, on alternating worker lanes; "sync": at the call, on the main stream; "deferred" (default): when
        # the results are read, batched (three Chebyshev evaluations in one call, then three bootstraps in one call)
        monkeypatch.setenv("FHELIN_LAZY_HEAVY", "1" if mode == "deferred" else "0")
        monkeypatch.setenv("FHELIN_ASYNC", "0" if mode == "sync" else "1")
        eng = _engine(fa, 10)
        try:
            rng = np.random.default_rng(11)
            ms = [rng.uniform(-0.5, 0.5, 1 << 10) for _ in range(3)]
            outs = []
            for m in ms:
                ct = eng.encrypt(m, level=eng.n_q - 6)
                p = eng.eval_chebyshev(ct, cheb, -1.0, 1.0)     # lane k
                del ct                                           # the host drops the input while lane k may still read it
                outs.append(eng.bootstrap(p))                   # same lane (chain), next ciphertext -> other lane
            s = eng.add(outs[2], outs[0])                       # consume in a different order than produced
            s = eng.add(s, outs[1])
            return [o.export() for o in outs] + [s.export()], [eng.decrypt(o) for o in outs], ms
        finally:
            eng.close()

    a, dec, ms = run("lanes")
    b, _, _ = run("sync")
    d, _, _ = run("deferred")
    for x, y, z in zip(a, b, d):
        assert np.array_equal(x, y) and np.array_equal(x, z)
    u = [np.polynomial.chebyshev.chebval(m, [cheb[0] / 2] + cheb[1:]) for m in ms]
    for d, w in zip(dec, u):
        assert np.max(np.abs(d - w)) < 5e-4


def test_packed_and_two_ciphertext_modular_reduction_agree(fa, monkeypatch):
    """sparse packing: the real and imaginary coefficient halves go through EvalMod in ONE ciphertext (last CoeffsToSlots stage
    written over 2n slots as [d | -i d], first SlotsToCoeffs stage reading [L | R]); FHELIN_BOOT_PACKED=0 keeps the two-ciphertext
    form.  Same message out of both, same level, and fewer key switches in the packed form's EvalMod."""
    res = {}
    for packed in ("1", "0"):
        monkeypatch.setenv("FHELIN_BOOT_PACKED", packed)
        eng = _engine(fa, 10)
        try:
            m = np.random.default_rng(3).uniform(-1, 1, 1 << 10)
            ct = eng.encrypt(m, level=eng.n_q - 3)
            out = eng.bootstrap(ct)
            res[packed] = (eng.decrypt(out), out.info()["ell"], out.info()["slots"])
        finally:
            eng.close()
    for packed in ("1", "0"):
        assert np.max(np.abs(res[packed][0] - m)) < 2e-4, packed
    assert res["1"][1:] == res["0"][1:]


def test_grouped_inner_sums_give_the_same_residues(fa, monkeypatch):
    """the inner sums of all giant steps of a linear stage come out of one pass over the rotated ciphertexts
    (Evaluator::dot_plain_groups, kernel ew_dot_groups): exact integer sums, so the bootstrapped ciphertext must equal the one
    computed with one pass per giant step (FHELIN_DOT_GROUPS=0) residue for residue"""
    outs = []
    for on in ("1", "0"):
        monkeypatch.setenv("FHELIN_DOT_GROUPS", on)
        eng = _engine(fa, 10)
        try:
            m = np.random.default_rng(3).uniform(-1, 1, 1 << 10)
            ct = eng.encrypt(m, level=eng.n_q - 3)               # same seed, same call sequence: the same keys and ciphertext
            outs.append(eng.bootstrap(ct).export())
        finally:
            eng.close()
    assert np.array_equal(outs[0], outs[1])


@pytest.mark.parametrize("log_slots", [10, 11])
def test_batched_bootstrap_gives_the_single_bootstraps_residues(fa, log_slots):
    """fhelin_bootstrap_batch (the GELU containers / the two affine-1 halves of a sample in one pipeline: one ModUp over the batch
    per baby-step set, batched giant steps, batched EvalMod) == fhelin_bootstrap one by one, residue for residue, for sparse
    and full packing, inputs at different levels and scales, with and without a planned drop; the deferred form (bootstraps
    issued back to back, results read afterwards) takes the same batched path"""
    eng = _engine(fa, log_slots)
    try:
        n = 1 << log_slots
        rng = np.random.default_rng(21)
        ms = [rng.uniform(-1, 1, n) for _ in range(3)]
        cts = [eng.encrypt(ms[0], level=eng.n_q - 3), eng.encrypt(ms[1], level=eng.n_q - 2), eng.mult_real(eng.encrypt(ms[2], level=eng.n_q - 4), 0.5)]
        ms[2] = 0.5 * ms[2]
        single = [eng.bootstrap_drop(c, 0).export() for c in cts]
        got = eng.bootstrap_batch(cts)
        for g, s, m in zip(got, single, ms):
            assert np.array_equal(g.export(), s)
            assert np.max(np.abs(eng.decrypt(g) - m)) < 2e-4
        lazy = [eng.bootstrap(c) for c in cts]                   # deferred: nothing runs until a result is read
        before = eng.stats()["bootstrap"]
        assert np.array_equal(lazy[1].export(), single[1])      # ... then all three, as one batch
        assert eng.stats()["bootstrap"] == before + 3
        assert np.array_equal(lazy[0].export(), single[0]) and np.array_equal(lazy[2].export(), single[2])
        dropped = [eng.bootstrap_drop(c, 3).export() for c in cts[:2]]
        eng.set_level_plan([eng.n_q - 15 - 3] * 2)
        eng.level_plan_begin("apply")
        planned = eng.bootstrap_batch(cts[:2])
        eng.level_plan_begin("off")
        for g, s in zip(planned, dropped):
            assert np.array_equal(g.export(), s)
    finally:
        eng.close()


def test_batched_bootstrap_groups_inputs_by_planned_drop(fa):
    """an applied level plan gives the three inputs of ONE fhelin_bootstrap_batch the drops [3, 1, 3]: inputs of equal drop share a
    batch, every output holds the residues of fhelin_bootstrap_drop with its own drop, and the call takes three sources of the plan"""
    eng = _engine(fa, 10)
    try:
        rng = np.random.default_rng(22)
        cts = [eng.encrypt(rng.uniform(-1, 1, 1 << 10), level=eng.n_q - ell) for ell in (3, 2, 4)]
        drops = [3, 1, 3]
        single = [eng.bootstrap_drop(c, d).export() for c, d in zip(cts, drops)]
        full = eng.n_q - eng.bootstrap_describe()["depth"]
        eng.set_level_plan([full - d for d in drops])
        eng.level_plan_begin("apply")
        got = eng.bootstrap_batch(cts)
        assert eng.level_plan_tell() == ("apply", 3)
        eng.level_plan_begin("off")
        for g, s, d in zip(got, single, drops):
            assert g.info()["ell"] == full - d and np.array_equal(g.export(), s)
    finally:
        eng.close()


def test_bootstrap_precision_at_the_headline_ring(fa):
    """N=2^16, 28+7 limbs, 16384 slots (sparse packing: one EvalMod ciphertext), the forward pass's configuration.  Measured in round 3 over
    four key seeds: 3.4e-5 ... 4.2e-5 maximum error for |m| <= 1 (2.4e-5 ... 2.8e-5 with two EvalMod ciphertexts); asserted at 1.5 x today's
    worst (6.3e-5) so that precision cannot be spent silently; with the planned drop of the GELU bootstraps (4 limbs) as well."""
    eng = fa.Engine("bench", seed=7, n_q=28, n_p=-1)
    try:
        eng.keygen()
        eng.gen_relin_key()
        eng.bootstrap_setup(3, 3, 16384)
        rng = np.random.default_rng(12)
        worst = {}
        for drop in (0, 4):
            m = rng.uniform(-1, 1, 16384)
            ct = eng.encrypt(m, level=eng.n_q - 2)
            out = eng.bootstrap_drop(ct, drop)
            worst[drop] = float(np.max(np.abs(eng.decrypt(out) - m)))
            assert out.info()["ell"] == eng.n_q - eng.bootstrap_describe()["depth"] - drop
        # 15 levels: the refreshed ciphertext keeps 12 rescales of the 27-level chain; the reference counts on 10 after OpenFHE's
        # (/root/reference/src/FHEController.cpp:27-33: "available multiplications: levelsUsedBeforeBootstrap - 2")
        assert eng.bootstrap_describe()["depth"] == 15 and eng.n_q - 15 - 1 >= 12 - 2
        print("bootstrap max error at N=2^16, 28+7 limbs:", {k: f"{v:.2e}" for k, v in worst.items()}, "(asserted < 6.3e-5)")
        assert max(worst.values()) < 6.3e-5, worst
    finally:
        eng.close()
