"""Rotations that gather at the inner product: every ModDown of a rotation is the identity one that the row pass of
NTT(conv) finishes.  A merged rotation sum gets its rotated c0 parts into the accumulator times P (ks_inner_multi_kernel); a plain
rotation reads digits, own limb and c0 through its map, the key's permuted copy, and converts with the signs of the automorphism
(ks_inner_kernel<true>, moddown_conv_kernel<., true>).  Everything is bit-identical by construction, so every check is an equality:
the default engine, FHELIN_ROT_GATHER=0 (gathers in moddown_finish_kernel) and FHELIN_FUSE_FINISH=0 (separate finishing kernels
everywhere) against the oracle - and therefore against each other - with the same imported uniform keys; the callers that Python
reaches only through composites are compared across the engines byte for byte (their equality with the oracle is what
test_composites_gpu.py and test_boot_residue_gpu.py assert).

Levels 24, 12, 7, 2, 1 of the bench chain (alpha = 6): full digits, a short last digit, one digit, the few-limb tail; the small ring
covers a column pass other than A = 8."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
LD = np.longdouble

KNOBS = {"default": {"FHELIN_ROT_GATHER": "1", "FHELIN_FUSE_FINISH": "1", "FHELIN_FUSE_MODDOWN": "0"},
         "finish_gathers": {"FHELIN_ROT_GATHER": "0", "FHELIN_FUSE_FINISH": "1", "FHELIN_FUSE_MODDOWN": "0"},
         "separate": {"FHELIN_ROT_GATHER": "1", "FHELIN_FUSE_FINISH": "0", "FHELIN_FUSE_MODDOWN": "0"}}
# preset -> (levels, the four rotations, the hoisted index list of more than 16)
RINGS = {"bench": ([24, 12, 7, 2, 1], [1, 128, -1, 8192], [1, 128, -1, 8192] + list(range(2, 15))),
         "toy13": ([7, 3], [1, 128, -1, 1024], [1, 128, -1, 1024] + list(range(2, 15)))}


def _engine(fa, preset, env, **kw):
    """a context created with the given knobs (they are read when the context is created)"""
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return fa.Engine(preset, device=0, **kw)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _ct(orc, eng, seed, ell):
    return np.stack([orc.uniform_residues(seed + 1000 * p, eng.q[:ell], eng.N) for p in range(2)])


def _evk(orc, eng, seed):
    d = eng.dnum_digits
    k = np.stack([orc.uniform_residues(seed + 50 * j, eng.moduli, eng.N) for j in range(2 * d)])
    return k.reshape(d, 2, eng.n_limbs, eng.N)


def _imp(eng, rev, x):
    """the same ciphertext on both sides: engine handle + oracle-side RCt (scale = the level's Delta as a double)"""
    from oracle.residue_eval import RCt
    sc = float(rev.sf[len(eng.q) - x.shape[1]])
    return eng.ct_import(x, deg=1, scale=sc), RCt(x, 1, LD(sc))


def _eq(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes(), what


@pytest.fixture(scope="module", params=list(RINGS))
def ring(request, fa, orc):
    """the three engines of one ring, every one with the same uniform 'keys' (parity of the residue functions needs no real keys)"""
    from oracle.residue_eval import ResidueEvaluator
    preset = request.param
    ells, rots, many = RINGS[preset]
    es = {name: _engine(fa, preset, env) for name, env in KNOBS.items()}
    e0 = es["default"]
    keys = {r: _evk(orc, e0, 7100 + 17 * (r % 100003)) for r in many}
    for e in es.values():
        for r, k in keys.items():
            e.key_import(1, r, k)
    rev = ResidueEvaluator(e0.q, e0.p, e0.psi_q, e0.psi_p, e0.alpha, e0.log_n, keys, e0.params.log_slots)
    yield preset, es, keys, rev, ells, rots, many
    for e in es.values():
        e.close()


def _orc_rotate(orc, e0, keys, x, r):
    return orc.rotate(x, keys[r], orc.galois(e0.log_n, r), e0.alpha, e0.q, e0.p, e0.psi_q, e0.psi_p)


def test_plain_rotations_equal_the_oracle(ring, orc):
    """raw_rotate, rotate, rotate_batch, rotate_many (2 and more than 16 indices), rotate_each == orc.rotate, batch 1 and 3"""
    preset, es, keys, rev, ells, rots, many = ring
    e0 = es["default"]
    for ell in ells:
        xs = [_ct(orc, e0, 300 + 7 * i + ell, ell) for i in range(3)]
        want = {(i, r): _orc_rotate(orc, e0, keys, xs[i], r) for i in range(3) for r in rots}
        want.update({(0, r): _orc_rotate(orc, e0, keys, xs[0], r) for r in many if r not in rots})
        for name, e in es.items():
            tag = (preset, name, ell)
            for r in rots:
                _eq(e.raw_rotate(e.ct_import(xs[0]), r).export(), want[0, r], tag + ("raw_rotate", r))
                _eq(e.rotate(e.ct_import(xs[0]), r).export(), want[0, r], tag + ("rotate", r))
                for i, g in enumerate(e.rotate_batch([e.ct_import(x) for x in xs], r)):
                    _eq(g.export(), want[i, r], tag + ("rotate_batch", r, i))
            for idx in (rots[:2], many):
                for r, g in zip(idx, e.rotate_many(e.ct_import(xs[0]), idx)):
                    _eq(g.export(), want[0, r], tag + ("rotate_many", len(idx), r))
            _eq(e.rotate_each([e.ct_import(xs[0])], rots[:1])[0].export(), want[0, rots[0]], tag + ("rotate_each", 1))
            for i, g in enumerate(e.rotate_each([e.ct_import(x) for x in xs], rots[1:])):
                _eq(g.export(), want[i, rots[1 + i]], tag + ("rotate_each", 3, i))


def test_merged_sums_equal_the_oracle(ring, orc):
    """rotate_sum, rotate_each_sum, hoisted_dot(rescale=False) == orc.rotate_sum, orc.rotate_each_sum, orc.hoisted_dot, batch 1 and 3"""
    preset, es, keys, rev, ells, rots, many = ring
    e0 = es["default"]
    evks = np.stack([keys[r] for r in rots])
    gs = [orc.galois(e0.log_n, r) for r in rots]
    rng = np.random.default_rng(77)
    vals = [rng.uniform(-1, 1, 1 << e0.params.log_slots) for _ in range(len(rots) + 1)]
    pts0 = [e0.encode(v) for v in vals]
    encs = [(lambda p: (lambda ell, sc: e0.pt_export(p, ell, sc)))(p) for p in pts0]
    for ell in ells:
        xs = [_ct(orc, e0, 500 + 7 * i + ell, ell) for i in range(4)]
        want_sum = [orc.rotate_sum(x, evks, gs, e0.alpha, e0.q, e0.p, e0.psi_q, e0.psi_p) for x in xs[:3]]
        rcts = [_imp(e0, rev, x)[1] for x in xs]
        want_each = rev.rotate_each_sum(rcts, rots)
        want_each2 = rev.rotate_each_sum(rcts[:2], rots[:2])
        want_dot = [rev.hoisted_dot(r, encs, rots, rescale=False) for r in rcts[:3]]
        for name, e in es.items():
            tag = (preset, name, ell)
            pts = [e.encode(v) for v in vals]
            imp = lambda x: _imp(e, rev, x)[0]
            _eq(e.rotate_sum([imp(xs[0])], rots)[0].export(), want_sum[0], tag + ("rotate_sum", 1))
            for g, w in zip(e.rotate_sum([imp(x) for x in xs[:3]], rots), want_sum):
                _eq(g.export(), w, tag + ("rotate_sum", 3))
            _eq(e.rotate_each_sum([imp(x) for x in xs], rots).export(), want_each.d, tag + ("rotate_each_sum", 4))
            _eq(e.rotate_each_sum([imp(x) for x in xs[:2]], rots[:2]).export(), want_each2.d, tag + ("rotate_each_sum", 2))
            _eq(e.hoisted_dot([imp(xs[0])], pts, rots, rescale=False)[0].export(), want_dot[0].d, tag + ("hoisted_dot", 1))
            for g, w in zip(e.hoisted_dot([imp(x) for x in xs[:3]], pts, rots, rescale=False), want_dot):
                _eq(g.export(), w.d, tag + ("hoisted_dot", 3))


def _real_engines(fa, preset, extra_env, setup, **kw):
    """the three engines with the SAME real keys (one test seed, the same key generation calls in the same order)"""
    es = {}
    for name, env in KNOBS.items():
        e = _engine(fa, preset, dict(env, **extra_env), seed=99, **kw)
        e.keygen()
        e.gen_relin_key()
        setup(e)
        es[name] = e
    return es


def _same_everywhere(es, run, what):
    """run(engine) -> list of ciphertexts; equal bytes on the three engines"""
    got = {name: [c.export() for c in run(e)] for name, e in es.items()}
    for name in ("finish_gathers", "separate"):
        assert len(got[name]) == len(got["default"])
        for i, (a, b) in enumerate(zip(got["default"], got[name])):
            _eq(b, a, (what, name, i))


def test_composite_callers_agree_across_the_engines(fa):
    """rotsum / rotsum_batch without merged steps (rotate_add, rotate_add_batch) and matmulRE over 128 rows (rotate_many_batch with
    row_mod; rotate_each_sum_rows in its shift sums)"""
    idx = fa.circuit_rotation_indices()
    for merge in ("0", "1"):
        es = _real_engines(fa, "bench", {"FHELIN_MERGE_ROT": merge}, lambda e: e.gen_rotation_keys(idx), n_q=8, n_p=2, dnum=4)
        try:
            e0 = es["default"]
            rng = np.random.default_rng(12)
            src = [e0.encrypt(rng.uniform(-1, 1, 16384)).export() for _ in range(3)]
            W, b = rng.uniform(-1, 1, 16384) / 8, rng.uniform(-1, 1, 16384)
            rows = [e0.encrypt(np.repeat(rng.uniform(-1, 1, 128), 128)).export() for _ in range(128)]
            if merge == "0":
                _same_everywhere(es, lambda e: [e.rotsum(e.ct_import(src[0]), 128, 128), e.rotsum(e.ct_import(src[0]), 32, 128)], "rotsum")
                _same_everywhere(es, lambda e: e.rotsum_batch([e.ct_import(x) for x in src], 128, 1), "rotsum_batch")
            _same_everywhere(es, lambda e: e.matmulRE([e.ct_import(x) for x in rows], e.encode(W), e.encode(b)), "matmulRE " + merge)
        finally:
            for e in es.values():
                e.close()


def test_bootstrap_agrees_across_the_engines(fa):
    """one bootstrap: baby steps (rotate_many_batch), giant steps (rotate_each_sum_rows), conjugation"""
    es = _real_engines(fa, "boot12", {}, lambda e: e.bootstrap_setup(3, 3, 1 << 10), log_slots=10)
    try:
        e0 = es["default"]
        m = np.random.default_rng(3).uniform(-1, 1, 1 << 10)
        ct = e0.encrypt(m, level=e0.n_q - 3)
        x, inf, (hi, lo) = ct.export(), ct.info(), ct.scale_parts()
        _same_everywhere(es, lambda e: e.bootstrap_batch([e.ct_import(x, deg=inf["deg"], scale=float(LD(hi) + LD(lo)))] * 2), "bootstrap")
        assert np.max(np.abs(e0.decrypt(e0.bootstrap(ct)) - m)) < 2e-4      # ... and it is a bootstrap
    finally:
        for e in es.values():
            e.close()
