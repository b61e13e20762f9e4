"""Sparse-secret bootstrapping (include/fhelin.h "Sparse-secret bootstrapping"): with Engine.set_bootstrap_sparse_secret(h~)
the ModRaise step switches to an ephemeral secret of Hamming weight h~ at two limbs, raises, and switches back at the raised level; the
cosine fit then needs five levels and a bootstrap spends 14 instead of 15.  The bootstrap must equal - residues, limbs, noise degree,
80-bit scale - the stage-by-stage oracle (oracle/residue_boot.py) with its `mod_raise` replaced by the definition: orc.keyswitch on c1
with the exported keys of kinds 3 and 4, c0 added, around the parent's rescale and orc.modraise.  Off is the parent's path.

Preset boot12 (N = 2^12, 22 + 6 limbs), h~ = 32, seed 77.  The knob writes cheb_degree 28, not 31: the Chebyshev evaluator takes
degree 31 in six levels (tests/test_boot_residue_gpu.py pins that), 28 is the largest degree it takes in five."""
import os
import struct

import numpy as np
import pytest

from test_boot_residue_gpu import _boot_input, _rev, _same

pytestmark = pytest.mark.gpu
LD = np.longdouble
ERR_ARG, ERR_STATE, ERR_KEY = 1, 4, 5
H = 32
ABS_BOUND = 2e-4          # what tests/test_boot_residue_gpu.py holds this ring to
DEPTH_ON, DEPTH_OFF = 14, 15


def _sparse_bootstrapper(orc):
    from oracle.residue_boot import ResidueBootstrapper
    from oracle.residue_eval import RCt, _llround

    class SparseResidueBootstrapper(ResidueBootstrapper):
        """Bootstrapper::mod_raise with the knob on; rev.keys["to_sparse"] / ["from_sparse"] are the exported keys of kinds 3 / 4"""

        def _switch(self, a, evk):
            rev = self.rev
            ql = rev.q[:a.ell]
            ks = orc.keyswitch(a.d[1], evk, rev.alpha, rev.q, rev.p, rev.psi_q, rev.psi_p)
            return RCt(np.stack([orc.add(a.d[0], ks[0], ql), ks[1]]), a.deg, a.scale)     # (c0 + KS(c1)[0], KS(c1)[1])

        def mod_raise(self, ct, top_ell):
            rev = self.rev
            corr = self.desc["correction"]
            x = rev.rescale(ct) if ct.deg >= 2 else ct
            assert x.npoly == 2 and x.ell >= 2
            if x.ell > 2:
                x = rev.level_reduce(x, 2)
            q0, q1 = LD(int(rev.q[0])), LD(int(rev.q[1]))
            k0 = _llround(q0 / LD(1 << corr) * q1 / x.scale)
            assert k0 >= 2
            x = rev.mult_int(x, k0, True, x.scale * LD(k0))
            x = self._switch(x, rev.keys["to_sparse"])          # at two limbs, in front of the rescale to q0
            x = rev.rescale(x)
            rho = x.scale * LD(1 << corr) / q0
            up = RCt(orc.modraise(x.d[:, 0], top_ell, rev.q[:top_ell], rev.psi_q[:top_ell]), 1, rev.sf[0])
            up = self._switch(up, rev.keys["from_sparse"])      # back to s at the raised level
            gap = (self.N // 2) // self.n
            j = 1
            while j < gap:
                idx = self.n * j
                r = orc.rotate(up.d, rev.keys[idx], orc.galois(rev.log_n, idx), rev.alpha, rev.q, rev.p, rev.psi_q, rev.psi_p)
                up = rev.add(up, RCt(r, up.deg, up.scale))
                j <<= 1
            return up, rho

    return SparseResidueBootstrapper


def _engine(fa, log_slots, h=H, seeded=False, lt=False, **kw):
    eng = fa.Engine("boot12", seed=77, log_slots=log_slots, **kw)
    if seeded:
        eng.set_seeded_keys(True)
    eng.keygen()
    eng.gen_relin_key()
    if h:
        eng.set_bootstrap_sparse_secret(h)
    if lt:
        eng.set_bootstrap_lt(True)
    eng.bootstrap_setup(3, 3, 1 << log_slots)
    return eng


def _oracle(orc, eng):
    """the oracle-side bootstrapper of an engine: the subclass when the knob is on, the unmodified class otherwise"""
    from oracle.residue_boot import ResidueBootstrapper
    desc = eng.bootstrap_describe()
    keys = {"relin": eng.key_export(0), "conj": eng.key_export(2)}
    need = set()
    for st in desc["c2s"] + desc["s2c"]:
        for (g, b, _) in st["terms"]:
            need.update((g, b))
    j = 1
    while j < (eng.N // 2) // desc["slots"]:
        need.add(desc["slots"] * j)
        j <<= 1
    for r in sorted(need - {0}):
        keys[r] = eng.key_export(1, r)
    if desc["sparse_h"]:
        keys["to_sparse"], keys["from_sparse"] = eng.key_export(3), eng.key_export(4)
    cls = _sparse_bootstrapper(orc) if desc["sparse_h"] else ResidueBootstrapper
    return cls(_rev(eng, keys), desc, lambda pt: (lambda ell, sc: eng.pt_export(pt, ell, sc)))


def _equal(a, b):
    return np.array_equal(a.export(), b.export()) and a.info() == b.info() and a.scale_parts() == b.scale_parts()


def _code(fa, fn, *a, **kw):
    with pytest.raises(fa.FhelinError) as ei:
        fn(*a, **kw)
    return ei.value.code, str(ei.value)


@pytest.fixture(scope="module")
def on(fa, orc):
    """(engine, oracle bootstrapper) with the knob on, per log_slots, made once for the module"""
    made = {}

    def get(log_slots):
        if log_slots not in made:
            eng = _engine(fa, log_slots)
            made[log_slots] = (eng, _oracle(orc, eng))
        return made[log_slots]

    yield get
    for eng, _ in made.values():
        eng.close()


@pytest.fixture(scope="module")
def off(fa, orc):
    """the twin with the knob never touched, 1024 slots"""
    eng = _engine(fa, 10, h=0)
    yield eng, _oracle(orc, eng)
    eng.close()


# ---- 1. bit for bit against the oracle, stage by stage ------------------------------------------------------------------------------
@pytest.mark.parametrize("log_slots", [10, 11])     # 10: sparse packing (SubSum after the switch back); 11: full packing
def test_sparse_bootstrap_bit_exact_stage_by_stage(on, log_slots):
    eng, boot = on(log_slots)
    assert boot.desc["packed"] == (log_slots == 10) and boot.desc["sparse_h"] == H == eng.bootstrap_sparse_secret()
    m, ct, r = _boot_input(eng, boot)
    for stage in (1, 2, 3):
        _same(eng.bootstrap_partial(ct, stage), boot.run(r, stop_after=stage), ("stage", stage))    # residues, limbs, degree, 80-bit scale
    _same(eng.bootstrap(ct), boot.run(r), "bootstrap under a sparse ephemeral secret")
    want = boot.run(r, drop=2)
    assert want.ell == eng.n_q - DEPTH_ON - 2
    _same(eng.bootstrap_drop(ct, 2), want, "drop 2")
    if log_slots == 10:
        # not vacuous: the unmodified class on the same keys raises without the switches and ends elsewhere
        from oracle.residue_boot import ResidueBootstrapper
        other = ResidueBootstrapper(boot.rev, boot.desc, boot.enc).run(r, stop_after=1)
        assert not np.array_equal(other.d, boot.run(r, stop_after=1).d)


# ---- 2. limbs -----------------------------------------------------------------------------------------------------------------------
def test_fourteen_levels_and_the_default_untouched(fa, on, off):
    eng, boot = on(10)
    d = boot.desc
    assert (d["depth"], d["K"], d["R"], d["cheb_degree"], d["sparse_h"]) == (DEPTH_ON, 12, 3, 28, H)
    assert len(d["cheb"]) == 29
    m, ct, r = _boot_input(eng, boot)
    assert eng.bootstrap(ct).info()["ell"] == eng.n_q - DEPTH_ON
    twin, tboot = off
    td = tboot.desc
    assert (td["depth"], td["K"], td["R"], td["cheb_degree"], td["sparse_h"]) == (DEPTH_OFF, 28, 3, 47, 0)
    assert twin.bootstrap_sparse_secret() == 0
    tm, tct, tr = _boot_input(twin, tboot)
    out = twin.bootstrap(tct)
    assert out.info()["ell"] == twin.n_q - DEPTH_OFF
    _same(out, tboot.run(tr), "the default path is the unmodified oracle class")
    for kind in (3, 4):
        assert _code(fa, twin.key_info, kind)[0] == ERR_ARG          # kinds of the knob: unknown without it: nothing was drawn or made


def _describe_words(eng):
    """fhelin_bootstrap_describe's raw words"""
    import ctypes as C
    n = C.c_int32()
    eng._ck(eng.lib.fhelin_bootstrap_describe(eng.h, None, 0, C.byref(n)))
    d = (C.c_int32 * n.value)()
    eng._ck(eng.lib.fhelin_bootstrap_describe(eng.h, d, n.value, C.byref(n)))
    return list(d)


def test_describe_trailer(on, off):
    """the stage table ends the words with the knob off; on, exactly the pair (2, h~) follows it"""
    for (eng, boot), tail in ((off, []), (on(10), [2, H])):
        d = boot.desc
        table = 9 + sum(2 + 2 * len(st["terms"]) for st in d["c2s"] + d["s2c"])
        words = _describe_words(eng)
        assert len(words) == table + len(tail) and words[table:] == tail


# ---- 3. it is a bootstrap -----------------------------------------------------------------------------------------------------------
def _fit_error(d):
    """max error of the exported cosine fit on 4097 points of [-1, 1] against cos((2 pi K y - pi/2) / 2^R)"""
    c = np.array(d["cheb"], dtype=np.float64)
    c[0] *= 0.5
    y = np.linspace(-1.0, 1.0, 4097)
    return float(np.max(np.abs(np.polynomial.chebyshev.chebval(y, c) - np.cos((2 * np.pi * d["K"] * y - np.pi / 2) / 2 ** d["R"]))))


def test_it_is_a_bootstrap(on, off):
    eng, boot = on(10)
    twin, tboot = off
    m, ct, _ = _boot_input(eng, boot)
    tm, tct, _ = _boot_input(twin, tboot)
    assert np.array_equal(m, tm)
    err = float(np.max(np.abs(eng.decrypt(eng.bootstrap(ct)) - m)))
    err_off = float(np.max(np.abs(twin.decrypt(twin.bootstrap(tct)) - tm)))
    print(f"max decryption error: sparse secret {err:.3e}, default {err_off:.3e}, ratio {err / err_off:.3f}")
    assert err < ABS_BOUND
    fit, fit_off = _fit_error(boot.desc), _fit_error(tboot.desc)
    print(f"cosine fit error on 4097 points: degree 28 at K = 12 {fit:.3e}, degree 47 at K = 28 {fit_off:.3e}")
    assert fit <= fit_off


# ---- 4. the secret and the keys -----------------------------------------------------------------------------------------------------
def test_the_ephemeral_secret_and_its_keys(fa, orc, on):
    eng, boot = on(10)
    s = eng.boot_sparse_secret()
    assert s.dtype == np.int8 and s.shape == (eng.N,)
    assert set(np.unique(s)) <= {-1, 0, 1} and int(np.count_nonzero(s)) == H
    q0 = int(eng.q[0])
    co = np.array([[int(v) % q0 for v in s]], dtype=np.uint64)
    assert not np.array_equal(orc.ntt_batch(co, eng.q[:1], eng.psi_q[:1])[0], eng.secret_export()[0])
    k3, k4 = eng.key_export(3), eng.key_export(4)
    i3, i4 = eng.key_info(3), eng.key_info(4)
    assert i3["max_ell"] == 2 and i3["digits"] == -(-2 // eng.alpha) == k3.shape[0]
    assert i4["max_ell"] == eng.n_q and i4["digits"] == eng.dnum_digits == k4.shape[0]
    # the key that targets s~ exists on two Q limbs and P only
    assert not k3[0][:, 2:eng.n_q].any() and not k3[1:].any()
    for half in range(2):
        for row in (0, 1, eng.n_q, eng.n_limbs - 1):
            assert k3[0][half][row].any()
    assert k4[-1][:, eng.n_q - 1].any()
    # the same seed gives the same secret and keys
    again = _engine(fa, 10)
    try:
        assert np.array_equal(again.boot_sparse_secret(), s)
        assert np.array_equal(again.key_export(3), k3) and np.array_equal(again.key_export(4), k4)
        assert np.array_equal(again.key_export(2), eng.key_export(2))
    finally:
        again.close()
    # the knob binds at set-up
    assert _code(fa, eng.set_bootstrap_sparse_secret, 0)[0] == ERR_STATE
    assert _code(fa, eng.set_bootstrap_sparse_secret, 64)[0] == ERR_STATE
    assert eng.bootstrap_sparse_secret() == H


# ---- 5. every pipeline goes through the same step -----------------------------------------------------------------------------------
def test_batch_pair_and_iterative(on):
    eng, boot = on(10)
    ins = [_boot_input(eng, boot, ell_left=k, seed=20 + k) for k in (3, 4, 2)]
    cts = [c for _, c, _ in ins]
    singles = [eng.bootstrap(c) for c in cts]
    for s, b in zip(singles, eng.bootstrap_batch(cts)):
        assert _equal(s, b)
    (ma, ca, _), (mb, cb, _) = ins[0], ins[1]
    pa, pb = eng.bootstrap_pair(ca, cb)
    ea, eb = float(np.max(np.abs(eng.decrypt(pa) - ma))), float(np.max(np.abs(eng.decrypt(pb) - mb)))
    print(f"pair error a {ea:.3e} b {eb:.3e}")
    assert ea < ABS_BOUND and eb < ABS_BOUND
    assert pa.info()["ell"] == pb.info()["ell"] == eng.n_q - DEPTH_ON
    out = eng.bootstrap_paired_batch(cts)
    assert _equal(out[0], pa) and _equal(out[1], pb)
    assert _equal(out[2], singles[2])                     # the odd last one travels as a single
    it = eng.bootstrap_iter(ca, 12)
    e1, e2 = float(np.max(np.abs(eng.decrypt(singles[0]) - ma))), float(np.max(np.abs(eng.decrypt(it) - ma)))
    print(f"single error {e1:.3e}, iterative (p = 12) error {e2:.3e}")
    assert e2 < e1 and it.info()["ell"] == eng.n_q - DEPTH_ON - 1


def test_key_switch_count(on, off):
    """two more key switches per pipeline item than the same stages would take without the knob"""
    eng, boot = on(10)
    m, ct, _ = _boot_input(eng, boot)
    s0 = eng.stats()
    eng.bootstrap_partial(ct, 1)
    s1 = eng.stats()
    twin, tboot = off
    tm, tct, _ = _boot_input(twin, tboot)
    t0 = twin.stats()
    twin.bootstrap_partial(tct, 1)
    t1 = twin.stats()
    assert (s1["keyswitch"] - s0["keyswitch"]) - (t1["keyswitch"] - t0["keyswitch"]) == 2
    # a pair is one pipeline item
    _, ct2, _ = _boot_input(eng, boot, seed=4)
    _, tct2, _ = _boot_input(twin, tboot, seed=4)
    eng.bootstrap_pair_partial(ct, ct2, 1)
    s2 = eng.stats()
    twin.bootstrap_pair_partial(tct, tct2, 1)
    t2 = twin.stats()
    assert (s2["keyswitch"] - s1["keyswitch"]) - (t2["keyswitch"] - t1["keyswitch"]) == 2


def test_with_the_linear_transform_knob(fa, on):
    eng = _engine(fa, 10, lt=True)
    try:
        d = eng.bootstrap_describe()
        assert d["lt"] and d["sparse_h"] == H and d["depth"] == DEPTH_ON
        m = np.random.default_rng(3).uniform(-1, 1, 1024)
        out = eng.bootstrap(eng.encrypt(m, level=eng.n_q - 3))
        err = float(np.max(np.abs(eng.decrypt(out) - m)))
        print(f"linear-transform knob and sparse secret: error {err:.3e}")
        assert err < ABS_BOUND and out.info()["ell"] == eng.n_q - DEPTH_ON
    finally:
        eng.close()


def test_interleaved_equals_the_stride_one_twin(fa, on):
    """stride 2 on 512 logical slots against the stride-1 engine at 1024 slots: the same seed and the same calls"""
    from test_interleave_gpu import _move
    B, _ = on(10)
    A = _engine(fa, 9, interleave=2)
    try:
        assert A.bootstrap_describe()["slots"] == 1024 and A.bootstrap_describe()["sparse_h"] == H
        assert np.array_equal(A.boot_sparse_secret(), B.boot_sparse_secret())
        assert np.array_equal(A.key_export(3), B.key_export(3)) and np.array_equal(A.key_export(4), B.key_export(4))
        z = np.random.default_rng(21).uniform(-0.5, 0.5, (1, 2, 512))
        ca = A.encrypt_interleaved_batch(z, level=A.n_q - 3)[0]
        cb = _move(ca, B, slots=1024)
        ya, yb = A.bootstrap(ca), B.bootstrap(cb)
        assert ya.slots == 512 and yb.slots == 1024
        assert np.array_equal(ya.export(), yb.export()) and ya.scale_parts() == yb.scale_parts()
        ia, ib = ya.info(), yb.info()
        assert (ia["ell"], ia["deg"]) == (ib["ell"], ib["deg"]) == (A.n_q - DEPTH_ON, 1)
        got = A.decrypt_interleaved(ya)
        assert max(float(np.max(np.abs(got[i] - z[0, i]))) for i in range(2)) < ABS_BOUND
    finally:
        A.close()


# ---- 6. key sets --------------------------------------------------------------------------------------------------------------------
def _entries(path, n_limbs):
    """(format magic, version, [(kind, last word)] of the key table) of a key-set file, from the documented layout"""
    b = open(path, "rb").read()
    magic, version, n_keys = b[:8], *struct.unpack_from("<II", b, 8)
    header = {b"FHELINEK": 96, b"FHELINEC": 128, b"FHELINEP": 136}[magic]
    entry = 40 if version == 1 and magic != b"FHELINEP" else 48
    table = header + 8 * n_limbs
    out = []
    for k in range(n_keys):
        at = table + entry * k
        out.append((struct.unpack_from("<I", b, at)[0], struct.unpack_from("<I", b, at + 44)[0] if entry == 48 else 0))
    return magic, version, out, len(b)


def test_key_sets_carry_the_knob(fa, on, tmp_path, monkeypatch):
    from test_evalkeys_gpu import move
    monkeypatch.delenv("FHELIN_BOOT_SPARSE_H", raising=False)
    cl = _engine(fa, 10, seeded=True)
    try:
        m = np.random.default_rng(3).uniform(-1, 1, 1024)
        ct = cl.encrypt(m, level=cl.n_q - 3)
        want = cl.bootstrap(ct)
        assert float(np.max(np.abs(cl.decrypt(want) - m))) < ABS_BOUND
        paths = {k: str(tmp_path / f"sparse.{k}") for k in ("full", "compact", "packed")}
        cl.save_eval_keys(paths["full"])
        cl.save_eval_keys(paths["compact"], compact=True)
        cl.save_evalkeys_packed(paths["packed"])
        for name, path in paths.items():
            magic, version, ent, _ = _entries(path, cl.n_limbs)
            kinds = [k for k, _ in ent]
            assert kinds[:5] == [0, 1, 3, 4, 5], (name, kinds[:5])         # after the conjugation key, in front of the rotations
            assert [w for k, w in ent if k in (4, 5)] == [H, H] and all(w == 0 for k, w in ent if k < 4)
            _, bt, _ = fa.Engine.eval_keys_params(path)
            assert (bt["K"], bt["R"], bt["cheb_degree"]) == (12, 3, 28)
            ev = fa.Engine.from_eval_keys(path, seed=4)                     # no call of the setter
            try:
                d = ev.bootstrap_describe()
                assert ev.bootstrap_sparse_secret() == H == d["sparse_h"] and d["depth"] == DEPTH_ON
                assert ev.key_info(3)["max_ell"] == 2 and ev.key_info(3)["seeded"] == (name == "compact")
                assert _equal(ev.bootstrap(move(ct, ev)), want), name
                assert _code(fa, ev.boot_sparse_secret)[0] == ERR_KEY       # an evaluation context never holds s~
            finally:
                ev.close()
    finally:
        cl.close()


def test_knob_off_sets_are_what_they_were(fa, off, tmp_path, monkeypatch):
    monkeypatch.delenv("FHELIN_BOOT_SPARSE_H", raising=False)
    twin, _ = off
    path = str(tmp_path / "off.evk")
    twin.save_eval_keys(path)
    magic, version, ent, size = _entries(path, twin.n_limbs)
    assert (magic, version) == (b"FHELINEK", 1) and not any(k >= 4 for k, _ in ent)
    # header, moduli, 40-byte entries, zeros up to 4096, then every key whole: 2 n_q N words for the public key, digits 2 (n_q + n_p) N each
    n_sw = len(ent) - 1
    table_end = 96 + 8 * twin.n_limbs + 40 * len(ent)
    assert size == -(-table_end // 4096) * 4096 + 8 * twin.N * (2 * twin.n_q + n_sw * twin.dnum_digits * 2 * twin.n_limbs)
    # the same set into a context with the knob on: the missing key is named at the set-up
    monkeypatch.setenv("FHELIN_BOOT_SPARSE_H", str(H))
    code, msg = _code(fa, fa.Engine.from_eval_keys, path, 0, 4)
    assert code == ERR_KEY and "to-sparse key" in msg, msg
    monkeypatch.delenv("FHELIN_BOOT_SPARSE_H")
    ev = fa.Engine.from_eval_keys(path, seed=4)
    try:
        assert ev.bootstrap_sparse_secret() == 0 and ev.bootstrap_describe()["depth"] == DEPTH_OFF
    finally:
        ev.close()


# ---- 7. the recorded cap table goes back in ------------------------------------------------------------------------------------------
def test_caps_recorded_from_a_sparse_bootstrap(fa, on):
    """record -> caps_from_usage -> set_key_caps with the knob on: the table names both new kinds, a fresh context of the same seed takes
    it as it is, holds the to-sparse key at two limbs whatever its entry says, and bootstraps to the same residues"""
    from test_evalkeys_gpu import move
    eng, boot = on(10)
    m, ct, _ = _boot_input(eng, boot)
    with eng.key_usage() as u:
        want = eng.bootstrap(ct)
        eng.sync()
    table = u.table
    sparse = {(k, g): ell for k, g, ell in table if k in (4, 5)}
    assert sparse == {(4, 0): 2, (5, 0): eng.n_q}
    caps = fa.caps_from_usage(table, eng.n_q)
    assert caps == table
    caps = [(k, g, 5 if k == 4 else ell) for k, g, ell in caps]       # whatever the table says about the to-sparse key
    capped = fa.Engine("boot12", seed=77, log_slots=10)
    try:
        assert _code(fa, capped.set_key_caps, caps)[0] == ERR_ARG      # the two kinds belong to the knob: set it first
        capped.set_bootstrap_sparse_secret(H)
        capped.set_key_caps(caps)
        capped.keygen()
        capped.gen_relin_key()
        capped.bootstrap_setup(3, 3, 1 << 10)
        assert capped.key_info(3)["max_ell"] == 2 and capped.key_info(4)["max_ell"] == eng.n_q
        assert np.array_equal(capped.key_export(3), eng.key_export(3))
        got = capped.bootstrap(move(ct, capped))
        assert _equal(got, want)
        assert _code(fa, capped.set_key_caps, [(5, 0, 3)])[0] == ERR_STATE      # the key is held: caps apply to keys made afterwards
    finally:
        capped.close()
