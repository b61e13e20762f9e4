"""Level-capped keys on the GPU (include/fhelin.h "Level-capped keys").  Two contexts from one secret seed - A uncapped, B with a cap
table - show the sub-block rule (B's keys are the present rows of A's, in default and in seeded-key mode, and keys made afterwards are
unchanged), bit-identical evaluation of every key-switching family at every ell <= cap, the refusal above the cap, the version 2 key
sets, and the usage recorder.  Shapes: toy (6+2 limbs, alpha 2: caps 1, 2, 3, 5 hold 1, 1, 2, 3 digits, a partial and a full last
digit), toy13 (7+3, alpha 3: caps 3 and 4), boot12 for the bootstrap."""
import struct

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_STATE, ERR_KEY = 1, 4, 5

# rotation index -> cap on toy; index 7 is generated after all of these and stays uncapped
TOY_ROT = {1: 3, 2: 3, 3: 3, 5: 5, -1: 1, 4: 2}
TOY_RELIN, TOY_CONJ = 3, 2
LATE = 7


def _g(e, r):
    return pow(5, r % (e.N // 2), 2 * e.N)


def _client(fa, preset, rot_caps, relin_cap, conj_cap, capped, seeded, late=(LATE,), seed=77):
    e = fa.Engine(preset, seed=seed)
    if seeded:
        e.set_seeded_keys(True)
    if capped:
        table = [(2, _g(e, r), c) for r, c in rot_caps.items()]
        if relin_cap:
            table.append((1, 0, relin_cap))
        if conj_cap:
            table.append((3, 2 * e.N - 1, conj_cap))
        e.set_key_caps(table)
    e.keygen()
    e.gen_relin_key()
    e.gen_rotation_keys(list(rot_caps))
    e.gen_conj_key()
    e.gen_rotation_keys(list(late))
    return e


@pytest.fixture(scope="module", params=[False, True], ids=["default", "seeded"])
def toy(fa, request):
    """(A, B, seeded): the uncapped and the capped client of one seed on toy, once per key mode"""
    a = _client(fa, "toy", TOY_ROT, TOY_RELIN, TOY_CONJ, False, request.param)
    b = _client(fa, "toy", TOY_ROT, TOY_RELIN, TOY_CONJ, True, request.param)
    yield a, b, request.param
    a.close()
    b.close()


def _digits(e, cap):
    return -(-cap // e.alpha)


def _check_sub_block(a, b, kind, index, cap):
    """B's key: digits_at(cap) digits; present rows = A's, residue for residue; absent rows zero (A's are not)"""
    ka, kb = a.key_export(kind, index), b.key_export(kind, index)
    d, n_q = _digits(b, cap), b.n_q
    assert b.key_info(kind, index) == dict(digits=d, max_ell=cap, seeded=a.key_info(kind, index)["seeded"])
    assert a.key_info(kind, index)["digits"] == a.dnum_digits and a.key_info(kind, index)["max_ell"] == n_q
    assert ka.shape[0] == a.dnum_digits and kb.shape == (d, 2, b.n_limbs, b.N)
    assert np.array_equal(kb[:, :, :cap], ka[:d, :, :cap]), (kind, index, "Q rows")
    assert np.array_equal(kb[:, :, n_q:], ka[:d, :, n_q:]), (kind, index, "special rows")
    if cap < n_q:
        assert not kb[:, :, cap:n_q].any(), (kind, index, "absent rows")
        assert ka[:d, :, cap:n_q].any()      # rows the uncapped key does hold: B's zeros there are never read (evaluation tests)


def test_sub_block_rule(toy):
    a, b, seeded = toy
    assert b.alpha == 2 and [_digits(b, c) for c in (1, 2, 3, 5)] == [1, 1, 2, 3]
    for r, cap in TOY_ROT.items():
        _check_sub_block(a, b, 1, r, cap)
    _check_sub_block(a, b, 0, 0, TOY_RELIN)
    _check_sub_block(a, b, 2, 0, TOY_CONJ)
    # the key generated after all the capped ones: uncapped and identical - the generators were consumed alike
    assert b.key_info(1, LATE) == dict(digits=b.dnum_digits, max_ell=b.n_q, seeded=seeded)
    assert np.array_equal(a.key_export(1, LATE), b.key_export(1, LATE))
    # ... and so is everything else drawn afterwards: a fresh encryption
    v = np.linspace(-1, 1, 1 << a.params.log_slots)
    assert np.array_equal(a.encrypt(v).export(), b.encrypt(v).export())


def test_sub_block_rule_toy13(fa):
    caps = {1: 3, 2: 4}
    for seeded in (False, True):
        a = _client(fa, "toy13", caps, 4, 3, False, seeded, late=(3,))
        b = _client(fa, "toy13", caps, 4, 3, True, seeded, late=(3,))
        try:
            assert b.alpha == 3
            for r, cap in caps.items():
                _check_sub_block(a, b, 1, r, cap)      # cap 3: one full digit; cap 4: two digits, the last partial
            _check_sub_block(a, b, 0, 0, 4)
            _check_sub_block(a, b, 2, 0, 3)
            assert np.array_equal(a.key_export(1, 3), b.key_export(1, 3))
        finally:
            a.close()
            b.close()


# ---- evaluation

def _ct(e, ell, seed, deg=1):
    rng = np.random.default_rng(seed)
    limbs = np.stack([np.stack([rng.integers(0, int(q), e.N, dtype=np.uint64) for q in e.q[:ell]]) for _ in range(2)])
    return e.ct_import(limbs, deg=deg)


def _pts(e, n, seed):
    rng = np.random.default_rng(seed)
    return [e.encode(rng.uniform(-1, 1, 1 << e.params.log_slots)) for _ in range(n)]


def _lt(e):
    rng = np.random.default_rng(5)
    return e.lt_create(rng.uniform(-1, 1, (4, 1 << e.params.log_slots)), [0, 1, 2, 3], n1=2)


def _ex(x):
    return [c.export() for c in x] if isinstance(x, (list, tuple)) else [x.export()]


# every family of the interface that binds a key, over the keys capped at 3 limbs (indices 1, 2, 3; the relinearisation key)
def _families(e, ell):
    x = [_ct(e, ell, 10 + i) for i in range(3)]
    pts = _pts(e, 3, 3)
    fam = {
        "rotate": lambda: e.rotate(x[0], 1),
        "rotate_batch": lambda: e.rotate_batch(x, 2),
        "rotate_many": lambda: e.rotate_many(x[0], [1, 2, 3]),
        "rotate_each": lambda: e.rotate_each(x, [1, 2, 3]),
        "rotate_sum": lambda: e.rotate_sum(x, [1, 2, 3]),
        "rotate_each_sum": lambda: e.rotate_each_sum(x, [1, 2, 3]),
        "hoisted_dot": lambda: e.hoisted_dot(x, pts, [1, 2]),
        "lt_apply": lambda: e.lt_apply(_lt(e), x),
        "mult": lambda: e.mult(x[0], x[1]),
        "mult_batch": lambda: e.mult_batch(x[:2], x[1:]),
        "raw_rotate": lambda: e.raw_rotate(x[0], 3),
    }
    if ell >= 2:
        fam["hoisted_dot_rescale"] = lambda: e.hoisted_dot(x, pts, [1, 2], rescale=True)
        fam["mult_affine_batch"] = lambda: e.mult_affine_batch(x[:2], x[1:], [2, 1], [-1.0, 0.5], [None, x[0]], [0, 1])
    return fam


@pytest.mark.parametrize("ell", [3, 2, 1])     # the cap (two digits, the last partial); one full digit; a single limb
def test_bit_identical_at_and_below_the_cap(toy, ell):
    a, b, _ = toy
    assert sorted(_lt(a).rotations()) == [1, 2]
    fa_, fb_ = _families(a, ell), _families(b, ell)
    for name in fa_:
        got, want = _ex(fb_[name]()), _ex(fa_[name]())
        assert len(got) == len(want)
        for g, w in zip(got, want):
            assert np.array_equal(g, w), (name, ell)


@pytest.mark.parametrize("index,ells", [(5, (5, 4)), (4, (2, 1)), (-1, (1,))])
def test_bit_identical_other_caps(toy, index, ells):
    """cap 5: three digits, the last partial (ell 5) / unused (ell 4); cap 2: one full digit; cap 1: one limb"""
    a, b, _ = toy
    for ell in ells:
        assert np.array_equal(b.rotate(_ct(b, ell, 40), index).export(), a.rotate(_ct(a, ell, 40), index).export()), (index, ell)


def test_capped_key_against_the_oracle(fa, orc):
    """raw_rotate with a capped key at ell = cap equals the oracle's rotation with that key zero-padded to [dnum][2][L+1+k][N]"""
    e = _client(fa, "toy13", {1: 4}, 0, 0, True, False, late=())
    try:
        key = e.key_export(1, 1)
        assert key.shape[0] == 2 and e.dnum_digits == 3
        evk = np.zeros((e.dnum_digits, 2, e.n_limbs, e.N), dtype=np.uint64)
        evk[:2] = key
        for ell in (4, 3):
            ct = np.stack([orc.uniform_residues(7 + 1000 * p, e.q[:ell], e.N) for p in range(2)])
            want = orc.rotate(ct, evk, orc.galois(e.log_n, 1), e.alpha, e.q, e.p, e.psi_q, e.psi_p)
            assert np.array_equal(e.raw_rotate(e.ct_import(ct), 1).export(), want), ell
    finally:
        e.close()


def test_refusal_above_the_cap(fa, toy):
    a, b, _ = toy
    ell = 4     # cap 3 + 1
    fam_b = _families(b, ell)
    for name, fn in fam_b.items():
        before = b.stats()["keyswitch"]
        with pytest.raises(fa.FhelinError) as ei:
            fn()
        msg = str(ei.value)
        assert ei.value.code == ERR_KEY, (name, msg)
        assert "capped at 3 limbs" in msg and "at 4 limbs" in msg, (name, msg)
        if name.startswith("mult"):
            assert "relinearisation key" in msg, (name, msg)
        else:
            assert any(f"index {r} (Galois element {_g(b, r)})" in msg for r in (1, 2, 3)), (name, msg)
        assert b.stats()["keyswitch"] == before, name
    # a mixed batch - one row within the cap, one above - is refused as a whole, before the row within the cap runs
    before = b.stats()["keyswitch"]
    with pytest.raises(fa.FhelinError) as ei:
        b.rotate_sum([_ct(b, 3, 1), _ct(b, 4, 2)], [1, 2, 3])
    assert ei.value.code == ERR_KEY and b.stats()["keyswitch"] == before
    # in a deferred unit the refusal surfaces where that unit's errors surface: at the read that forces it, with the same code
    # (with FHELIN_LAZY_HEAVY=0 nothing is deferred and the call itself refuses)
    with pytest.raises(fa.FhelinError) as ei:
        y = b.eval_chebyshev(_ct(b, 5, 6), [0.1, 0.2, 0.3, 0.4])      # T_2 multiplies at 5 limbs, the relinearisation key holds 3
        y.export()
    assert ei.value.code == ERR_KEY and "relinearisation key is capped at 3 limbs" in str(ei.value)
    # the uncapped context evaluates the same calls, and the next valid call on B still matches it
    for name, fn in _families(a, ell).items():
        fn()
    assert np.array_equal(b.rotate_sum([_ct(b, 3, 1)], [1, 2, 3])[0].export(), a.rotate_sum([_ct(a, 3, 1)], [1, 2, 3])[0].export())
    assert np.array_equal(b.rotate(_ct(b, 6, 1), LATE).export(), a.rotate(_ct(a, 6, 1), LATE).export())   # an uncapped key: any level


def test_set_key_caps_state_errors(fa, toy, tmp_path):
    a, b, _ = toy
    with pytest.raises(fa.FhelinError) as ei:
        b.set_key_caps([(2, _g(b, 9), 2), (2, _g(b, 1), 2)])      # index 1 is held
    assert ei.value.code == ERR_STATE
    with pytest.raises(fa.FhelinError) as ei:
        b.set_key_caps([(1, 0, 2)])
    assert ei.value.code == ERR_STATE
    b.gen_rotation_keys([9])                                       # the refused table changed nothing: index 9 is uncapped
    assert b.key_info(1, 9)["max_ell"] == b.n_q
    path = str(tmp_path / "a.evk")
    a.save_eval_keys(path)
    c = fa.Engine("toy")
    try:
        c.load_eval_keys(path)
        with pytest.raises(fa.FhelinError) as ei:
            c.set_key_caps([(2, _g(c, 11), 2)])
        assert ei.value.code == ERR_KEY
    finally:
        c.close()


# ---- files

def _table(data):
    compact = data[:8] == b"FHELINEC"
    version, n_keys = struct.unpack_from("<II", data, 8)
    prm = struct.unpack_from("<9i", data, 16)
    data_offset = struct.unpack_from("<Q", data, 80)[0]
    base = (128 if compact else 96) + 8 * (prm[1] + prm[4])
    size = 48 if version == 2 else 40
    ents = []
    for k in range(n_keys):
        kind, digits, g, off, words, dg = struct.unpack_from("<IIQQQQ", data, base + size * k)
        max_ell, rsv = struct.unpack_from("<II", data, base + size * k + 40) if version == 2 else (prm[1], 0)
        ents.append(dict(kind=kind, digits=digits, galois=g, offset=off, words=words, digest=dg, max_ell=max_ell, reserved=rsv,
                         at=base + size * k))
    return version, data_offset, base + size * n_keys, ents


def _expected_caps(e):
    want = {(1, 0): TOY_RELIN, (3, 2 * e.N - 1): TOY_CONJ}
    want.update({(2, _g(e, r)): c for r, c in TOY_ROT.items()})
    return want


def _eval_some(e):
    return [e.rotate(_ct(e, 3, 1), 1).export(), e.rotate_sum([_ct(e, 2, 2)], [1, 2, 3])[0].export(), e.mult(_ct(e, 3, 3), _ct(e, 3, 4)).export(),
            e.rotate(_ct(e, 5, 5), 5).export(), e.rotate(_ct(e, 6, 6), LATE).export()]


@pytest.mark.parametrize("compact", [False, True], ids=["full", "compact"])
def test_version2_set_round_trip(fa, tmp_path, compact):
    b = _client(fa, "toy", TOY_ROT, TOY_RELIN, TOY_CONJ, True, True)
    c = fa.Engine("toy")
    c2 = fa.Engine("toy")
    try:
        path, other = str(tmp_path / "b.evk"), str(tmp_path / "b.other")
        b.save_eval_keys(path, compact=compact)
        b.save_eval_keys(other, compact=not compact)
        data = open(path, "rb").read()
        N, n_q, n_p = b.N, b.n_q, b.n_p
        version, data_offset, table_end, ents = _table(data)
        assert version == 2 and data[:8] == (b"FHELINEC" if compact else b"FHELINEK")
        assert data_offset == -(-table_end // 4096) * 4096
        caps, halves, at = _expected_caps(b), (1 if compact else 2), data_offset
        assert len(ents) == 1 + 2 + len(TOY_ROT) + 1
        for en in ents:
            cap = n_q if en["kind"] == 0 else caps.get((en["kind"], en["galois"]), n_q)
            assert en["max_ell"] == cap and en["reserved"] == 0 and en["offset"] == at
            want = halves * n_q * N if en["kind"] == 0 else _digits(b, cap) * halves * (cap + n_p) * N
            assert en["words"] == want and en["digits"] == (0 if en["kind"] == 0 else _digits(b, cap))
            at += 8 * en["words"]
        assert len(data) == at                               # the formula, exactly
        # the compact set carries the full set's digests
        assert [en["digest"] for en in ents] == [en["digest"] for en in _table(open(other, "rb").read())[3]]
        if not compact:   # the payload is the present rows of the key, dense, and the digest covers what is stored
            from test_evalkeys_host import key_digest
            en = next(x for x in ents if (x["kind"], x["galois"]) == (2, _g(b, 1)))
            stored = np.frombuffer(data, dtype=np.uint64, count=en["words"], offset=en["offset"]).reshape(2, 2, 3 + n_p, N)
            key = b.key_export(1, 1)
            assert np.array_equal(stored[:, :, :3], key[:, :, :3]) and np.array_equal(stored[:, :, 3:], key[:, :, n_q:])
            assert key_digest(stored, N) == en["digest"]
        # a fresh evaluation context: the same keys, the same results, the same refusals, the same bytes
        c.load_eval_keys(path)
        for r, cap in TOY_ROT.items():
            assert c.key_info(1, r) == dict(digits=_digits(b, cap), max_ell=cap, seeded=compact)
            assert np.array_equal(c.key_export(1, r), b.key_export(1, r))
        assert np.array_equal(c.key_export(0), b.key_export(0)) and np.array_equal(c.key_export(2), b.key_export(2))
        for g, w in zip(_eval_some(c), _eval_some(b)):
            assert np.array_equal(g, w)
        with pytest.raises(fa.FhelinError) as ei:
            c.rotate(_ct(c, 4, 1), 1)
        assert ei.value.code == ERR_KEY and "capped at 3 limbs" in str(ei.value)
        again = str(tmp_path / "c.evk")
        c.save_eval_keys(again, compact=compact)
        assert open(again, "rb").read() == data
        # corruptions: FHELIN_ERR_ARG, and the context stays empty (it then loads the good set)
        en = next(x for x in ents if (x["kind"], x["galois"]) == (2, _g(b, 1)))
        bad = {}
        flip = bytearray(data)
        flip[en["offset"] + 8 * 5] ^= 1
        bad["payload word"] = bytes(flip)
        for name, off, val in (("max_ell", 40, 2), ("digits", 4, 1), ("reserved", 44, 1)):
            m = bytearray(data)
            struct.pack_into("<I", m, en["at"] + off, val)
            bad[name] = bytes(m)
        for name, blob in bad.items():
            p = str(tmp_path / "bad.evk")
            open(p, "wb").write(blob)
            with pytest.raises(fa.FhelinError) as ei:
                c2.load_eval_keys(p)
            assert ei.value.code == ERR_ARG, name
            with pytest.raises(fa.FhelinError) as ei:
                c2.key_info(1, 1)
            assert ei.value.code == ERR_KEY, name
        c2.load_eval_keys(path)
        assert np.array_equal(c2.key_export(1, 1), b.key_export(1, 1))
    finally:
        b.close()
        c.close()
        c2.close()


def test_uncapped_context_still_writes_version1(fa, toy, tmp_path):
    a, b, seeded = toy
    forms = (False, True) if seeded else (False,)
    for compact in forms:
        path = str(tmp_path / "a.evk")
        a.save_eval_keys(path, compact=compact)
        data = open(path, "rb").read()
        version, data_offset, table_end, ents = _table(data)
        halves, nl = (1 if compact else 2), a.n_limbs
        assert version == 1 and table_end == (128 if compact else 96) + 8 * nl + 40 * len(ents)
        n_sw = len(ents) - 1
        assert len(data) == data_offset + 8 * (halves * a.n_q * a.N + n_sw * a.dnum_digits * halves * nl * a.N)
        c = fa.Engine("toy")
        try:
            c.load_eval_keys(path)        # a version 1 set still loads, its keys uncapped
            assert c.key_info(1, 1) == dict(digits=a.dnum_digits, max_ell=a.n_q, seeded=compact)
            assert np.array_equal(c.rotate(_ct(c, 6, 1), 1).export(), a.rotate(_ct(a, 6, 1), 1).export())
        finally:
            c.close()


# ---- usage

def test_usage_table_of_a_scripted_sequence(toy):
    a, _, _ = toy
    with a.key_usage() as u:
        a.rotate(_ct(a, 2, 1), 1)
        a.rotate(_ct(a, 3, 2), 1)                                  # max(ell) per key: 3 for index 1
        a.rotate_sum([_ct(a, 2, 3)], [1, 2, 3])                    # indices 2 and 3 at 2 limbs
        a.mult(_ct(a, 2, 4), _ct(a, 2, 5))                         # the relinearisation key at 2 limbs ...
        y = a.eval_chebyshev(_ct(a, 5, 6), [0.1, 0.2, 0.3, 0.4])   # ... and, deferred, at 5: T_2 = 2 x^2 - 1 multiplies at x's limbs
        a.rotate(_ct(a, 6, 7), LATE)
    assert u.table == sorted([(1, 0, 5), (2, _g(a, 1), 3), (2, _g(a, 2), 2), (2, _g(a, 3), 2), (2, _g(a, LATE), 6)])
    assert y.info()["ell"] >= 1
    with a.key_usage() as u:          # a new recording starts empty; a key that was never used has no entry
        a.rotate(_ct(a, 1, 1), -1)
    assert u.table == [(2, _g(a, -1), 1)]


# two circuit rotations no bootstrap stage uses (its stages rotate by j, 16 j and 128 j with |j| < 16 at 1024 slots)
BOOT_R4, BOOT_R2 = 777, 555


def _boot_client(fa, caps=None):
    e = fa.Engine("boot12", seed=77, log_slots=10)
    e.set_seeded_keys(True)
    if caps is not None:
        e.set_key_caps(caps)
    e.keygen()
    e.gen_relin_key()
    e.bootstrap_setup(3, 3, 1 << 10)
    e.gen_rotation_keys([BOOT_R4, BOOT_R2])
    return e


def _boot_pass(e):
    rng = np.random.default_rng(3)
    m = [rng.uniform(-1, 1, 1 << 10) for _ in range(3)]
    x = [e.encrypt(v, level=e.n_q - 3) for v in m]
    out = [e.bootstrap(x[0])]
    out += list(e.bootstrap_pair(x[1], x[2]))          # its conjugations run through the conjugation key
    out += [e.rotate(e.level_reduce(out[0], 4), BOOT_R4), e.rotate(e.level_reduce(out[1], 2), BOOT_R2)]
    return [c.export() for c in out]


def test_caps_recorded_from_a_bootstrap(fa, tmp_path):
    a = _boot_client(fa)
    try:
        with a.key_usage() as u:
            want = _boot_pass(a)
        table = u.table
        n_q = a.n_q
        assert (3, 2 * a.N - 1) in {(k, g) for k, g, _ in table}            # the conjugation key, once, as kind 3
        assert len({(k, g) for k, g, _ in table}) == len(table) and table == sorted(table)
        used = {(k, g): m for k, g, m in table}
        assert used[(2, _g(a, BOOT_R4))] == 4 and used[(2, _g(a, BOOT_R2))] == 2
        caps = fa.caps_from_usage(table, n_q)
        boot_capped = [c for c in caps if c[2] < n_q and c[1] not in (_g(a, BOOT_R4), _g(a, BOOT_R2))]
        assert boot_capped, "no bootstrapping key comes out capped"
        pa = str(tmp_path / "a.evc")
        a.save_eval_keys(pa, compact=True)
    finally:
        a.close()
    b = _boot_client(fa, caps)
    try:
        got = _boot_pass(b)
        assert len(got) == len(want)
        for g, w in zip(got, want):
            assert np.array_equal(g, w)                                      # the capped context's pass, bit for bit
        pb = str(tmp_path / "b.evc")
        b.save_eval_keys(pb, compact=True)
        import os
        assert os.path.getsize(pb) < os.path.getsize(pa)
        # above the recorded use the pass is refused, it does not misdecrypt
        with pytest.raises(fa.FhelinError) as ei:
            b.rotate(b.encrypt(np.zeros(1 << 10), level=n_q - 5), BOOT_R4)
        assert ei.value.code == ERR_KEY and "capped at 4 limbs" in str(ei.value)
    finally:
        b.close()
