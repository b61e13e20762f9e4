"""The content-keyed plaintext cache of fhelin_encode (capi_internal.h PtCache).

A second encode of the same (n, slots, level hint, value bytes) gives a handle that shares the first one's device encodings; nothing else
may change.  Every case runs on two engines of the same seed, one of them with FHELIN_PT_CACHE=0 (every encode a plaintext of its own,
the behaviour before the cache): ciphertext residues and pt_export bytes must be equal."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _engine(fa, **env):
    """a toy context (N = 2^12) created under the given knobs (they are read when the context is created)"""
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return fa.Engine("toy", device=0, seed=1)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.fixture(scope="module")
def pair(fa):
    on, off = _engine(fa, FHELIN_PT_CACHE="1"), _engine(fa, FHELIN_PT_CACHE="0")
    for e in (on, off):
        e.keygen()
    yield on, off
    on.close()
    off.close()


@pytest.fixture(scope="module")
def cts(orc, pair):
    """the same two ciphertexts (5 and 3 limbs) in both engines"""
    on, _ = pair
    return {ell: np.stack([orc.uniform_residues(31 + ell + 1000 * p, on.q[:ell], on.N) for p in range(2)]) for ell in (5, 3)}


def _vec(eng, seed):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, 1 << eng.params.log_slots)


def _use(eng, cts, pts):
    """every plaintext multiplied and added at both levels: exported residues, then the encodings themselves"""
    out = []
    for ell, x in cts.items():
        c = eng.ct_import(x)
        for p in pts:
            out.append(eng.mult(c, p).export())
            out.append(eng.add(c, p).export())
    for p in pts:
        for ell in cts:
            out.append(eng.pt_export(p, ell))
    return out


def _equal(a, b):
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert np.array_equal(x, y), i


def test_same_values_encoded_twice(pair, cts):
    on, off = pair
    v = _vec(on, 1)
    res, enc = {}, {}
    for name, eng in (("on", on), ("off", off)):
        entries = eng.cache_stats()["pt_cache_entries"]
        p1, p2 = eng.encode(v), eng.encode(v.copy())
        enc[name + "_entries"] = eng.cache_stats()["pt_cache_entries"] - entries
        before = eng.stats()["encode"]
        res[name] = _use(eng, cts, [p1, p2])
        enc[name] = eng.stats()["encode"] - before
    # mult_plain and add_plain of an imported ciphertext meet the plaintext at the same (limbs, Delta of the level): one encoding per
    # level for the shared plaintext, one per level and handle without the cache
    assert (enc["on"], enc["off"]) == (2, 4)
    assert (enc["on_entries"], enc["off_entries"]) == (1, 0)
    _equal(res["on"], res["off"])


def test_vectors_that_must_not_collide(pair, cts):
    on, off = pair
    v = _vec(on, 2)
    v[3] = 0.0
    one_slot = v.copy()
    one_slot[777] += 2.0 ** -40
    neg_zero = v.copy()
    neg_zero[3] = -0.0
    half = v[:1024]
    specs = [(v, 0, 0), (one_slot, 0, 0), (neg_zero, 0, 0), (half, 0, 1024), (half, 0, 2048), (v, 1, 0)]   # (values, level hint, slots)
    entries = on.cache_stats()["pt_cache_entries"]
    pts_on = [on.encode(a, lvl, s) for a, lvl, s in specs]
    assert on.cache_stats()["pt_cache_entries"] - entries == len(specs), "every vector is an entry of its own"
    pts_off = [off.encode(a, lvl, s) for a, lvl, s in specs]
    r_on, r_off = _use(on, cts, pts_on), _use(off, cts, pts_off)
    _equal(r_on, r_off)
    n = len(specs)
    tail = r_on[-2 * n:]                        # pt_export of plaintext i at 5 limbs: tail[2 i]
    assert not np.array_equal(tail[0], tail[2]), "one slot changed, same encoding"
    assert not np.array_equal(tail[6], tail[8]), "1024 and 2048 slots, same encoding"
    for eng, pts in ((on, pts_on), (off, pts_off)):   # the level hint decides where an encryption starts
        assert [eng.encrypt(pts[i]).info()["ell"] for i in (0, 5)] == [eng.n_q, eng.n_q - 1]


def test_caller_changes_its_array_after_encode(pair, cts):
    on, off = pair
    v = _vec(on, 3)
    a = v.copy()
    p = on.encode(a)
    entries = on.cache_stats()["pt_cache_entries"]
    a[0] += 1.0                                                # the library copied the values: the entry still holds the old ones
    again = on.encode(v)
    assert on.cache_stats()["pt_cache_entries"] == entries, "the old values are still a hit"
    changed = on.encode(a)
    assert on.cache_stats()["pt_cache_entries"] == entries + 1, "the changed array is a new entry"
    _equal(_use(on, cts, [p, again, changed]), _use(off, cts, [off.encode(v), off.encode(v), off.encode(a)]))


def test_eviction(fa, pair, cts):
    """cap 1 MB; a toy plaintext exported at 6, 5, 4 and 3 limbs holds 18 limbs x 32 KiB = 576 KiB: the third plaintext finds 1152 KiB
    held and evicts the first"""
    _, off = pair
    small = _engine(fa, FHELIN_PT_CACHE="1", FHELIN_PT_CACHE_MB="1")
    try:
        vs = [_vec(small, 10 + i) for i in range(3)]
        pts, got = [], []
        for i, v in enumerate(vs):
            pts.append(small.encode(v))
            st = small.cache_stats()
            assert st["pt_cache_entries"] == (i + 1 if i < 2 else 2), st
            got += [small.pt_export(pts[-1], ell) for ell in (6, 5, 4, 3)]
            assert small.cache_stats()["pt_cache_bytes"] == min(i + 1, 2) * 18 * 8 * small.N
        first_again = small.encode(vs[0])                       # evicted: a new plaintext, which in turn evicts the second
        assert small.cache_stats()["pt_cache_entries"] == 2
        got += _use(small, cts, pts + [first_again])            # the evicted plaintext's handle still works
        want = []
        ref = [off.encode(v) for v in vs]
        for p in ref:
            want += [off.pt_export(p, ell) for ell in (6, 5, 4, 3)]
        want += _use(off, cts, ref + [off.encode(vs[0])])
        _equal(got, want)
    finally:
        small.close()


def test_free_every_handle(fa, cts):
    """fhelin_pt_free drops the handle's reference only: the cache keeps the encodings until the context is trimmed or closed"""
    eng = _engine(fa, FHELIN_PT_CACHE="1")
    eng.sync()
    base = eng.cache_stats()["pool_live_bytes"]                 # the context's own tables
    pts = [eng.encode(_vec(eng, 20 + i)) for i in range(3)] + [eng.encode(_vec(eng, 20))]
    c = eng.ct_import(cts[5])
    outs = [eng.mult(c, p) for p in pts]
    eng.sync()
    for h in outs + [c]:
        h.free()
    for p in pts:
        p.free()
    eng.sync()
    st = eng.cache_stats()
    assert st["pt_cache_entries"] == 3 and st["pt_cache_bytes"] == 3 * 5 * 8 * eng.N
    assert st["pool_live_bytes"] >= base + st["pt_cache_bytes"], "the cached encodings are still in use"
    eng.trim()
    st = eng.cache_stats()
    assert (st["pt_cache_entries"], st["pt_cache_bytes"], st["pool_live_bytes"]) == (0, 0, base)
    p = eng.encode(_vec(eng, 20))                               # the context closes with an entry and a live handle to it
    eng.pt_export(p, 4)
    p.free()
    eng.close()
