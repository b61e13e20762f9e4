"""tests/test_stale_memory_gpu.py continued: the client side, keys, reply sanitisation, the composites with real keys and bootstrapping,
each on the three engines (FHELIN_POOL_FILL off, 1, 2) with identical inputs and twice over.  The engines share one seed, so they draw the
same secret, the same encryption randomness and the same flood terms: every exported residue, decrypted double and file byte is equal."""
import numpy as np
import pytest

from stale_memory import LD, make_trios, run
from test_default_path_gpu import _ct
from test_wrapped_interleaved_gpu import UNWRAP_KEYS, _embs, _expanded, _ring, _shared

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def trios(fa):
    """(preset, overrides) -> [engine with the knob off, with w = 1, with w = 2]: the same arguments and the same non-zero seed"""
    yield from make_trios(fa)


# ------------------------------------------------------------------------------------------------ client and keys: the three engines agree
def _with_keys(eng):
    if not getattr(eng, "_stale_keygen", False):
        eng.keygen()
        eng._stale_keygen = True


def _client_scenario(s):
    eng = s.eng
    _with_keys(eng)
    ns = 1 << eng.params.log_slots
    rng = np.random.default_rng(s.seed(5))
    v = rng.uniform(-1, 1, ns)
    rows = rng.uniform(-1, 1, (3, ns))
    pt = eng.encode(v)
    s.raw("encode, pt_export", eng.pt_export(pt, eng.n_q))
    s.raw("encode, pt_export at 2 limbs", eng.pt_export(pt, 2))
    c = s.operand(eng.encrypt(v), "encrypt")
    s.out("encrypt", c)
    cts = [s.operand(x, "encrypt_batch") for x in eng.encrypt_batch(rows)]
    for i, x in enumerate(cts):
        s.out(f"encrypt_batch {i}", x)
    low = s.operand(eng.encrypt(v, level=eng.n_q - 2), "encrypt at 2 limbs")
    s.out("encrypt at 2 limbs", low)
    d = eng.decrypt(c)
    s.raw("decrypt", d)
    assert np.max(np.abs(d[:ns] - v)) < 1e-6
    db = eng.decrypt_batch(cts + [low])
    s.raw("decrypt_batch", db)
    assert np.max(np.abs(np.asarray(db)[:3, :ns] - rows)) < 1e-6
    s.raw("decrypt_batch, slot list", eng.decrypt_batch(cts, idx=[0, 5, ns - 1]))
    s.raw("decrypt_batch, flooded", eng.decrypt_batch(cts, flood_bits=20))


def test_encode_encrypt_decrypt(trios, orc):
    run(trios("toy"), orc, _client_scenario)


@pytest.mark.parametrize("seeded", [False, True])
def test_key_generation_and_key_set_file(trios, orc, tmp_path, seeded):
    """key generation, plain and seeded: exported relinearisation and rotation key residues; an evaluation-key set (full / compact):
    file bytes.  The second round generates a new key set on the same context."""
    def scen(s):
        eng = s.eng
        if seeded and not getattr(eng, "_stale_seeded", False):
            eng.set_seeded_keys(True)                    # once, while the context holds no key
            eng._stale_seeded = True
        eng.keygen()
        eng.gen_relin_key()
        eng.gen_rotation_keys([1, -3])
        s.raw("secret", eng.secret_export())
        s.raw("relin key", eng.key_export(0))
        s.raw("rotation key 1", eng.key_export(1, 1))
        s.raw("rotation key -3", eng.key_export(1, -3))
        path = str(tmp_path / f"keys_{s.rnd}_{s.k}.bin")
        eng.save_eval_keys(path, compact=seeded)
        with open(path, "rb") as f:
            s.raw("key set file", np.frombuffer(f.read(), dtype=np.uint8))
    run(trios("toy", tag=("keys", seeded)), orc, scen)


def test_compact_round_trip(trios, orc):
    def scen(s):
        eng = s.eng
        _with_keys(eng)
        ns = 1 << eng.params.log_slots
        rows = np.random.default_rng(s.seed(9)).uniform(-1, 1, (2, ns))
        eng.set_seeded_encryption(True)
        try:
            cts = eng.encrypt_batch(rows)
        finally:
            eng.set_seeded_encryption(False)
        blobs = [c.export_compact() for c in cts]
        for i, b in enumerate(blobs):
            s.raw(f"compact blob {i}", np.frombuffer(b, dtype=np.uint8))
        for i, (c, back) in enumerate(zip(cts, eng.import_compact(blobs))):
            s.operand(c, "seeded encryption")
            s.out(f"expanded {i}", back, c.export())
    run(trios("toy"), orc, scen)


@pytest.mark.parametrize("stride", [1, 2])
def test_wrapped_inputs(trios, orc, stride):
    """wrapped ingest -> compact bytes -> unwrap (the masked drop over the p_0 limb, three merged rotate-and-sums per input), on the
    smallest ring that holds the layout's 16384 logical slots (N = 2^15, at stride 2 N = 2^16: the chain of
    tests/test_wrapped_interleaved_gpu.py).  One wrapped ciphertext of 2 inputs at n_q limbs and one of 66 at 2 limbs, so that t reaches
    65: every a and b offset set and both signs of the 64 step.  The three engines agree on the wrapped bytes and on every unwrapped
    residue; the blobs imported again unwrap to the same residues; every lane decrypts to its expanded row within
    1e-8 * max(1, max|row|), the bound of tests/test_wrapped_inputs_gpu.py.  Of the 30 unwrap keys four are watched as operands (one of
    each fan and sign; a key of this ring is 11 - 22 MB to read back)."""
    def scen(s):
        eng = s.eng
        if not getattr(eng, "_stale_wrapped", False):
            eng.keygen()
            eng.gen_rotation_keys(UNWRAP_KEYS)
            eng._stale_wrapped = True
        for k in (1, -7, 56, -64):
            s.key(1, k)
        S = 3
        n = 64 + S + 1
        sh, embs = _shared(S, s.seed(6)), _embs(S, stride, s.seed(6))
        targets = [eng.n_q] * 2 + [2] * (n - 2)
        if stride == 1:
            ws, x_in, proj = eng.client_ingest_wrapped(**sh, emb=embs[0], targets=targets, want_proj=True)
            x_in, proj = [x_in], [proj]
        else:
            ws, x_in, proj = eng.client_ingest_wrapped_interleaved(**sh, embs=embs, targets=targets, want_proj=True)
        assert [w.wrapped_info()["count"] for w in ws] == [2, n - 2]
        blobs = [w.export_compact() for w in ws]
        for i, (w, b) in enumerate(zip(ws, blobs)):
            s.wrapped(w, f"wrapped {i}")
            s.raw(f"wrapped {i}, compact bytes", np.frombuffer(b, dtype=np.uint8))
            s.raw(f"wrapped {i}, positions", np.array(w.wrapped_info()["positions"], dtype=np.int64))
        outs = eng.unwrap_inputs(ws)
        assert len(outs) == n
        back = eng.unwrap_inputs(eng.import_compact(blobs))
        for v, (o, o2) in enumerate(zip(outs, back)):
            s.out(f"input {v}", o)
            assert o2.info() == o.info() and o2.scale_parts() == o.scale_parts() and np.array_equal(o2.export(), s.arrays[-3]), \
                ("unwrapped after the compact round trip", v)
        got = np.asarray(eng.decrypt_batch(outs, 16384, all_lanes=stride > 1)).reshape(n, stride, 16384)
        s.raw("decrypted, every lane", got)
        for lane in range(stride):
            rows = np.vstack([proj[lane], x_in[lane]])                      # read order: E rows, F rows, tokens
            for v in range(n):
                err = np.max(np.abs(got[v, lane] - _expanded(rows[v])))
                assert err < 1e-8 * max(1.0, np.max(np.abs(rows[v]))), (v, lane, err)
    kw = dict(interleave=stride) if stride > 1 else {}
    run(trios("toy13", tag="wrapped", **_ring(stride), **kw), orc, scen)


def test_interleaved_encode_encrypt_decrypt(trios, orc):
    """the same on an engine with interleave = 2: two samples per ciphertext"""
    def scen(s):
        eng = s.eng
        _with_keys(eng)
        n = 1 << eng.params.log_slots
        rng = np.random.default_rng(s.seed(6))
        z = rng.uniform(-1, 1, (2, 2, n))
        v = rng.uniform(-1, 1, n)
        s.raw("encode, pt_export", eng.pt_export(eng.encode(v), eng.n_q))
        cts = [s.operand(c, "encrypt_interleaved_batch") for c in eng.encrypt_interleaved_batch(z)]
        for i, c in enumerate(cts):
            s.out(f"encrypt_interleaved_batch {i}", c)
        c1 = s.operand(eng.encrypt(v), "encrypt")
        s.out("encrypt", c1)
        d = eng.decrypt_interleaved(cts[0])
        s.raw("decrypt_interleaved", d)
        assert np.max(np.abs(d - z[0])) < 1e-6
        s.raw("decrypt_batch, all lanes", eng.decrypt_batch(cts, all_lanes=True))
        s.raw("decrypt_batch, flooded", eng.decrypt_batch(cts, flood_bits=20))
    run(trios("toy", log_slots=10, interleave=2), orc, scen)


def test_reply_sanitisation(trios, orc):
    """mask, shrink, re-randomise and flood in one fused launch: the engines draw the same randomness, so the replies are equal"""
    def scen(s):
        eng = s.eng
        _with_keys(eng)
        ns = 1 << eng.params.log_slots
        rng = np.random.default_rng(s.seed(12))
        rows = rng.uniform(-1, 1, (2, ns))
        cts = [s.operand(c, "result") for c in eng.encrypt_batch(rows)]
        sq = s.operand(eng.mult(cts[0], eng.encode(rows[1])), "degree-2 result")
        mask = np.zeros(ns)
        mask[:128] = 1.0
        for i, o in enumerate(eng.sanitize(cts + [sq], flood_bits=20, out_ell=2)):
            s.out(f"sanitised {i}", o)
        mask_pt = s.plain(eng.encode(mask), [(eng.n_q, 0.0)], "mask")
        one = eng.sanitize(cts[1], mask=mask_pt, flood_bits=0, out_ell=1)
        s.out("masked, one limb", one)
        d = eng.decrypt(one)
        s.raw("decrypted reply", d)
        assert np.max(np.abs(d[:ns] - rows[1] * mask)) < 1e-3
    run(trios("toy"), orc, scen)


# ------------------------------------------------------------------------------------------------ composites, real keys
BULK_NEED = sorted({sg * k for sg in (1, -1) for k in range(1, 8)} | {8 * sg * k for sg in (1, -1) for k in range(1, 8)} | {64, -64})
TREE_NEED = sorted({128 * k for k in range(1, 9)} | {1536} | {-512 * k for k in range(1, 8)})
COMPOSITE = dict(n_q=4, n_p=2, dnum=2)


def _composite_keys(s):
    """real keys for the composites, generated once per engine; the oracle side gets every rotation key the engine holds, so that it
    takes the same merged steps"""
    eng = s.eng
    if not getattr(eng, "_stale_composite", False):
        eng.keygen()
        eng.gen_rotation_keys(BULK_NEED + TREE_NEED)
        eng._stale_composite = True
    for r in BULK_NEED + TREE_NEED:
        s.key(1, r)
    if s.anchor:
        if not hasattr(eng, "_stale_exported"):
            eng._stale_exported = {r: eng.key_export(1, r) for r in BULK_NEED + TREE_NEED}
        return eng._stale_exported
    return None


def test_unwrap_expanded_bulk(trios, orc):
    """70 rows read together: the fans rot(c, j) and every row as a sliding-window sum over four tap chunks, the first with
    accumulate = 0 into a fresh block of 32 destinations (ew_window_dot_kernel), the rest accumulating in place"""
    def scen(s):
        eng = s.eng
        keys = _composite_keys(s)
        ns, n, ell = 1 << eng.params.log_slots, 70, 4
        c = s.operand(eng.ct_import(_ct(s.orc, eng, s.seed(77), ell)))
        rows = eng.unwrapExpanded(c, n)
        eng.force(rows)
        want = None
        if s.anchor:
            from oracle.residue_eval import RCt
            rev = s.rev(keys)
            enc_of = lambda p: (lambda l, sc: eng.pt_export(p, l, sc))
            masks = []
            for k in range(128):
                m = np.zeros(ns)
                m[k::128] = 1.0
                masks.append(enc_of(eng.encode(m)))
            hi, lo = c.scale_parts()
            want = rev.unwrapExpanded_bulk(RCt(c.export(), 1, LD(hi) + LD(lo)), n, list(range(n)), masks)
        for i in range(n):
            s.out(f"bulk row {i}", rows[i], want[i] if want is not None and i in (0, 1, 31, 32, 63, 64, 69) else None)
    run(trios("toy13", tag="composite", **COMPOSITE), orc, scen)


def test_lazy_rows_out_of_order_and_containers(trios, orc):
    """matmulRE's deferred rows read out of order hold the residues of the eager call; generate_containers of evaluated rows.
    Nothing here is anchored on the CPU oracle: the lazy rows are held against the SAME engine's eager matmulRE, and the
    unwrapExpanded rows and the containers only against the other two engines (as in
    test_deferred_rows_match_eager_and_skip_dead_rows; the oracle's side of these composites is test_unwrap_expanded_bulk's)."""
    def scen(s):
        eng = s.eng
        _composite_keys(s)
        ns = 1 << eng.params.log_slots
        rng = np.random.default_rng(s.seed(4))
        w, b = eng.encode(rng.uniform(-1, 1, ns) / 8), eng.encode(rng.uniform(-1, 1, ns))
        rows = [s.operand(eng.ct_import(_ct(s.orc, eng, s.seed(500 + i), 4))) for i in range(5)]
        eng.set_lazy_rows(False)
        try:
            eager = [o.export() for o in eng.matmulRE(rows, w, b, 16, 128)]
        finally:
            eng.set_lazy_rows(True)
        lazy = eng.matmulRE(rows, w, b, 16, 128)
        for i in (4, 1, 2):                                        # one row alone, then two more; rows 0 and 3 are read last
            s.out(f"lazy row {i}", lazy[i], eager[i])
        for i in (3, 0):
            s.out(f"lazy row {i}", lazy[i], eager[i])
        un = eng.unwrapExpanded(rows[0], 6)
        for i in (5, 0, 3):
            s.out(f"unwrapped row {i}", un[i])
        for k, c in enumerate(eng.generate_containers(rows[:4])):
            s.out(f"container {k}", c)
    run(trios("toy13", tag="composite", **COMPOSITE), orc, scen)


# ------------------------------------------------------------------------------------------------ bootstrapping
def _boot_ready(s):
    eng = s.eng
    if not getattr(eng, "_stale_boot", False):
        eng.keygen()
        eng.gen_relin_key()
        eng.bootstrap_setup(3, 3, 1 << eng.params.log_slots)
        eng._stale_boot = True


def test_chebyshev_and_bootstrap(trios, orc):
    """a small Chebyshev evaluation, one bootstrap and one bootstrap_iter on boot12 with real keys, each anchored on the oracle
    (oracle/residue_boot.py, composed as in tests/test_exact_products_gpu.py and tests/test_bootstrap_iter_gpu.py); the results are
    bootstraps (the bound of those tests: 2e-4 at this ring)"""
    from test_bootstrap_iter_gpu import _iter_oracle
    from test_exact_products_gpu import _boot_oracle
    from oracle.residue_eval import RCt

    def scen(s):
        eng = s.eng
        _boot_ready(s)
        s.key(0)
        n = 1 << eng.params.log_slots
        rev = s.rev({"relin": eng.key_export(0)}) if s.anchor else None
        if s.anchor and not boots:
            boots.append(_boot_oracle(eng))                   # the keys stay the same over both rounds
        x = _ct(s.orc, eng, s.seed(4119), 8)
        sc = float(eng.scaling_factors[eng.n_q - 8])
        c = s.operand(eng.ct_import(x, deg=1, scale=sc))
        coeffs = [0.3, -0.7, 0.11, 0.05, -0.02, 0.4, 0.0, 0.21, -0.13, 0.07, 0.3, -0.2, 0.1]
        s.out("chebyshev 12", eng.eval_chebyshev(c, coeffs, -1.0, 1.0), (lambda: rev.eval_chebyshev(RCt(x, 1, LD(sc)), coeffs, -1.0, 1.0)))
        m = np.random.default_rng(s.seed(3)).uniform(-1, 1, n)
        ct = s.operand(eng.encrypt(m, level=eng.n_q - 3), "bootstrap input")
        o = eng.bootstrap(ct)
        hi, lo = ct.scale_parts()
        r = RCt(ct.export(), ct.info()["deg"], LD(hi) + LD(lo))
        s.out("bootstrap", o, lambda: boots[0].run(r))
        d = eng.decrypt(o)
        s.raw("bootstrap, decrypted", d)
        assert np.max(np.abs(d[:n] - m)) < 2e-4
        o2 = eng.bootstrap_iter(ct, 8)
        s.out("bootstrap_iter", o2, lambda: _iter_oracle(boots[0], r, 8, 0)[0])
        assert np.max(np.abs(eng.decrypt(o2)[:n] - m)) < 2e-4
    boots = []
    run(trios("boot12", tag="boot", log_slots=10), orc, scen)
