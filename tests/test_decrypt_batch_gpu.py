"""Batched decryption (include/fhelin.h "Batched decryption") on the GPU: the device decoder held to the model and to the host decoder.

Every double is compared as a bit pattern (.view(np.uint64)); there is no tolerance anywhere except the flood's statistical bound.

  1. the constant channel of tests/encode_model.py - (c0, c1) = (K at every NTT position, 0) decodes to one double in every slot - for every
     case of tests/decode_model.py (lift ties both ways, carries, inexact divisions, ties and double rounding in the conversion to double,
     both signs, the boundaries of the centred lift), 32 ciphertexts to a call: decode_lift_kernel against the model;
  2. general data - fresh encryptions at 1, 2 and n_q limbs, an unrescaled product, a rotated ciphertext, mixed in one call - at every
     slot count at which the forward FFT takes another path: decrypt_batch(cts)[b] == decrypt(cts[b]);
  3. slot lists, interleaved lanes, a wrapped input;  4. flooding and the sampler's stream accounting;  5. the device-decode knob;
  6. every refusal;  7. one case at the headline ring N = 2^16.
All of them need fhelin_decrypt_batch, which the library did not have before."""
import numpy as np
import pytest

import decode_model as dm
import encode_model as em

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_KEY = 1, 5
WRAP_RING = dict(log_n=15, n_q=5, n_p=2, dnum=3, log_slots=14, hamming=64)   # the smallest ring with the 16384 slots of the wrapped layout


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _code(fa, fn, *a, **kw):
    with pytest.raises(fa.FhelinError) as ei:
        fn(*a, **kw)
    return ei.value.code


@pytest.fixture(scope="module")
def eng(fa):
    e = fa.Engine("toy", seed=41)
    e.keygen()
    e.gen_rotation_keys([1])
    yield e
    e.close()


@pytest.fixture(scope="module")
def model(eng):
    """{limbs read: [(K, ms, es, the model's double)]} once for every test; the chain restated in encode_model.py is the engine's"""
    q = [int(x) for x in eng.q]
    deltas = em.delta_chain(q)
    for lvl in (0, eng.n_q - 2, eng.n_q - 1):
        assert eng.encrypt(np.zeros(4), level=lvl).scale_parts() == em.hi_lo(*deltas[lvl])
    by_limbs = {1: [], 2: []}
    for read, K, ms, es in dm.cases(q, deltas):
        by_limbs[len(read)].append((K, ms, es, dm.case_trace(K, read, ms, es)[0]))
    return by_limbs


def _import_constant(e, K, ell, slots, ms, es):
    """(K at every NTT position, 0) over ell limbs at the exact scale ms * 2^es"""
    limbs = np.zeros((2, ell, e.N), dtype=np.uint64)
    limbs[0] = np.array([K % int(m) for m in e.moduli[:ell]], dtype=np.uint64)[:, None]
    hi, lo = em.hi_lo(ms, es)
    buf = e.upload(limbs)
    try:
        ct = e.ct_import_device(buf.ptr.value, 2, ell, 1, hi, lo, slots)
        e.sync()
    finally:
        buf.free()
    return ct


# ------------------------------------------------------------------------------------------------ 1. constant channel against the model
@pytest.mark.parametrize("slots", [8, 0])            # 8 slots and full packing (N/2)
@pytest.mark.parametrize("ell", [1, 2, 4])           # one limb read; two; two of four
def test_constant_channel_equals_the_model(eng, model, ell, slots):
    n = slots or eng.N // 2
    cases = model[min(ell, 2)]
    bad = []
    for lo in range(0, len(cases), 32):
        chunk = cases[lo:lo + 32]
        cts = [_import_constant(eng, K, ell, n, ms, es) for K, ms, es, _ in chunk]
        got = eng.decrypt_batch(cts)
        assert got.shape == (len(chunk), n)
        for (K, ms, es, want), row in zip(chunk, got):
            if not np.array_equal(_bits(row), _bits(np.full(n, want))):
                bad.append((K, hex(ms), es, want.hex(), row[:2]))
    print("ell %d, %d slots: %d cases" % (ell, n, len(cases)))
    assert not bad, (len(bad), bad[:4])


# ------------------------------------------------------------------------------- 2. device decoder == host decoder on general data
@pytest.mark.parametrize("slots", [1, 2, 8, 256, 512, 1024, 2048])   # no stage; one; a short tile; exactly one LDS tile (512); the first
def test_batch_equals_single_on_general_data(eng, slots):            # global stage (1024); full packing, gap = 1 (2048)
    rng = np.random.default_rng(1000 + slots)
    z = [rng.uniform(-1, 1, slots) for _ in range(5)]
    w = rng.uniform(-1, 1, slots)
    cts = [eng.encrypt(z[0], level=eng.n_q - 1, slots=slots),                                 # one limb
           eng.encrypt(z[1], level=eng.n_q - 2, slots=slots),                                 # two
           eng.encrypt(z[2], level=0, slots=slots),                                           # n_q: two of six read
           eng.mult(eng.encrypt(z[3], level=eng.n_q - 3, slots=slots), eng.encode(w, slots=slots)),   # unrescaled product, 3 limbs
           eng.rotate(eng.encrypt(z[4], level=eng.n_q - 4, slots=slots), 1)]
    assert [c.info()["ell"] for c in cts] == [1, 2, eng.n_q, 3, 4] and cts[3].info()["deg"] == 2
    single = [eng.decrypt(c) for c in cts]
    assert all(s.shape == (slots,) for s in single)
    assert np.abs(single[1] - z[1]).max() < 1e-6 and np.abs(single[3] - z[3] * w).max() < 1e-6     # the reference decodes the data
    for pick in ([0, 1, 2, 3, 4], [3, 0], [0], [1], [2], [3], [4]):                            # batches of 5, 2 and 1
        got = eng.decrypt_batch([cts[i] for i in pick])
        assert got.shape == (len(pick), slots)
        for row, i in zip(got, pick):
            assert np.array_equal(_bits(row), _bits(single[i])), (slots, pick, i)
    assert cts[3].info()["deg"] == 2 and _same(eng.decrypt(cts[3]), single[3])                # the inputs are untouched


# ------------------------------------------------------------------------------------------------------------------- 3. idx and lanes
def test_slot_lists(eng):
    rng = np.random.default_rng(5)
    cts = [eng.encrypt(rng.uniform(-1, 1, 256), level=eng.n_q - k, slots=256) for k in (1, 2, 3)]
    full = eng.decrypt_batch(cts)
    idx = [200, 3, 255, 3, 0, 17]                       # unsorted, one entry repeated
    got = eng.decrypt_batch(cts, idx=idx)
    assert got.shape == (3, len(idx)) and _same(got, full[:, idx])
    assert _same(eng.decrypt_batch(cts, slots=256, idx=[9]), full[:, [9]])


def test_interleaved_lanes(fa):
    e = fa.Engine("toy", seed=43, interleave=2, log_slots=10)
    try:
        e.keygen()
        rng = np.random.default_rng(6)
        n = 1 << e.params.log_slots
        cts = e.encrypt_interleaved_batch(rng.uniform(-1, 1, (3, 2, n)), level=e.n_q - 2)
        lanes = e.decrypt_batch(cts, all_lanes=True)
        assert lanes.shape == (3, 2, n)
        lane0 = e.decrypt_batch(cts)
        for b, ct in enumerate(cts):
            assert _same(lanes[b], e.decrypt_interleaved(ct)) and _same(lane0[b], e.decrypt(ct))
        idx = [5, 1, n - 1, 5]
        assert _same(e.decrypt_batch(cts, idx=idx, all_lanes=True), lanes[:, :, idx])
    finally:
        e.close()


def test_wrapped_input(fa):
    e = fa.Engine("toy13", seed=44, **WRAP_RING)
    try:
        e.keygen()
        rng = np.random.default_rng(7)
        S = 2
        ws = e.client_ingest_wrapped(cls=rng.uniform(-1, 1, 128), pos=rng.uniform(-1, 1, (S, 128)), E_w=rng.uniform(-0.1, 0.1, (32, S + 1)),
                                     E_b=rng.uniform(-0.1, 0.1, 32), F_w=rng.uniform(-0.1, 0.1, (32, S + 1)), F_b=rng.uniform(-0.1, 0.1, 32),
                                     emb=rng.uniform(-1, 1, (S, 128)), targets=[2] * 32 + [e.n_q] * (32 + S + 1))
        assert len(ws) == 2 and sorted(w.info()["ell"] for w in ws) == [3, e.n_q + 1]
        plain = e.encrypt(rng.uniform(-1, 1, 16384), level=e.n_q - 1)
        got = e.decrypt_batch(ws + [plain], slots=16384)               # wrapped inputs of two limb counts and an ordinary one-limb one
        for row, ct in zip(got, ws + [plain]):
            assert _same(row, e.decrypt(ct, 16384))
        assert np.abs(got[0]).max() > 0.01
    finally:
        e.close()


# ------------------------------------------------------------------------------------------------------------------------ 4. flooding
def test_flooding_and_the_sampler_streams(fa):
    a, b = fa.Engine("toy", seed=45), fa.Engine("toy", seed=45)
    try:
        z = np.random.default_rng(8).uniform(-1, 1, 8)
        cts = []
        for e in (a, b):
            e.keygen()
            cts.append(e.encrypt(z, level=e.n_q - 2, slots=8))
        assert np.array_equal(cts[0].export(), cts[1].export())
        # a batch of one IS decrypt_flooded: the same key draw, the same stream, the same counter afterwards
        got = a.decrypt_batch([cts[0]], flood_bits=24)
        want = b.decrypt_flooded(cts[1], 24)
        assert _same(got[0], want)
        (ka, ca), (kb, cb) = a.debug_sampler_peek(2), b.debug_sampler_peek(2)
        assert ca == cb and np.array_equal(ka, kb)
        # a batch of three: ONE key draw, the flood of ciphertext b on stream (C << 32) + b, C += 2
        plain = a.decrypt(cts[0])
        keys_before, c0 = a.debug_sampler_peek(2)
        three = a.decrypt_batch([cts[0]] * 3, flood_bits=24)
        keys_after, c1 = a.debug_sampler_peek(1)
        assert c1 == c0 + 2 and np.array_equal(keys_after[0], keys_before[1])      # exactly one key was drawn
        hi, lo = cts[0].scale_parts()
        # a slot of an n-slot decoding sums n uniform coefficient pairs against unit roots, standard deviation
        # sqrt(n) * (2^B / sqrt 3) / Delta; 6 of them bound 24 samples (the bound tests/test_sanitize_gpu.py uses)
        sd = np.sqrt(8) * np.sqrt(4.0 ** 24 / 3) / (hi + lo)
        diff = three - plain
        print("flooded slot error: max %.3e, predicted sd %.3e" % (np.abs(diff).max(), sd))
        for i in range(3):
            assert not np.array_equal(_bits(three[i]), _bits(plain))
            assert np.abs(diff[i]).max() < 6 * sd
            for j in range(i):
                assert not np.array_equal(_bits(three[i]), _bits(three[j]))
        # b makes the same call: deterministic in the seed and the call sequence
        assert _same(b.decrypt_batch([cts[1]] * 3, flood_bits=24), three)
        # a refused call draws nothing and leaves the counter where it found it
        one_limb = a.encrypt(z, level=a.n_q - 1, slots=8)
        before = a.debug_sampler_peek(1)
        assert _code(fa, a.decrypt_batch, [cts[0]], flood_bits=63) == ERR_ARG
        assert _code(fa, a.decrypt_batch, [cts[0], one_limb], flood_bits=54) == ERR_ARG       # too wide for the one limb read (55 bits)
        after = a.debug_sampler_peek(1)
        assert before[1] == after[1] and np.array_equal(before[0], after[0])
        assert _same(a.decrypt_batch([cts[0]])[0], plain)
    finally:
        a.close()
        b.close()


# ------------------------------------------------------------------------------------------------------------------------ 5. the knob
def test_device_decode_knob(fa, eng):
    rng = np.random.default_rng(9)
    cts = [eng.encrypt(rng.uniform(-1, 1, 1024), level=eng.n_q - k, slots=1024) for k in (1, 2, 4)]
    cts.append(eng.mult(cts[2], eng.encode(rng.uniform(-1, 1, 1024), slots=1024)))
    off = [(eng.decrypt(c), eng.decrypt_flooded(c, 0), eng.decrypt_interleaved(c)) for c in cts]
    eng.set_device_decode(True)
    try:
        on = [(eng.decrypt(c), eng.decrypt_flooded(c, 0), eng.decrypt_interleaved(c)) for c in cts]
    finally:
        eng.set_device_decode(False)
    for x, y in zip(off, on):
        assert all(_same(p, q) for p, q in zip(x, y))
    il = fa.Engine("toy", seed=46, interleave=2, log_slots=10)
    try:
        il.keygen()
        ct = il.encrypt_interleaved_batch(rng.uniform(-1, 1, (1, 2, 1024)), level=il.n_q - 2)[0]
        off = (il.decrypt(ct), il.decrypt_interleaved(ct))
        il.set_device_decode(True)
        assert _same(il.decrypt(ct), off[0]) and _same(il.decrypt_interleaved(ct), off[1])
    finally:
        il.close()


# -------------------------------------------------------------------------------------------------------------------------- 6. errors
def test_refusals_and_the_context_goes_on(fa, eng, tmp_path):
    import ctypes as C
    rng = np.random.default_rng(10)
    z = rng.uniform(-1, 1, 64)
    ct = eng.encrypt(z, level=eng.n_q - 2, slots=64)
    other = eng.encrypt(z[:32], level=eng.n_q - 2, slots=32)
    want = eng.decrypt(ct)
    lib, f = eng.lib, eng.lib.fhelin_decrypt_batch
    out = np.full((2, 64), 7.0)
    op = out.ctypes.data_as(C.POINTER(C.c_double))
    arr = (C.c_void_p * 2)(ct.h, ct.h)
    assert f(eng.h, None, 1, 0, 0, None, 0, op, 0) == ERR_ARG                         # a null array
    assert f(eng.h, (C.c_void_p * 2)(ct.h, None), 2, 0, 0, None, 0, op, 0) == ERR_ARG  # a null entry
    assert f(eng.h, arr, 2, 0, 0, None, 0, None, 0) == ERR_ARG                        # a null out
    assert f(eng.h, arr, -1, 0, 0, None, 0, op, 0) == ERR_ARG                         # n < 0
    assert f(eng.h, None, 0, 0, 0, None, 0, None, 0) == 0                             # n = 0: fine, touches nothing
    assert np.all(out == 7.0)
    assert _code(fa, eng.decrypt_batch, [ct], idx=[64]) == ERR_ARG                    # idx out of range
    assert _code(fa, eng.decrypt_batch, [ct], idx=[-1]) == ERR_ARG
    assert f(eng.h, arr, 2, 0, 0, (C.c_int32 * 1)(0), 0, op, 0) == ERR_ARG            # n_idx <= 0 with idx given
    assert _code(fa, eng.decrypt_batch, [ct, other]) == ERR_ARG                       # disagreeing slot counts
    assert _code(fa, eng.decrypt_batch, [ct], flood_bits=-1) == ERR_ARG
    assert _code(fa, eng.decrypt_batch, [ct], flood_bits=63) == ERR_ARG
    assert _code(fa, eng.decrypt_batch, [ct], slots=48) == ERR_ARG                    # not a power of two
    assert eng.decrypt_batch([]).shape[0] == 0
    path = str(tmp_path / "batch.evk")
    eng.save_eval_keys(path)
    sv = fa.Engine.from_eval_keys(path, seed=123)
    try:
        inf = ct.info()
        there = sv.ct_import(ct.export(), deg=inf["deg"], scale=inf["scale"], slots=inf["slots"])
        assert _code(fa, sv.decrypt_batch, [there]) == ERR_KEY                        # an evaluation context holds no secret
    finally:
        sv.close()
    got = eng.decrypt_batch([ct, other], slots=64)                                    # the context still decrypts; explicit slots may differ
    assert _same(got[0], want) and _same(got[1], eng.decrypt(other, 64))


# -------------------------------------------------------------------------------------------------- 7. one case at the headline ring
def test_headline_ring_batch_equals_single(fa):
    for n_q in (1, 2):                                  # the shortest chain the preset accepts (one limb read), and two limbs read
        e = fa.Engine("bench", seed=47, n_q=n_q)
        try:
            e.keygen()
            rng = np.random.default_rng(11)
            for slots in (16384, 32768):
                cts = [e.encrypt(rng.uniform(-1, 1, slots), level=0, slots=slots) for _ in range(3)]
                got = e.decrypt_batch(cts)
                assert got.shape == (3, slots)
                for row, ct in zip(got, cts):
                    assert _same(row, e.decrypt(ct)), (n_q, slots)
        finally:
            e.close()
