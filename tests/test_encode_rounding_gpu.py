"""The encoder's rounding and the decoder's lift pinned at their boundaries against tests/encode_model.py, exactly (no tolerance anywhere).

Channel (encode_model.py): a constant vector (c, ..., c) passes the inverse special FFT without rounding, so its encoding at scale S is the
constant polynomial K = sign(c) * round_half_away(RNE64(|c| S)), and in NTT form every word of limb l is K mod q_l; a ciphertext
(K at every position, 0) decrypts to one double in every slot.  fhelin_pt_export takes S exactly (hi + lo), so a test chooses both c and the
64-bit significand of S: first-rounding ties both ways, carries out of 64 bits, second-rounding ties, double rounding, 1/2 -> 1, products at
and above 2^64, both sides of the host's 9.0e18 switch, negative multiples of 2^64, subnormals and zeros - the census of
tests/test_encode_rounding_host.py holds the generator to at least 4 cases of each.

The device leg (x87_mul_round in encode_round_reduce_kernel) and the host leg (ld_to_i128 + reduce_i128_kernel) run on two contexts: the
content-keyed plaintext cache of one context would hand the second encoder the first one's encoding of the same values.  Both must equal
the model, and therefore each other.  The slots = 1 path (host only, whichever encoder is set) runs one case per category.

Out of the encoder's domain (include/fhelin.h): NaN and infinities are refused by fhelin_encode and fhelin_encrypt_batch, an encoding with
max|v| * S that may reach 2^125 (by the exponents of the two factors) where it is made; the context goes on working."""
import ctypes as C
import time

import numpy as np
import pytest

import encode_model as em
from test_client_randomness_gpu import _import_exact

pytestmark = pytest.mark.gpu

ODD52 = em.ODD52


@pytest.fixture(scope="module")
def ctx(fa):
    """(device-encoder context with keys, host-encoder context, Delta of every level as (ms, es)) on the toy preset, N = 2^12"""
    dev = fa.Engine("toy", seed=41)
    host = fa.Engine("toy", seed=41)
    host.set_host_encode(True)
    dev.keygen()
    deltas = em.delta_chain([int(x) for x in dev.q])
    for lvl in (0, 1, dev.n_q - 1):               # the chain restated in encode_model.py is the engine's, to the last bit
        assert dev.encrypt(np.zeros(4), level=lvl).scale_parts() == em.hi_lo(*deltas[lvl])
    yield dev, host, deltas
    dev.close()
    host.close()


@pytest.fixture(scope="module")
def model(ctx):
    """[(c, ms, es, K, trace)] once for every test"""
    _, _, deltas = ctx
    return [(c, ms, es) + em.encode_int(c, ms, es) for c, ms, es in em.cases([deltas[0], deltas[1], deltas[-1]])]


def _export(eng, pt, ell, ms, es):
    """fhelin_pt_export at the exact scale ms * 2^es"""
    hi, lo = em.hi_lo(ms, es)
    out = np.empty((ell, eng.N), dtype=np.uint64)
    eng._ck(eng.lib.fhelin_pt_export(eng.h, pt.h, ell, hi, lo, out.ctypes.data_as(C.c_void_p), out.size))
    return out


def _residues(eng, K, ell):
    return np.array([K % int(m) for m in eng.moduli[:ell]], dtype=np.uint64)[:, None]


def _ells(eng, es):
    """n_q and 1 limb; the full key basis too for the scales near 2^104 (a 128-bit magnitude reduced modulo the 60-bit special limbs)"""
    return (eng.n_q, 1) + ((eng.n_q + eng.n_p,) if es > 0 else ())


@pytest.mark.parametrize("slots", [0, 8])          # full packing (N/2 slots) and 8 slots
@pytest.mark.parametrize("encoder", ["device", "host"])
def test_constant_channel_equals_the_model(ctx, model, encoder, slots):
    dev, host, _ = ctx
    eng = dev if encoder == "device" else host
    n = slots or 1 << eng.params.log_slots
    bad, checked, t0 = [], 0, time.time()
    for c, ms, es, K, trace in model:
        pt = eng.encode(np.full(n, c), slots=slots)
        for ell in _ells(eng, es):
            got = _export(eng, pt, ell, ms, es)
            checked += 1
            if not np.array_equal(got, np.broadcast_to(_residues(eng, K, ell), got.shape)):
                bad.append((c.hex(), hex(ms), es, ell, sorted(trace), K, [int(x) for x in got[:, 0]]))
    print("%s encoder, %d slots: %d cases, %d exports, %.2f s" % (encoder, n, len(model), checked, time.time() - t0))
    assert not bad, (len(bad), bad[:4])


def test_one_slot_path_equals_the_model(ctx, model):
    """slots = 1 is encoded on the host whichever encoder is set: one case per category and sign through both contexts"""
    dev, host, _ = ctx
    seen, picked = set(), []
    for case in model:
        new = {(k, case[0] < 0) for k in case[4]} - seen
        if new:
            seen |= new
            picked.append(case)
    assert {k for k, _ in seen} == set(em.TRACE_ENCODE)
    for c, ms, es, K, trace in picked:
        for eng in (dev, host):
            pt = eng.encode([c], slots=1)
            for ell in _ells(eng, es):
                got = _export(eng, pt, ell, ms, es)
                assert np.array_equal(got, np.broadcast_to(_residues(eng, K, ell), got.shape)), (c.hex(), hex(ms), es, ell, sorted(trace))


def _few_bit_vector(rng, slots, ms, es):
    """slot values k/4096 whose mean - coefficient 0 of the encoding, exact in fp64: the sums of the inverse FFT's first column are sums of
    few-bit values - makes a first-rounding tie that goes DOWN at the scale ms * 2^es (the tie a `rem >= half` would round up).
    The tie is at coefficient 0 ONLY.  Every other coefficient of a real slot vector is a sum of products with the irrational ksi
    table, an ordinary double that does not tie: a few-bit vector cannot put a tie there, so the ties on all coefficients are what the
    constant channel is for, and this vector shows one inside an encoding that is not constant."""
    for _ in range(4000):
        k = rng.integers(-8192, 8193, slots)
        mean = float(k.sum()) / (4096.0 * slots)
        if mean != 0.0 and "tie1_down" in em.encode_int(mean, ms, es)[1]:
            return k / 4096.0
    raise AssertionError("no tie found")


def test_every_slot_count_device_equals_host(ctx):
    """the special FFT's stage kernel at every size from 2 to N/2 (the t >= size/2 guard, rot[j] % lenq at short lengths): the residues of
    the device encoder equal the host encoder's, on another context"""
    dev, host, deltas = ctx
    rng = np.random.default_rng(7)
    ell = dev.n_q
    big = (deltas[0][0], deltas[0][1] + 52)       # Delta_0 * 2^52: the same significand, and one unit of its last place is an integer
    slots = 2
    while slots <= dev.N // 2:
        vecs = {"uniform": rng.uniform(-1, 1, slots),
                "short": rng.uniform(-1, 1, max(1, slots // 2 - 1)),                       # zero padding up to `slots`
                "fewbit": _few_bit_vector(rng, slots, *big)}                              # a tie inside a vector that is not constant
        if slots >= 128:
            vecs["mask"] = np.where(np.arange(slots) % 128 == 0, 1.0, 0.0)
        for name, v in vecs.items():
            for ms, es in (deltas[0], ODD52, big):
                got = _export(dev, dev.encode(v, slots=slots), ell, ms, es)
                want = _export(host, host.encode(v, slots=slots), ell, ms, es)
                assert np.array_equal(got, want), (slots, name, es)
                assert got.any()
        slots *= 2


class _Like:
    """what _import_exact reads of a ciphertext: degree, slots, exact scale"""

    def __init__(self, slots, ms, es):
        self._inf, self._scale = {"deg": 1, "slots": slots}, em.hi_lo(ms, es)

    def info(self):
        return self._inf

    def scale_parts(self):
        return self._scale


@pytest.mark.parametrize("ell", [1, 2, 4])          # one limb read; two; two of four
def test_decoder_lift_equals_the_model(ctx, ell):
    """(c0, c1) = (K at every NTT position, 0): the phase is the constant K, coefficient 0 decodes to (double)(lift / scale) and the forward
    FFT adds 0 * ksi to it - every slot holds that double.  K at 0, +-1, floor(M/2) and its neighbours, M - 1, and 20 uniform values"""
    dev, _, deltas = ctx
    q = [int(x) for x in dev.q]
    read = q[:min(ell, 2)]
    seen = set()
    for slots in (1 << dev.params.log_slots, 8):
        for ms, es in (deltas[dev.n_q - ell], ODD52):
            for K in em.decode_cases(read, ell):
                limbs = np.zeros((2, ell, dev.N), dtype=np.uint64)
                limbs[0] = _residues(dev, K, ell)
                got = dev.decrypt(_import_exact(dev, limbs, _Like(slots, ms, es)))
                want, trace = em.decode_double(K, read, ms, es)
                seen |= trace
                assert got.shape == (slots,)
                assert np.array_equal(got, np.full(slots, want)), (slots, es, K, sorted(trace), got[:2], want)
    assert seen == set(em.TRACE_DECODE)


# ----------------------------------------------------------------------------------------------------------------- out of the domain
def _code(fa, fn):
    with pytest.raises(fa.FhelinError) as ei:
        fn()
    return ei.value.code


def _still_works(dev, host, deltas, ref, before, tag):
    """after refusals: the earlier vector exports its earlier bytes (within one context the plaintext cache may serve that from the
    encoding made before, so it proves little alone); a vector never encoded before equals the host encoder's residues on the other
    context; a constant never encoded before equals the model"""
    assert np.array_equal(dev.pt_export(dev.encode(ref), dev.n_q), before)
    fresh = ref.copy()
    fresh[5] = 0.3141592653589793 + tag
    ms, es = deltas[1]
    assert np.array_equal(_export(dev, dev.encode(fresh), dev.n_q, ms, es), _export(host, host.encode(fresh), dev.n_q, ms, es))
    c = 0.7071067811865476 + tag
    got = _export(dev, dev.encode(np.full(ref.size, c)), dev.n_q, ms, es)
    assert np.array_equal(got, np.broadcast_to(_residues(dev, em.encode_int(c, ms, es)[0], dev.n_q), got.shape))


def test_non_finite_values_are_refused_and_the_context_goes_on(fa, ctx):
    dev, host, deltas = ctx
    n = 1 << dev.params.log_slots
    ref = np.linspace(-1.0, 1.0, n)
    before = dev.pt_export(dev.encode(ref), dev.n_q)
    for eng in (dev, host):
        for bad in (float("nan"), float("inf"), float("-inf")):
            for pos in (0, n // 2, n - 1):
                v = ref.copy()
                v[pos] = bad
                assert _code(fa, lambda: eng.encode(v)) == 1, (bad, pos)
    rows = np.tile(ref, (3, 1))
    source = dev.level_plan_tell()[1]
    for bad in (float("nan"), float("inf"), float("-inf")):
        for r, pos in ((0, 0), (1, n // 2), (2, n - 1)):
            a = rows.copy()
            a[r, pos] = bad
            assert _code(fa, lambda: dev.encrypt_batch(a, level=dev.n_q - 2)) == 1, (bad, r, pos)
    assert dev.level_plan_tell()[1] == source                           # a refused call is no source of the level plan
    _still_works(dev, host, deltas, ref, before, 0.0)
    cts = dev.encrypt_batch(rows, level=dev.n_q - 2)
    assert len(cts) == 3 and all(ct.info()["ell"] == 2 for ct in cts)               # the batch path still encrypts


def test_over_range_encodings_are_refused_where_they_are_made(fa, ctx):
    """what may reach 2^125 is refused: floor(log2 max|v|) + floor(log2 scale) > 123.  Delta_0 = q_L lies just below 2^52 (2^73 * Delta_0 is
    2^125 (1 - 4.9e-11)), so 2^73 is out and 2^72 is in"""
    dev, host, deltas = ctx
    ms, es = deltas[0]
    assert 2 ** 51 <= em.scale_of(ms, es) < 2 ** 52
    assert not em.in_domain(2.0 ** 73, ms, es) and em.in_domain(2.0 ** 72, ms, es) and em.in_domain(-(2.0 ** 73 - 2.0 ** 20), ms, es)
    n = 1 << dev.params.log_slots
    ref = np.linspace(-1.0, 1.0, n)
    before = dev.pt_export(dev.encode(ref), dev.n_q)
    for eng in (dev, host):
        for sign in (1.0, -1.0):
            v = ref.copy()
            v[n // 3] = sign * 2.0 ** 73
            pt = eng.encode(v)                                          # the values are fine for a smaller scale: nothing is made yet
            assert _code(fa, lambda: eng.pt_export(pt, eng.n_q)) == 1                     # at Delta_0
            assert _code(fa, lambda: _export(eng, pt, eng.n_q, ms, es)) == 1
            one = (1 << 63, -63)
            _export(eng, pt, 2, *one)                                   # the same plaintext still encodes at scale 1
            big = eng.encode(np.full(n, sign * 2.0 ** 73))
            K, _ = em.encode_int(sign * 2.0 ** 73, *one)
            got = _export(eng, big, eng.n_q, *one)
            assert np.array_equal(got, np.broadcast_to(_residues(eng, K, eng.n_q), got.shape))
            ok = eng.encode(np.full(n, sign * 2.0 ** 72))
            K, _ = em.encode_int(sign * 2.0 ** 72, ms, es)
            got = eng.pt_export(ok, eng.n_q)                            # 2^72 at Delta_0: inside
            assert np.array_equal(got, np.broadcast_to(_residues(eng, K, eng.n_q), got.shape))
    v = ref.copy()
    v[-1] = 2.0 ** 73
    source = dev.level_plan_tell()[1]
    assert _code(fa, lambda: dev.encrypt(dev.encode(v))) == 1
    assert _code(fa, lambda: dev.encrypt_batch(np.stack([ref, v]), level=0)) == 1
    assert dev.level_plan_tell()[1] == source                           # a refused call is no source of the level plan
    v[-1] = 2.0 ** 72
    assert len(dev.encrypt_batch(np.stack([ref, v]), level=0)) == 2 and dev.level_plan_tell()[1] == source + 2
    _still_works(dev, host, deltas, ref, before, 1.0)
