"""tests/encode_model.py held against real x87 arithmetic, and a census of its case generator (no device).

The model states the encoder's rounding and the decoder's lift in Python int / Fraction; tests/test_encode_rounding_gpu.py compares the
kernels and the host code with it, exactly.  Here, where numpy.longdouble is the 80-bit x87 format, every generated case must give the
same integer / double when the definition is carried out in numpy.longdouble: `(long double)c * S` then round half away; the centred lift as
hi * 2^64 + lo, divided by S, converted to double.  The census is a condition: the generator must reach every edge it names at least 4 times
(ties and carries with both signs), so that an edit of the generator cannot quietly take the hard cases out of the GPU file.  Non-finite
slot values are refused by fhelin_encode without a device."""
from fractions import Fraction

import numpy as np
import pytest

import encode_model as em

LD = np.longdouble
X87 = np.finfo(LD).nmant == 63
needs_x87 = pytest.mark.skipif(not X87, reason="numpy.longdouble is not the x87 80-bit format on this machine")


@pytest.fixture(scope="module")
def toy(fa):
    eng = fa.Engine("toy", device=-1)
    q = [int(x) for x in eng.q]
    sf = np.array(eng.scaling_factors)
    eng.close()
    return q, sf, em.delta_chain(q)


@pytest.fixture(scope="module")
def case_list(toy):
    _, _, deltas = toy
    return em.cases([deltas[0], deltas[1], deltas[-1]])


def _ld_u64(x):
    """an integer below 2^64 as a long double, exactly (never through a double)"""
    assert 0 <= x < 1 << 64
    return LD(x >> 32) * LD(4294967296.0) + LD(x & 0xFFFFFFFF)


def _ld_scale(ms, es):
    hi, lo = em.hi_lo(ms, es)
    s = LD(hi) + LD(lo)
    assert _ld_int(np.ldexp(s, -es)) == ms
    return s


def _ld_int(y):
    """a non-negative integral long double below 2^128 as a Python int, exactly"""
    two64 = LD(18446744073709551616.0)
    h = np.floor(y / two64)
    l = y - h * two64

    def small(v):                                            # below 2^64: two 32-bit halves, each exact as a double
        a = np.floor(v / LD(4294967296.0))
        return int(float(a)) * 4294967296 + int(float(v - a * LD(4294967296.0)))

    return small(h) * (1 << 64) + small(l)


def _ld_encode(c, s):
    """sign(c) * llroundl(|c| * s) in long double arithmetic"""
    y = abs(LD(c)) * s
    fl = np.floor(y)
    r = _ld_int(fl) + (1 if y - fl >= LD(0.5) else 0)
    return -r if np.signbit(c) else r


def _ld_decode(K, moduli_read, s):
    M = 1
    for q in moduli_read:
        M *= q
    v = em.centred(K, M)
    mag = _ld_u64(abs(v) >> 64) * LD(18446744073709551616.0) + _ld_u64(abs(v) & ((1 << 64) - 1))
    d = float(np.float64(mag / s))
    return -d if v < 0 else d


def test_delta_chain_is_the_engines(toy):
    q, sf, deltas = toy
    assert deltas[0] == em.scale_parts(q[-1])
    for k in range(len(q)):
        assert float(em.round_sig(em.scale_of(*deltas[k]), 53)[0]) == sf[k], k


@needs_x87
def test_encoder_model_equals_x87(case_list):
    assert len(case_list) > 1000
    bad = []
    for c, ms, es in case_list:
        assert em.in_domain(c, ms, es)
        K, trace = em.encode_int(c, ms, es)
        got = _ld_encode(c, _ld_scale(ms, es))
        if got != K:
            bad.append((c.hex(), hex(ms), es, K, got, sorted(trace)))
    assert not bad, bad[:5]


@needs_x87
def test_decoder_model_equals_x87(toy):
    q, _, deltas = toy
    odd = em.ODD52
    n = 0
    for ell in (1, 2, 4):
        read = q[:min(ell, 2)]
        for ms, es in (deltas[len(q) - ell], odd):
            s = _ld_scale(ms, es)
            for K in em.decode_cases(read, ell):
                want, _ = em.decode_double(K, read, ms, es)
                got = _ld_decode(K, read, s)
                assert got == want and np.signbit(got) == np.signbit(want), (ell, K, got, want)
                n += 1
    assert n == 3 * 2 * 27


def test_census_of_the_generated_cases(toy, case_list):
    """every edge at least 4 times; ties and carries with both signs"""
    q, _, deltas = toy
    cnt = em.census(case_list)
    print("cases:", len(case_list), {k: tuple(v) for k, v in cnt.items()})
    for k in em.TRACE_ENCODE:
        assert sum(cnt[k]) >= 4, (k, cnt[k])
    for k in em.SIGNED:
        assert min(cnt[k]) >= 1, (k, cnt[k])
    dec = {k: set() for k in em.TRACE_DECODE}                  # distinct (modulus, scale, phase): what the GPU file really decodes
    for ell in (1, 2, 4):
        read = q[:min(ell, 2)]
        for scale in (deltas[len(q) - ell], em.ODD52):
            for K in em.decode_cases(read, ell):
                M = read[0] * (read[1] if len(read) > 1 else 1)
                for k in em.decode_double(K, read, *scale)[1]:
                    dec[k].add((M, scale, K % M))
    for k in em.TRACE_DECODE:
        assert len(dec[k]) >= 4, (k, sorted(dec[k]))


def test_hand_worked_cases():
    """a few cases small enough to check by hand, so that the model is pinned where numpy.longdouble is not x87 too"""
    one = (1 << 63, -63)                                       # scale 1
    assert em.encode_int(2.5, *one) == (3, {"tie2"})
    assert em.encode_int(-2.5, *one) == (-3, {"tie2"})
    assert em.encode_int(0.49999999999999994, *one) == (0, {"below_half"})
    assert em.encode_int(0.5, *one) == (1, {"tie2", "half_to_one"})
    assert em.encode_int(-0.0, *one) == (0, {"zero"})
    odd = ((1 << 63) | 1, -63)                                 # 1 + 2^-63: 1.5 * scale = 1.5 + 1.5 * 2^-63 needs 65 bits, the tie goes to even
    K, tr = em.encode_int(1.5, *odd)
    assert K == 2 and tr == {"tie1_up"}                         # 3 * (2^63 + 1) = ...11 | 1 -> odd quotient, up
    K, tr = em.encode_int(-2.0 ** 64, (1 << 63), -63)
    assert K == -(1 << 64) and tr == {"ge_2^64", "host_big", "host_lo_zero"}
    mv, ms = em.carry_pairs(__import__("random").Random(1), 1)[0]
    K, tr = em.encode_int(float(mv) * 2.0 ** -52, ms, -64)     # product just below 2^116 * 2^-116 = 1
    assert K == 1 and "carry" in tr
    assert em.decode_double(7, [17], 1 << 63, -63)[0] == 7.0 and em.decode_double(9, [17], 1 << 63, -63) == (-8.0, {"above_half"})
    assert em.decode_double(8, [17], 1 << 63, -63) == (8.0, {"at_half"}) and em.decode_double(16, [17], 1 << 63, -62) == (-0.5, {"max"})
    assert em.hi_lo((1 << 63) | 1, -63) == (1.0, 2.0 ** -63)
    assert Fraction(em._step(1.0, 1)) - 1 == Fraction(1, 1 << 52)


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), float("-inf")])
def test_encode_refuses_non_finite_values_without_a_device(fa, bad):
    eng = fa.Engine("toy", device=-1)
    try:
        n = 1 << eng.params.log_slots
        for pos in (0, n // 2, n - 1):
            v = np.linspace(-1.0, 1.0, n)
            v[pos] = bad
            with pytest.raises(fa.FhelinError) as ei:
                eng.encode(v)
            assert ei.value.code == 1, (pos, ei.value)
        eng.encode(np.linspace(-1.0, 1.0, n))                   # the context goes on accepting finite values
        v = np.linspace(-1.0, 1.0, n + 4)
        v[n + 1] = bad                                          # past the slots: never part of the plaintext
        eng.encode(v)
    finally:
        eng.close()
