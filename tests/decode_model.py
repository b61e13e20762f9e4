"""The decoder's number conversion with the edges a case touches, on top of tests/encode_model.py (imported unchanged).

decode_trace(v, ms, es) is encode_model.decode_double's value for the centred phase v,
    sign(v) * RNE53( RNE64( RNE64(|v|) / S ) ),   S = ms * 2^es,
plus which roundings were exact, inexact or ties.  csrc/decode_lift.h (host build: tests/test_decode_lift_host.py; device:
tests/test_decrypt_batch_gpu.py) and the x87 long double code of Client::decrypt_physical both promise exactly this double.

cases() is the seeded generator the two tests share: the toy chain's (q0) and (q0, q1), three scales each - the Delta of the level that
has that many limbs, the odd long-double scale ODD52 and a power of two - and phases built for every edge; census() counts them."""
from fractions import Fraction
import random

import encode_model as em

TRACE_LIFT = ("lift_inexact", "lift_tie_down", "lift_tie_up")       # two limbs only: one limb's magnitude is below 2^55
TRACE_STEPS = TRACE_LIFT + ("div_inexact", "dbl_tie_down", "dbl_tie_up", "double_rounding", "negative")
TRACE_ALL = TRACE_STEPS + em.TRACE_DECODE                            # + at_half, above_half, max, zero (decode_double's own)
POW2 = (1 << 63, -11)                                                # 2^52 as (ms, es)


def decode_trace(v, ms, es):
    """(the double every slot holds for the centred phase v at scale ms * 2^es, the edges of TRACE_STEPS it touches)"""
    trace = set()
    if v == 0:
        return 0.0, trace
    if v < 0:
        trace.add("negative")
    s = em.scale_of(ms, es)
    mag, how, _ = em.round_sig(abs(v), 64)
    if how != "exact":
        trace.add("lift_inexact")
    if how in ("tie_down", "tie_up"):
        trace.add("lift_" + how)
    quo, how, _ = em.round_sig(mag / s, 64)
    if how != "exact":
        trace.add("div_inexact")
    assert how not in ("tie_down", "tie_up"), "a quotient of two 64-bit significands is never a midpoint"
    d, how, _ = em.round_sig(quo, 53)
    if how in ("tie_down", "tie_up"):
        trace.add("dbl_" + how)
    if d != em.round_sig(Fraction(abs(v)) / s, 53)[0]:
        trace.add("double_rounding")
    d = float(d)
    return (-d if v < 0 else d), trace


def case_trace(K, moduli_read, ms, es):
    """(double, edges of TRACE_ALL) of the phase K read on moduli_read: decode_double and decode_trace, which must agree"""
    want, own = em.decode_double(K, moduli_read, ms, es)
    M = 1
    for q in moduli_read:
        M *= int(q)
    got, steps = decode_trace(em.centred(K, M), ms, es)
    assert got.hex() == want.hex()
    return want, own | steps


def _sig64(x):
    """a positive integer shifted to a 64-bit significand"""
    n = x.bit_length()
    return x << (64 - n) if n <= 64 else x >> (n - 64)


def cases(q, deltas, seed=20250611):
    """[(moduli_read, K, ms, es)] with K in [0, M); q the chain, deltas = encode_model.delta_chain(q).  Deterministic."""
    rng = random.Random(seed)
    q = [int(x) for x in q]
    n_q = len(q)
    out = []
    for read in ((q[0],), (q[0], q[1])):
        M = 1
        for m in read:
            M *= m
        half = M // 2
        for ms, es in (deltas[n_q - len(read)], em.ODD52, POW2):
            s = em.scale_of(ms, es)

            def both(mag):
                if 0 < mag <= half:
                    out.append((read, mag, ms, es))
                    out.append((read, M - mag, ms, es))

            for K in em.decode_cases(read, rng.randrange(1 << 30)):
                out.append((read, K % M, ms, es))
            for _ in range(12):                               # small phases: what a decryption of ordinary data holds
                both(rng.randrange(1, 1 << rng.randrange(2, 54)))
            if len(read) == 2:
                for k in (1, 2, 11, 12, 30, 41, 42):          # first-rounding ties both ways, and their neighbours
                    for parity in (0, 1):
                        m = (rng.getrandbits(64) | (1 << 63)) & ~1 | parity
                        tie = (m << k) | (1 << (k - 1))
                        both(tie)
                        both(tie + 1)
                        both(tie - 1)
                for _ in range(12):                           # carries out of 64 bits: 64 ones, then at least one half
                    k = rng.randrange(1, 43)
                    both((((1 << 64) - 1) << k) | (1 << (k - 1)) | rng.getrandbits(k - 1))
            # the 64-bit quotient ends in 0x400: the conversion to double ties.  At the power-of-two scale the quotient's significand is
            # the (rounded) magnitude's; at the others the magnitude is built from the quotient wanted, |v| = round(quo * S), which the
            # division rounds back onto quo (a step of |v| moves the quotient by about one unit in its last place once |v| >= 2^63)
            for _ in range(40):
                sig = (rng.getrandbits(64) | (1 << 63)) >> 12 << 12 | 0x400 | (rng.getrandbits(1) << 11)
                if len(read) == 1:
                    both(sig >> 10)                           # 54 bits, odd: the one-limb magnitudes whose significand ends in 0x400
                    continue
                if (ms, es) == POW2:
                    both(sig << rng.randrange(0, 42))
                else:
                    x = Fraction(sig) * s
                    while x >= 1 << 64:
                        x /= 2
                    while x < 1 << 63:
                        x *= 2
                    both(em.half_away(x))
    return out


def census(case_list):
    """{edge: count} over TRACE_ALL, and {edge: count} of the lift edges among the one-limb cases (must stay empty)"""
    cnt = {k: 0 for k in TRACE_ALL}
    one_limb_lift = 0
    for read, K, ms, es in case_list:
        tr = case_trace(K, read, ms, es)[1]
        for k in tr:
            cnt[k] += 1
        if len(read) == 1 and tr & set(TRACE_LIFT):
            one_limb_lift += 1
    return cnt, one_limb_lift
