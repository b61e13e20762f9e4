"""The client's number conversion stated from its definitions, in Python int / fractions.Fraction (no mantissa products, no shifts).

Encoder.  A slot value c (a double) at scale S = ms * 2^es (a long double: 2^63 <= ms < 2^64) becomes the integer
    K = sign(c) * round_half_away( RNE64(|c| * S) )
where RNE64 rounds a positive real to 64 significant bits, ties to even: `llroundl((long double)c * S)` on x87.  The device kernel
x87_mul_round (csrc/kernels_client.hip) and the host leg ld_to_i128 + reduce_i128_kernel both promise exactly this.

Decoder.  A phase coefficient with residues K mod q_l becomes the double
    RNE53( RNE64( RNE64(centred(K mod M)) / S ) ),   M = q_0 (one limb read) or q_0 q_1
(Client::decrypt: the centred CRT lift as hi * 2^64 + lo in long double, divided by the scale, converted to double).

An exact channel reaches both without any floating-point noise: the constant vector (c, ..., c) goes through the inverse special FFT
exactly (every butterfly difference is 0, the sums are 2c, 4c, ... n c, the final 1/n is exact), so the encoding is the constant
polynomial K; and a ciphertext (c0, c1) = (K at every NTT position, 0) has phase K, which decodes to the same double in every slot.

Each function returns the set of edges a case touches (TRACE_ENCODE / TRACE_DECODE); cases() is the generator the tests share and
census() counts what it reaches.  tests/test_encode_rounding_host.py holds both against numpy.longdouble where that is the x87 format."""
from fractions import Fraction
import functools
import math
import random
import struct

TWO64 = 1 << 64
HOST_SWITCH = 9 * 10 ** 18                     # ld_to_i128: |v| below it goes through llroundl, at or above through the 128-bit split
ODD52 = (0xC3A5C85C97CB3127, -11)             # an odd long-double scale near 2^52 (slot-count sweep, decoder)
DOMAIN = 1 << 125                              # the encoder refuses whatever may reach it (in_domain)

TRACE_ENCODE = ("tie1_down", "tie1_up", "carry", "tie2", "below_half", "half_to_one", "ge_2^64", "double_rounding", "subnormal", "zero",
                "host_big", "host_lo_zero")
TRACE_DECODE = ("at_half", "above_half", "max", "zero")
SIGNED = ("tie1_down", "tie1_up", "carry")     # categories the census wants with both signs


# ------------------------------------------------------------------------------------------------------------------ rounding primitives
def round_sig(x, bits):
    """(x > 0 rounded to `bits` significant bits, ties to even; what happened: "exact" / "down" / "up" / "tie_down" / "tie_up";
    whether rounding up crossed a power of two)"""
    x = Fraction(x)
    assert x > 0
    e = (x.numerator.bit_length() - x.denominator.bit_length()) - bits
    while x >= Fraction(2) ** (e + bits):
        e += 1
    while x < Fraction(2) ** (e + bits - 1):
        e -= 1
    ulp = Fraction(2) ** e
    n = x / ulp                                  # 2^(bits-1) <= n < 2^bits
    fl = n.numerator // n.denominator
    rem = n - fl
    if rem == 0:
        return x, "exact", False
    if rem == Fraction(1, 2):
        how = "tie_up" if fl & 1 else "tie_down"
    else:
        how = "up" if rem > Fraction(1, 2) else "down"
    up = how in ("up", "tie_up")
    return (fl + up) * ulp, how, up and fl + 1 == 1 << bits


def half_away(y):
    """y >= 0 rounded to an integer, halves up (away from zero for the magnitude)"""
    return (2 * y.numerator + y.denominator) // (2 * y.denominator)


def scale_of(ms, es):
    assert (1 << 63) <= ms < TWO64
    return Fraction(ms) * Fraction(2) ** es


def scale_parts(x):
    """a positive real that has at most 64 significant bits -> (ms, es)"""
    x = Fraction(x)
    y, how, _ = round_sig(x, 64)
    assert how == "exact", "not a long double"
    es = 0
    while x >= TWO64:
        x /= 2
        es += 1
    while x < 1 << 63:
        x *= 2
        es -= 1
    assert x.denominator == 1
    return int(x), es


@functools.lru_cache(maxsize=None)
def hi_lo(ms, es):
    """the scale as the two doubles the C ABI takes (hi + lo is exact: 53 + 11 bits)"""
    s = scale_of(ms, es)
    hi = float(round_sig(s, 53)[0])
    lo = s - Fraction(hi)
    assert Fraction(float(lo)) == lo
    return hi, float(lo)


def is_subnormal(c):
    return c != 0.0 and abs(c) < 2.0 ** -1022


# ------------------------------------------------------------------------------------------------------------------------------ encoder
def encode_int(c, ms, es):
    """(K, trace) for the slot value c (a Python float) at scale ms * 2^es"""
    trace = set()
    neg = math.copysign(1.0, c) < 0
    if c == 0.0:
        return 0, {"zero"}
    if is_subnormal(c):
        trace.add("subnormal")
    s = scale_of(ms, es)
    x = abs(Fraction(c)) * s
    y, how, crossed = round_sig(x, 64)
    if how in ("tie_down", "tie_up"):
        trace.add("tie1_" + how[4:])
    if crossed:
        trace.add("carry")
    r = half_away(y)
    if y - (y.numerator // y.denominator) == Fraction(1, 2):
        trace.add("tie2")
    if y < Fraction(1, 2):
        trace.add("below_half")
    elif y < 1:
        trace.add("half_to_one")
    if r >= TWO64:
        trace.add("ge_2^64")
    if s < 1 << 63 and r != half_away(x):
        trace.add("double_rounding")
    if r >= HOST_SWITCH:
        trace.add("host_big")
    if neg and r and r % TWO64 == 0:
        trace.add("host_lo_zero")
    return (-r if neg else r), trace


def in_domain(c, ms, es):
    """what the encoder accepts (include/fhelin.h): floor(log2 |c|) + floor(log2 S) <= 123, which keeps |c| * S below DOMAIN"""
    if c == 0.0:
        return True
    ok = (math.frexp(abs(c))[1] - 1) + (es + 63) <= 123
    assert not ok or abs(Fraction(c)) * scale_of(ms, es) < DOMAIN
    return ok


# ------------------------------------------------------------------------------------------------------------------------------ decoder
def centred(K, M):
    x = K % M
    return x - M if x > M // 2 else x


def decode_double(K, moduli_read, ms, es):
    """(the double every slot of the decryption holds, trace) for a constant phase K read on one or two limbs"""
    assert len(moduli_read) in (1, 2)
    M = 1
    for q in moduli_read:
        M *= int(q)
    x = K % M
    trace = set()
    if x == 0:
        trace.add("zero")
    if x == M // 2:
        trace.add("at_half")
    if x == M // 2 + 1:
        trace.add("above_half")
    if x == M - 1:
        trace.add("max")
    v = centred(K, M)
    if v == 0:
        return 0.0, trace
    mag = round_sig(abs(v), 64)[0]               # hi * 2^64 + lo in long double
    quo = round_sig(mag / scale_of(ms, es), 64)[0]
    d = float(round_sig(quo, 53)[0])
    return (-d if v < 0 else d), trace


def decode_cases(moduli_read, seed):
    """the boundary phases of the centred lift over M and 20 uniform ones"""
    M = 1
    for q in moduli_read:
        M *= int(q)
    rng = random.Random(seed)
    return [0, 1, -1, M // 2, M // 2 + 1, M - 1, M // 2 - 1] + [rng.randrange(M) for _ in range(20)]


# ---------------------------------------------------------------------------------------------------------------- the engine's own scales
def delta_chain(q):
    """Delta_0 = q_L, Delta_{k+1} = Delta_k^2 / q_{L-k}, each product and quotient rounded to 64 bits (context.cpp sf_real) -> [(ms, es)]"""
    q = [int(x) for x in q]
    L = len(q) - 1
    out = [Fraction(q[L])]
    for k in range(L):
        sq = round_sig(out[k] * out[k], 64)[0]
        out.append(round_sig(sq / q[L - k], 64)[0])
    return [scale_parts(x) for x in out]


# ------------------------------------------------------------------------------------------------------------------------ case generator
def _f(x):
    """the double nearest to a positive rational"""
    return float(round_sig(x, 53)[0])


def _step(c, k):
    """c moved by k units in the last place"""
    (b,) = struct.unpack("<q", struct.pack("<d", c))
    return struct.unpack("<d", struct.pack("<q", b + k))[0]


def _tie_scale(rng, mv, es):
    """a 64-bit significand at which the odd integer mv makes a first-rounding tie: with sh bits dropped the product must end in a one
    and sh - 1 zeros, so ms ends the same way (times mv^-1, which is odd)"""
    b = mv.bit_length()
    for _ in range(64):
        sh = rng.choice((b - 1, b)) if b > 1 else 1
        if sh < 1:
            continue
        ms = (rng.getrandbits(64) | (1 << 63)) >> sh << sh | (1 << (sh - 1))
        if (mv * ms).bit_length() - 64 == sh:
            return ms, es
    raise AssertionError("no tie scale found")


def carry_pairs(rng, n):
    """(mv, ms) with mv * ms within 2^51 below 2^116: 64 ones then a remainder of at least one half - the rounding carries out of 64 bits.
    The scale is built from the value."""
    out = []
    while len(out) < n:
        mv = rng.randrange((1 << 52) + 1, 1 << 53)
        ms = ((1 << 116) - 1) // mv
        if (1 << 63) <= ms < TWO64 and (1 << 116) - mv * ms <= 1 << 51:
            out.append((mv, ms))
    return out


def scales(deltas, seed=20240521):
    """[(name, ms, es)]: the engine's Delta of every level given, long doubles with odd significands near 2^52 and 2^104, doubles (11
    trailing zero bits) near both"""
    rng = random.Random(seed)
    out = [("delta%d" % k, ms, es) for k, (ms, es) in enumerate(deltas)]
    for es, tag in ((-11, "52"), (41, "104")):
        for i in range(2):
            out.append(("odd%s_%d" % (tag, i), rng.getrandbits(64) | (1 << 63) | 1, es))
        out.append(("oddlow%s" % tag, (1 << 63) | rng.getrandbits(61) | 1, es))       # 3 * ms stays below 2^65: one bit dropped at 1.5
        for i in range(2):
            out.append(("dbl%s_%d" % (tag, i), (rng.getrandbits(53) | (1 << 52) | 1) << 11, es))
    return out


FEW_BITS = (1.0, 1.5, 0.75, 1.25, 0.625, 3.0, 0.375, 1.75, 2.5, 0.5, 1024.0)


def cases(deltas, seed=20240521):
    """[(c, ms, es)] inside the encoder's domain; `deltas` = delta_chain(q)[levels of interest].  Deterministic."""
    rng = random.Random(seed + 1)
    out = []

    def both(c, ms, es):
        for v in (c, -c):
            if in_domain(v, ms, es):
                out.append((v, ms, es))

    for name, ms, es in scales(deltas, seed):
        s = scale_of(ms, es)
        for c in FEW_BITS:
            both(c, ms, es)
        for _ in range(10):                                   # k/4096, k/8192 with 12- and 13-bit k: ties at scales that are doubles
            k = rng.randrange(2048, 8192) | 1
            both(k / 4096.0, ms, es)
            both(k / 8192.0, ms, es)
        both(0.0, ms, es)
        both(5e-324, ms, es)
        both(2.0 ** -1040 * 3, ms, es)
        for num in (Fraction(1, 4), Fraction(1, 2), Fraction(3, 4), Fraction(3, 2), Fraction(5, 2), Fraction(2001, 2)):
            c = _f(num / s)                                   # (j + 1/2) / scale and its neighbours
            for k in (-1, 0, 1):
                both(_step(c, k), ms, es)
        c = _f(Fraction(HOST_SWITCH) / s)                     # both sides of the host's switch
        for k in (-3, -1, 0, 1, 3):
            both(_step(c, k), ms, es)
        for _ in range(12):                                   # products in [2^61, 2^63): one or two fraction bits survive the first rounding
            both(_f(Fraction(rng.randrange(1 << 61, 1 << 63)) / s), ms, es)
        for m in (1, 2, 3, 1 << 20):                          # both sides of multiples of 2^64
            c = _f(Fraction(m * TWO64) / s)
            for k in (-1, 0, 1):
                both(_step(c, k), ms, es)
        for j in (64, 65, 70):                                # exact products that are multiples of 2^64 where the scale has trailing zeros
            both(2.0 ** j, ms, es)
            both(3 * 2.0 ** j, ms, es)
    # scales built from the value: first-rounding ties at few-bit values
    for es in (-11, 41):
        for mv, ex in ((3, -1), (3, -2), (5, -2), (7, -2), (5, -3), (11, -3), (4095, -12), (2049, -12), (6145, -13), (8191, -13)):
            for _ in range(3):
                ms, _ = _tie_scale(rng, mv, es)
                both(mv * 2.0 ** ex, ms, es)
    # ... and carries out of 64 bits, the rounded product landing on 1/4, 1/2, 1, 2^53, 2^64 and 2^70
    for mv, ms in carry_pairs(rng, 8):
        for es in (-11, 41):
            for target in (-2, -1, 0, 53, 64, 70):            # the rounded product is 2^target
                ev = target - 116 - es
                both(math.ldexp(float(mv), ev), ms, es)
    return out


def census(case_list):
    """{category: [count with c >= 0, count with c < 0]} over TRACE_ENCODE"""
    cnt = {k: [0, 0] for k in TRACE_ENCODE}
    for c, ms, es in case_list:
        for k in encode_int(c, ms, es)[1]:
            cnt[k][math.copysign(1.0, c) < 0] += 1
    return cnt
