"""A model of the device samplers, written against the text of include/fhelin.h "Sampler streams" (and DESIGN 7d / 7m), not against
csrc/: which ChaCha20 key and stream every random polynomial of the client side comes from, and how a block's words become
coefficients.  Plain module (no fixtures); tests/test_sampler_model_host.py pins it on the CPU, tests/test_client_randomness_gpu.py
holds the kernels to it residue for residue.

Ternary and flood coefficients are integer functions of the words.  The Gaussian is a REAL function,
    u1 = ((W_2j >> 11) + 1) 2^-53, u2 = (W_2j+1 >> 11) 2^-53, r = 3.19 sqrt(-2 ln u1), (round(r cos 2 pi u2), round(r sin 2 pi u2)),
evaluated here in np.longdouble (64-bit significand).  The kernel evaluates it in fp64: log, sqrt, sincos and three products, each
good to a few ulp on values of at most 28 (r <= 3.19 sqrt(2 * 53 ln 2) = 27.4), so the two evaluations differ by well under 2^-43.
A coefficient whose real value lies within BAND = 2^-40 of a half-integer could round either way; gaussian() counts those, and every
comparison asserts that the count is ZERO (about 2^-39 per coefficient: below 1e-5 over all tests).  A seed that ever produces one
is changed; the band is never widened and the cap never raised."""
import numpy as np

LD = np.longdouble
SIGMA = LD("3.19")
TWO_PI = LD(2) * LD("3.14159265358979323846264338327950288")
BAND = LD(2) ** -40
CHUNK = 32                                   # polynomials per sampler call where a caller chunks


def chacha20_words(seed, counter, stream):
    """ChaCha20 blocks (RFC 8439) for 64-bit counters (array), one 64-bit stream -> uint64 [len(counter)][8], little-endian
    (pinned to the RFC's vector, through the flood values, in tests/test_sanitize_host.py)"""
    ctr = np.atleast_1d(np.asarray(counter, dtype=np.uint64))
    key = np.frombuffer(bytes(seed), dtype="<u4")
    init = np.empty((16, ctr.size), dtype=np.uint32)
    init[0:4] = np.array([0x61707865, 0x3320646E, 0x79622D32, 0x6B206574], dtype=np.uint32)[:, None]
    init[4:12] = key[:, None]
    init[12] = (ctr & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    init[13] = (ctr >> np.uint64(32)).astype(np.uint32)
    init[14] = np.uint32(stream & 0xFFFFFFFF)
    init[15] = np.uint32(stream >> 32)
    x = init.copy()

    def rotl(v, k):
        return (v << np.uint32(k)) | (v >> np.uint32(32 - k))

    def qr(a, b, c, d):
        x[a] += x[b]; x[d] ^= x[a]; x[d] = rotl(x[d], 16)
        x[c] += x[d]; x[b] ^= x[c]; x[b] = rotl(x[b], 12)
        x[a] += x[b]; x[d] ^= x[a]; x[d] = rotl(x[d], 8)
        x[c] += x[d]; x[b] ^= x[c]; x[b] = rotl(x[b], 7)

    with np.errstate(over="ignore"):
        for _ in range(10):
            qr(0, 4, 8, 12); qr(1, 5, 9, 13); qr(2, 6, 10, 14); qr(3, 7, 11, 15)
            qr(0, 5, 10, 15); qr(1, 6, 11, 12); qr(2, 7, 8, 13); qr(3, 4, 9, 14)
        x += init
    w = x.astype(np.uint64)
    return (w[0::2] | (w[1::2] << np.uint64(32))).T


def flood_values(key, stream, bits, n):
    """coefficient i = (W >> (63 - B)) - 2^B, W = word i % 8 of block i / 8 (Python integers)"""
    W = chacha20_words(key, np.arange(n // 8, dtype=np.uint64), stream).reshape(-1)
    return [(int(w) >> (63 - bits)) - (1 << bits) for w in W]


def key_bytes(key_words):
    """eight u32 key words -> the 32 key bytes (little-endian), as chacha20_words takes them"""
    return np.asarray(key_words, dtype="<u4").tobytes()


def stream_of(calls, p):
    """stream number of polynomial p of the sampler call made at counter value `calls`"""
    return ((int(calls) << 32) + int(p)) & ((1 << 64) - 1)


def words(key_words, stream, n):
    """the n u64 words behind the n coefficients of one polynomial: word j of block b is coefficient 8 b + j's"""
    return chacha20_words(key_bytes(key_words), np.arange(n // 8, dtype=np.uint64), int(stream)).reshape(-1)


def ternary_from_words(W):
    """(W * 3 >> 64) - 1 in Python integers"""
    return np.array([((int(w) * 3) >> 64) - 1 for w in np.asarray(W).reshape(-1)], dtype=np.int64)


def gaussian_real(W, dtype=LD):
    """the real values r cos(2 pi u2), r sin(2 pi u2) before rounding, interleaved per word pair, in `dtype` arithmetic"""
    W = np.asarray(W, dtype=np.uint64).reshape(-1)
    a, b = W[0::2] >> np.uint64(11), W[1::2] >> np.uint64(11)
    if dtype is LD:
        scale, sigma, two_pi = LD(2) ** -53, SIGMA, TWO_PI
    else:
        scale, sigma, two_pi = dtype(2.0 ** -53), dtype(3.19), dtype(6.283185307179586476925)
    u1 = (a.astype(dtype) + dtype(1)) * scale             # (0, 1]: a + 1 <= 2^53 is exact in both types
    u2 = b.astype(dtype) * scale                          # [0, 1)
    r = np.sqrt(dtype(-2) * np.log(u1)) * sigma
    th = two_pi * u2
    x = np.empty(W.size, dtype=dtype)
    x[0::2] = r * np.cos(th)
    x[1::2] = r * np.sin(th)
    return x


def gaussian_from_words(W):
    """(coefficients int64, number of banded coefficients): the rounded Gaussian of the words in long double"""
    x = gaussian_real(W, LD)
    banded = int(np.count_nonzero(np.abs(np.abs(x - np.floor(x)) - LD("0.5")) < BAND))
    return np.rint(x).astype(np.int64), banded


def ternary(key_words, stream, n):
    return ternary_from_words(words(key_words, stream, n))


def gaussian(key_words, stream, n):
    return gaussian_from_words(words(key_words, stream, n))


def flood(key_words, stream, bits, n):
    """(W >> (63 - B)) - 2^B as an int64 array"""
    return np.array(flood_values(key_bytes(key_words), int(stream), int(bits), n), dtype=np.int64)


def residues(v, q):
    """signed integers v [..., N] -> residues [..., len(q), N] in [0, q_l) per limb"""
    v = np.asarray(v, dtype=np.int64)
    qs = np.array([int(x) for x in q], dtype=np.int64)
    return np.mod(v[..., None, :], qs[:, None]).astype(np.uint64)     # NumPy's mod takes the divisor's sign: in [0, q)


def ntt_of(orc, v, q, psi):
    """NTT form of the signed polynomials v [..., N] on the limbs q: through the oracle"""
    return orc.ntt_batch(residues(v, q), q, psi)


def enc_zero(orc, pk, u, w, e1, q, psi):
    """(pk_b NTT(u) + NTT(w), pk_a NTT(u) + NTT(e1)) on the limbs q [nl] for ONE ciphertext: pk [2][>= nl][N] NTT form, u / w / e1 signed
    integer polynomials [N] -> uint64 [2][nl][N]"""
    nl = len(q)
    U, Wn, E1 = (ntt_of(orc, x, q, psi) for x in (u, w, e1))
    c0 = orc.add(orc.mul(np.ascontiguousarray(pk[0][:nl]), U, q), Wn, q)
    c1 = orc.add(orc.mul(np.ascontiguousarray(pk[1][:nl]), U, q), E1, q)
    return np.stack([c0, c1])
