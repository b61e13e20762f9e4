"""Compact ciphertexts on the host: ChaCha20 restated in NumPy (RFC 8439 section 2.3.2, and the library's fhelin_prng_block under
the expansion's (l << 32) | b counter / nonce stream mapping), the expansion of c1 (include/fhelin.h "Compact ciphertexts")
restated with Python integers, and the header reader fhelin_compact_info on blobs built here from the documented format, with
its refusals.  No device needed."""
import ctypes as C
import struct

import numpy as np
import pytest

ERR_ARG = 1
M32 = np.uint32(0xFFFFFFFF)


def chacha20_words(seed, counter, stream):
    """ChaCha20 blocks (RFC 8439 block function) for key `seed` (32 bytes), 64-bit counters (array) and one 64-bit stream:
    the state layout of fhelin_prng_block (counter in words 12-13, stream in 14-15) -> uint64 [len(counter)][8], little-endian"""
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


def expand_c1(seed, nonce, limb, q, N):
    """the expansion: c1[limb][j] = (W[2k+1] * 2^64 + W[2k]) mod q, b = j / 4, k = j % 4, W = ChaCha20(seed, (limb << 32) | b,
    nonce) -> uint64 [N]"""
    b = np.arange(N // 4, dtype=np.uint64)
    W = chacha20_words(seed, (np.uint64(limb) << np.uint64(32)) | b, nonce)
    lo, hi = W[:, 0::2].reshape(-1), W[:, 1::2].reshape(-1)
    v = (hi.astype(object) * (1 << 64) + lo.astype(object)) % int(q)
    return v.astype(np.uint64)


def build_blob(log_n, ell, moduli, c0, deg=1, slots=None, scale=(2.0 ** 52, 0.0), nonce=3, seed=bytes(range(32)), digest=0,
               magic=b"FHELINCC", version=1, header=None):
    N = 1 << log_n
    slots = slots if slots is not None else N // 2
    h = bytearray(96)
    h[0:8] = magic
    struct.pack_into("<II4i2dQ", h, 8, version, 96 + 8 * ell if header is None else header, log_n, ell, deg, slots, scale[0], scale[1], nonce)
    h[56:88] = seed
    struct.pack_into("<Q", h, 88, digest)
    return bytes(h) + np.asarray(moduli, dtype="<u8").tobytes() + np.asarray(c0, dtype="<u8").tobytes()


def test_numpy_chacha20_rfc8439_and_prng_block(fa):
    lib = fa.load_library()
    key = bytes(range(32))
    # RFC 8439 2.3.2: nonce 00:00:00:09:00:00:00:4a:00:00:00:00, block count 1 = counter (0x09000000 << 32) | 1, stream 0x4a000000
    w = chacha20_words(key, (0x09000000 << 32) | 1, 0x4A000000)[0]
    want = bytes.fromhex("10f1e7e4d13b5915500fdd1fa32071c4c7d1f4c733c068030422aa9ac3d46c4e"
                         "d2826446079faa0914c2d705d98b02a2b5129cd1de164eb9cbd083e8a2503c4e")
    assert w.astype("<u8").tobytes() == want
    # the expansion's mapping: counter (l << 32) | b, stream = nonce
    rng = np.random.default_rng(5)
    seed = rng.integers(0, 256, 32, dtype=np.uint8).tobytes()
    out = (C.c_uint8 * 64)()
    for l, b, nonce in [(0, 0, 0), (0, 1, 0), (3, 1023, 7), (27, 16383, 193), (63, 5, (1 << 64) - 1)]:
        assert lib.fhelin_prng_block(seed, C.c_uint64((l << 32) | b), C.c_uint64(nonce), out) == 0
        assert chacha20_words(seed, (l << 32) | b, nonce)[0].astype("<u8").tobytes() == bytes(out), (l, b, nonce)


def test_expansion_restated_with_python_integers(fa):
    lib = fa.load_library()
    e = fa.Engine("toy", device=-1)
    try:
        N, q = e.N, [int(v) for v in e.q]
        seed = bytes(range(100, 132))
        nonce = 11
        out = (C.c_uint8 * 64)()
        for l in (0, len(q) - 1):
            c1 = expand_c1(seed, nonce, l, q[l], N)
            assert c1.shape == (N,) and int(c1.max()) < q[l]
            for j in (0, 1, 2, 3, 4, 77, N - 1):
                b, k = divmod(j, 4)
                assert lib.fhelin_prng_block(seed, C.c_uint64((l << 32) | b), C.c_uint64(nonce), out) == 0
                W = struct.unpack("<8Q", bytes(out))
                assert int(c1[j]) == (W[2 * k + 1] * 2 ** 64 + W[2 * k]) % q[l], (l, j)
            # close to uniform: the mean of N residues within 5 standard deviations of q / 2
            assert abs(float(np.mean(c1.astype(np.float64))) - q[l] / 2) < 5 * q[l] / np.sqrt(12 * N)
        # another nonce, another limb: other residues
        assert not np.array_equal(expand_c1(seed, nonce, 0, q[0], N), expand_c1(seed, nonce + 1, 0, q[0], N))
        assert not np.array_equal(expand_c1(seed, nonce, 0, q[1], N), expand_c1(seed, nonce, 1, q[1], N))
    finally:
        e.close()


def _code(fa, blob):
    with pytest.raises(fa.FhelinError) as ei:
        fa.compact_info(blob)
    return ei.value.code


def test_compact_info_accepts_a_synthetic_blob_and_refuses_malformed_ones(fa):
    log_n, ell = 12, 3
    N = 1 << log_n
    moduli = [(1 << 55) - 55, (1 << 52) - 47, (1 << 52) - 143]
    c0 = np.arange(ell * N, dtype=np.uint64)
    good = build_blob(log_n, ell, moduli, c0, deg=1, slots=1024)
    assert len(good) == 96 + 8 * ell + 8 * ell * N
    assert fa.compact_info(good) == dict(log_n=log_n, ell=ell, deg=1, slots=1024)
    assert fa.compact_info(build_blob(log_n, 1, moduli[:1], c0[:N], deg=2, slots=2048)) == dict(log_n=log_n, ell=1, deg=2, slots=2048)
    bad = {
        "magic": build_blob(log_n, ell, moduli, c0, magic=b"FHELINEK"),
        "version": build_blob(log_n, ell, moduli, c0, version=2),
        "header size": build_blob(log_n, ell, moduli, c0, header=96 + 8 * ell + 8),
        "truncated": good[:-8],
        "truncated header": good[:90],
        "oversized": good + bytes(8),
        "ell 0": build_blob(log_n, 0, [], []),
        "ell -1": build_blob(log_n, -1, [], [], header=88),
        "ell too many": build_blob(log_n, 65, [1] * 65, []),
        "log_n": build_blob(11, ell, moduli, np.zeros(ell << 11, dtype=np.uint64)),
        "deg": build_blob(log_n, ell, moduli, c0, deg=0),
        "slots": build_blob(log_n, ell, moduli, c0, slots=1000),
        "scale": build_blob(log_n, ell, moduli, c0, scale=(-1.0, 0.0)),
        "digest field": build_blob(log_n, ell, moduli, c0, digest=(1 << 61) - 1),
    }
    for what, blob in bad.items():
        assert _code(fa, blob) == ERR_ARG, what
