"""The sampler model (tests/sampler_model.py) and the read-only hook that tells a test which keys a call will use
(include/fhelin.h "Sampler streams", fhelin_debug_sampler_peek), on the CPU: the ternary map at its six boundary words, the Gaussian
model on 2^20 words (fp64 = long double coefficient for coefficient, no coefficient within 2^-40 of a rounding boundary, |e| <= 28, the
moments), the residue map, and the hook on device-less contexts - it consumes nothing, agrees between contexts of one seed and with
the generator as the header states it.  No device needed."""
import ctypes as C

import numpy as np

import sampler_model as sm
from sampler_model import chacha20_words


def test_ternary_map_at_its_boundaries():
    third, two_thirds = -(-(1 << 64) // 3), -(-(2 << 64) // 3)          # ceil(2^64 / 3), ceil(2 * 2^64 / 3)
    W = [0, third - 1, third, two_thirds - 1, two_thirds, (1 << 64) - 1]
    assert sm.ternary_from_words(np.array(W, dtype=np.uint64)).tolist() == [-1, -1, 0, 0, 1, 1]
    # the three values are equally likely to within 1 / 2^64
    assert third == two_thirds - third + 1 == (1 << 64) - two_thirds + 1


def test_gaussian_model_fp64_equals_long_double_on_2_20_words():
    assert np.finfo(sm.LD).nmant >= 63, "np.longdouble is no wider than fp64 here: the model needs the 64-bit significand"
    n = 1 << 20
    W = sm.words(np.arange(1, 9, dtype=np.uint32) * np.uint32(0x01020304), sm.stream_of(3, 1), n)
    assert W.shape == (n,) and len(set(W[:64].tolist())) == 64
    e, banded = sm.gaussian_from_words(W)
    assert banded == 0
    x64 = sm.gaussian_real(W, np.float64)
    xld = sm.gaussian_real(W, sm.LD)
    gap = float(np.abs(x64.astype(sm.LD) - xld).max())
    print("fp64 vs long double: largest difference of the real values", gap)
    assert gap < 2.0 ** -43                                              # the margin the 2^-40 band is built on
    assert np.array_equal(np.rint(x64).astype(np.int64), e)
    assert np.abs(e).max() <= 28
    f = e.astype(np.float64)
    # rounding adds 1/12 to the variance; 2^20 draws: the mean is good to 3.19 / 2^10 = 0.003 (x 5), the deviation to 0.0022 (x 5)
    assert abs(f.mean()) < 0.016 and abs(f.std() - np.sqrt(3.19 ** 2 + 1 / 12)) < 0.011
    # cosine and sine branches both there and not the same
    assert not np.array_equal(e[0::2], e[1::2])
    assert abs(np.corrcoef(f[0::2], f[1::2])[0, 1]) < 0.01
    # the extreme words: u1 = 2^-53 gives the largest radius, 27.34, on the cosine branch (u2 = 0); u1 = 1 gives 0
    top, _ = sm.gaussian_from_words(np.array([0, 0, (1 << 64) - 1, 0], dtype=np.uint64))
    assert top.tolist() == [27, 0, 0, 0]


def test_residues_are_reduced_per_limb():
    q = [97, (1 << 52) - 47]
    v = np.array([[-14, 8, 0, -1], [(1 << 62) + 5, -(1 << 62) - 28, 96, 97]], dtype=np.int64)
    r = sm.residues(v, q)
    assert r.shape == (2, 2, 4) and r.dtype == np.uint64
    for b in range(2):
        for l in range(2):
            assert r[b, l].tolist() == [int(x) % q[l] for x in v[b]]


def test_flood_is_the_pinned_restatement():
    # RFC 8439 2.3.2 key and nonce as tests/test_sanitize_host.py: block 0 here, so only shape, range and the key's byte order are checked
    kw = np.frombuffer(bytes(range(32)), dtype="<u4")
    assert sm.key_bytes(kw) == bytes(range(32))
    f = sm.flood(kw, 0x4A000000, 4, 64)
    assert f.shape == (64,) and f.min() >= -16 and f.max() < 16
    W = sm.words(kw, 0x4A000000, 64)
    assert f.tolist() == [(int(w) >> 59) - 16 for w in W]


def test_peek_consumes_nothing_and_follows_the_generator(fa):
    a, b, c = fa.Engine("toy", device=-1, seed=41), fa.Engine("toy", device=-1, seed=41), fa.Engine("toy", device=-1, seed=42)
    try:
        k1, calls = a.debug_sampler_peek(1)
        assert k1.shape == (1, 8) and k1.dtype == np.uint32 and calls == 0
        again, _ = a.debug_sampler_peek(1)
        assert np.array_equal(k1, again)                                 # two peeks are equal
        k2, _ = a.debug_sampler_peek(2)
        assert np.array_equal(k2[0], k1[0]) and not np.array_equal(k2[1], k2[0])
        assert np.array_equal(b.debug_sampler_peek(2)[0], k2)            # two contexts of one seed agree
        assert not np.array_equal(c.debug_sampler_peek(2)[0], k2)        # another seed: other keys
        # the generator as the header states it: ChaCha20(secret seed, stream 0), u64 words in order, four per key, low half first
        G = chacha20_words(a.secret_seed(), np.arange(4, dtype=np.uint64), 0).reshape(-1)
        k8, _ = a.debug_sampler_peek(8)
        want = np.stack([G[:32] & np.uint64(0xFFFFFFFF), G[:32] >> np.uint64(32)], axis=1).astype(np.uint32).reshape(8, 8)
        assert np.array_equal(k8, want)
        assert np.array_equal(a.debug_sampler_peek(1)[0], k1)            # still nothing consumed
    finally:
        for e in (a, b, c):
            e.close()


def test_peek_entry_point_and_its_arguments(fa):
    lib = fa.load_library()
    assert hasattr(lib, "fhelin_debug_sampler_peek") and hasattr(fa.Engine, "debug_sampler_peek")
    e = fa.Engine("toy", device=-1, seed=7)
    try:
        keys = np.zeros((2, 8), dtype=np.uint32)
        kp = keys.ctypes.data_as(C.c_void_p)
        calls = C.c_uint64(99)
        assert lib.fhelin_debug_sampler_peek(e.h, 2, kp, C.byref(calls)) == 0 and calls.value == 0 and keys.any()
        assert lib.fhelin_debug_sampler_peek(e.h, 2, kp, None) == 0      # the counter is optional
        assert lib.fhelin_debug_sampler_peek(e.h, 0, None, C.byref(calls)) == 0
        assert e.debug_sampler_peek(0)[0].shape == (0, 8)
        assert lib.fhelin_debug_sampler_peek(None, 1, kp, None) == 1     # FHELIN_ERR_ARG
        assert lib.fhelin_debug_sampler_peek(e.h, 1, None, None) == 1
        assert lib.fhelin_debug_sampler_peek(e.h, -1, kp, None) == 1
        assert lib.fhelin_debug_sampler_peek(e.h, 4097, kp, None) == 1
    finally:
        e.close()
