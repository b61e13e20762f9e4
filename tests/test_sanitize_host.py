"""Sanitised replies on the host (include/fhelin.h "Sanitised replies"): the three entry points exist, refuse NULL and zero-count
arguments and need a device; the Python restatement of the wide sampler that tests/test_sanitize_gpu.py holds the kernel to is pinned
here against values worked out by hand from the RFC 8439 section 2.3.2 block.  No device needed."""
import ctypes as C

import numpy as np

ERR_ARG, ERR_NO_DEVICE = 1, 2


def chacha20_words(seed, counter, stream):
    """ChaCha20 blocks (RFC 8439) for 64-bit counters (array), one 64-bit stream -> uint64 [len(counter)][8], little-endian
    (the helper of tests/test_compact_gpu.py)"""
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


def flood_values(key, stream, bits, n, first_counter=0):
    """the wide sampler by its definition: coefficient i = (W >> (63 - B)) - 2^B, W = word i % 8 of block first_counter + i / 8;
    Python integers"""
    W = chacha20_words(key, first_counter + np.arange(n // 8, dtype=np.uint64), stream).reshape(-1)
    return [(int(w) >> (63 - bits)) - (1 << bits) for w in W]


def flood_residues(f, q):
    return np.array([v % int(q) for v in f], dtype=np.uint64)   # Python's %: in [0, q) for negative v too


def test_sampler_restatement_against_hand_computed_values():
    # RFC 8439 2.3.2: key 00..1f, block count 1 and nonce 00:00:00:09:00:00:00:4a:00:00:00:00 = counter (0x09000000 << 32) | 1, stream
    # 0x4a000000; the block's 16 words, paired little-endian:
    #   15593bd1e4e7f110 c47120a31fdd0f50 0368c033c7f4d1c7 4e6cd4c39aaa2204 09aa9f07466482d2 a2028bd905d7c214 b94e16ded19c12b5 4e3c50a2e883d0cb
    key, ctr, stream = bytes(range(32)), (0x09000000 << 32) | 1, 0x4A000000
    # B = 1: the top two bits 00 11 00 01 00 10 10 01, minus 2
    assert flood_values(key, stream, 1, 8, ctr) == [-2, 1, -2, -1, -2, 0, 0, -1]
    # B = 4: the top five bits 00010 11000 00000 01001 00001 10100 10111 01001 = 2 24 0 9 1 20 23 9, minus 16
    assert flood_values(key, stream, 4, 8, ctr) == [-14, 8, -16, -7, -15, 4, 7, -7]
    # B = 62: (W >> 1) - 2^62; words 0 and 1: 0x0aac9de8f273f888 - 2^62 = -0x355362170d8c0778, 0x623890518fee87a8 - 2^62 = 0x223890518fee87a8
    f = flood_values(key, stream, 62, 8, ctr)
    assert f[0] == -0x355362170D8C0778 and f[1] == 0x223890518FEE87A8
    assert all(-(1 << 62) <= v < (1 << 62) for v in f)
    # residues: in [0, q), negative values wrap, |f| above q is reduced (q = 97: -14 = 83; 8; -16 = 81; ...)
    assert flood_residues([-14, 8, -16, -7, -15, 4, 7, -7], 97).tolist() == [83, 8, 81, 90, 82, 4, 7, 90]
    q = (1 << 52) - 47
    assert int(flood_residues(f[:1], q)[0]) == q - (0x355362170D8C0778 % q) and int(flood_residues(f[1:2], q)[0]) == 0x223890518FEE87A8 % q
    assert 0x355362170D8C0778 > q   # the case the 52-bit limbs meet at B = 62


def test_entry_points_exist(fa):
    lib = fa.load_library()
    for name in ("fhelin_sanitize", "fhelin_debug_flood", "fhelin_decrypt_flooded"):
        assert hasattr(lib, name), name
    for name in ("sanitize", "debug_flood", "decrypt_flooded"):
        assert hasattr(fa.Engine, name), name


def test_sanitize_calls_need_a_device_and_their_arguments(fa):
    lib = fa.load_library()
    e = fa.Engine("toy", device=-1)
    try:
        handles = (C.c_void_p * 1)(C.cast(C.create_string_buffer(64), C.c_void_p))   # never read: the device check comes first
        outs = (C.c_void_p * 1)()
        key = (C.c_uint8 * 32)(*range(32))
        words = np.zeros((1, e.N), dtype=np.uint64)
        slots = np.zeros(1 << e.params.log_slots)
        wp, sp = words.ctypes.data_as(C.c_void_p), slots.ctypes.data_as(C.POINTER(C.c_double))
        assert lib.fhelin_sanitize(e.h, handles, 1, None, 0, 2, outs) == ERR_NO_DEVICE
        assert lib.fhelin_debug_flood(e.h, key, 0, 20, 1, wp, words.size) == ERR_NO_DEVICE
        assert lib.fhelin_decrypt_flooded(e.h, handles[0], 20, sp, slots.size) == ERR_NO_DEVICE
        # NULL and zero-count arguments
        assert lib.fhelin_sanitize(None, handles, 1, None, 0, 2, outs) == ERR_ARG
        assert lib.fhelin_sanitize(e.h, None, 1, None, 0, 2, outs) == ERR_ARG
        assert lib.fhelin_sanitize(e.h, handles, 1, None, 0, 2, None) == ERR_ARG
        assert lib.fhelin_sanitize(e.h, handles, 0, None, 0, 2, outs) == ERR_ARG
        assert lib.fhelin_sanitize(e.h, handles, -1, None, 0, 2, outs) == ERR_ARG
        assert lib.fhelin_debug_flood(None, key, 0, 20, 1, wp, words.size) == ERR_ARG
        assert lib.fhelin_debug_flood(e.h, None, 0, 20, 1, wp, words.size) == ERR_ARG
        assert lib.fhelin_debug_flood(e.h, key, 0, 20, 1, None, words.size) == ERR_ARG
        assert lib.fhelin_decrypt_flooded(None, handles[0], 20, sp, slots.size) == ERR_ARG
        assert lib.fhelin_decrypt_flooded(e.h, None, 20, sp, slots.size) == ERR_ARG
        assert lib.fhelin_decrypt_flooded(e.h, handles[0], 20, None, slots.size) == ERR_ARG
        assert b"argument" in lib.fhelin_last_error()
    finally:
        e.close()
