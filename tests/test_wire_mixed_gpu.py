"""One import pipeline behind the blob formats and the device transport (csrc/wire.cpp): ciphertexts are allocated and range-checked
shape by shape and handed back in CALLER order.  Every call here interleaves the shapes so that group order and caller order differ,
gives every source its own residues, degree and slot count, and asks each result for exactly its own source; a refusal must name the
caller's index of the bad blob or frame.  N = 2^12.

A wrapped input needs the 2^14 slots of a larger ring to be MADE, but its blob is only a header around a seeded c0 (the digest covers
the payload alone), so the wrapped blobs here are seeded blobs of this ring with the header rewritten by hand as include/fhelin.h
describes it.  A wrapped handle cannot be exported; it is compared through info(), scale_parts(), wrapped_info() and its decryption,
which reads the first two limbs of both components, c1 being the expansion of the blob's seed and nonce.

Already asserted elsewhere and not repeated: several (stored, ell) groups of full packed blobs through one call
(test_packed_gpu.test_full_round_trips_sizes_and_mixed_limb_counts), a bad payload bit and a bad residue among same-format blobs
(test_packed_gpu.test_all_or_nothing), the range check of two equal frames (test_device_transport_gpu.test_range_check)."""
import ctypes as C
import struct

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ERR_ARG = 1
RAW, PACKED = 0, 1


@pytest.fixture(scope="module")
def client(fa):
    e = fa.Engine("toy", seed=91)
    e.keygen()
    yield e
    e.close()


def _rand_limbs(e, npoly, ell, seed):
    rng = np.random.default_rng(seed)
    return np.stack([np.stack([rng.integers(0, int(q), e.N, dtype=np.uint64) for q in e.q[:ell]]) for _ in range(npoly)])


def _seeded(e, ell, seed, slots):
    """a seeded (secret-key) encryption at ell limbs"""
    x = np.random.default_rng(seed).uniform(-1, 1, slots)
    return e.encrypt(x, level=e.n_q - ell, slots=slots)


def _positions(pos):
    return struct.pack("<%di" % len(pos), *pos) + b"\0" * (4 * (len(pos) % 2))


def _wrap_packed(blob, pos, total):
    """a seeded packed blob with the header of a wrapped input: count and total at 100, the positions after the moduli"""
    H, ell = struct.unpack_from("<I", blob, 12)[0], struct.unpack_from("<i", blob, 20)[0]
    assert H == 112 + 8 * ell and struct.unpack_from("<3I", blob, 96) == (1, 0, 0)
    head = bytearray(blob[:H]) + _positions(pos)
    struct.pack_into("<II", head, 100, len(pos), total)
    struct.pack_into("<I", head, 12, len(head))
    return bytes(head) + blob[H:]


def _wrap_compact(blob, pos, total):
    """a version 1 compact blob as version 2: count and total at 96, then the moduli, then the positions"""
    H, ell = struct.unpack_from("<I", blob, 12)[0], struct.unpack_from("<i", blob, 20)[0]
    assert H == 96 + 8 * ell and struct.unpack_from("<I", blob, 8)[0] == 1
    head = bytearray(blob[:96]) + struct.pack("<ii", len(pos), total) + blob[96:H] + _positions(pos)
    struct.pack_into("<I", head, 8, 2)
    struct.pack_into("<I", head, 12, len(head))
    return bytes(head) + blob[H:]


def _same(e, got, src, wrapped=None):
    """got holds what src holds; wrapped: (positions, total) of the header got was imported with"""
    ig, isrc = got.info(), src.info()
    assert (ig["npoly"], ig["ell"], ig["deg"], ig["slots"]) == (isrc["npoly"], isrc["ell"], isrc["deg"], isrc["slots"])
    assert got.scale_parts() == src.scale_parts()
    if wrapped is None:
        assert np.array_equal(got.export(), src.export())
    else:
        assert got.wrapped_info() == dict(count=len(wrapped[0]), total=wrapped[1], ell=isrc["ell"] - 1, positions=list(wrapped[0]))
        assert np.array_equal(e.decrypt(got), e.decrypt(src))


def _call(e, fn, blobs):
    """the C call itself: (status, message, outs)"""
    ptrs = (C.c_void_p * len(blobs))(*[C.cast(C.c_char_p(b), C.c_void_p) for b in blobs])
    sizes = (C.c_size_t * len(blobs))(*[len(b) for b in blobs])
    outs = (C.c_void_p * len(blobs))()
    rc = fn(e.h, ptrs, sizes, len(blobs), outs)
    return rc, e.lib.fhelin_last_error().decode(), list(outs)


def test_packed_import_of_interleaved_shapes(fa, client):
    e = client
    assert e.N == 1 << 12
    W = ([1, 3], 5)
    e.set_seeded_encryption(True)
    try:
        srcs = [
            _seeded(e, 3, 1, 1 << 11),                                         # stored 2, ell 3
            _seeded(e, 2, 2, 1 << 10),                                         # seeded, ell 2
            e.ct_import(_rand_limbs(e, 3, 3, 3), deg=2, slots=1 << 9),         # stored 3, ell 3
            _seeded(e, 3, 4, 1 << 8),                                          # seeded wrapped, ell 3
            e.ct_import(_rand_limbs(e, 2, 3, 5), deg=2, slots=1 << 7),         # stored 2, ell 3
        ]
        blobs = [srcs[0].export_packed(), srcs[1].export_packed(seeded=True), srcs[2].export_packed(),
                 _wrap_packed(srcs[3].export_packed(seeded=True), *W), srcs[4].export_packed()]
    finally:
        e.set_seeded_encryption(False)
    shapes = [(i["stored"], i["ell"], i["count"]) for i in map(fa.packed_info, blobs)]
    assert shapes == [(2, 3, 0), (1, 2, 0), (3, 3, 0), (1, 3, 2), (2, 3, 0)]
    got = e.import_packed(blobs)
    for k, (g, s) in enumerate(zip(got, srcs)):
        _same(e, g, s, W if k == 3 else None)
    # one payload field of blob 3 at 2^w - 1, above its modulus: residue 9 of the second limb vector
    ws = [int(q).bit_length() for q in e.q[:3]]
    H = struct.unpack_from("<I", blobs[3], 12)[0]
    stream = int.from_bytes(blobs[3][H:], "little") | (((1 << ws[1]) - 1) << (e.N * ws[0] + 9 * ws[1]))
    over = blobs[3][:H] + stream.to_bytes(len(blobs[3]) - H, "little")
    rc, msg, outs = _call(e, e.lib.fhelin_ct_import_packed, blobs[:3] + [over] + blobs[4:])
    assert rc == ERR_ARG and "blob 3" in msg and "range" in msg, msg
    assert outs == [None] * 5
    # only the digest field of blob 1 changed
    dg = bytearray(blobs[1])
    dg[88] ^= 1
    rc, msg, outs = _call(e, e.lib.fhelin_ct_import_packed, [blobs[0], bytes(dg)] + blobs[2:])
    assert rc == ERR_ARG and "blob 1" in msg and "digest" in msg, msg
    assert outs == [None] * 5


def test_compact_import_of_both_versions_interleaved(fa, client):
    e = client
    W = {1: ([0], 1), 2: ([2, 3, 7], 9)}
    e.set_seeded_encryption(True)
    try:
        # limb counts 4 and 3: a decryption reads two limbs of either, with or without the wrapped header (whose last limb is left out)
        srcs = [_seeded(e, ell, 10 + k, 1 << (6 + k)) for k, ell in enumerate([4, 3, 4, 3, 4])]
        blobs = [s.export_compact() for s in srcs]
    finally:
        e.set_seeded_encryption(False)
    for k in W:
        blobs[k] = _wrap_compact(blobs[k], *W[k])                              # version 1, 2, 2, 1, 1 at ell 4, 3, 4, 3, 4
    assert [struct.unpack_from("<I", b, 8)[0] for b in blobs] == [1, 2, 2, 1, 1]
    got = e.import_compact(blobs)
    for k, (g, s) in enumerate(zip(got, srcs)):
        _same(e, g, s, W.get(k))
    dg = bytearray(blobs[2])
    dg[88] ^= 1
    rc, msg, outs = _call(e, e.lib.fhelin_ct_import_compact, blobs[:2] + [bytes(dg)] + blobs[3:])
    assert rc == ERR_ARG and "blob 2" in msg and "digest" in msg, msg
    assert outs == [None] * 5


def _pack_model(v, w):
    """the packed limb vector of the residues v at width w, as bytes (64 residues are exactly w words)"""
    out = bytearray()
    for g in range(0, len(v), 64):
        stream = 0
        for j, x in enumerate(v[g:g + 64]):
            stream |= int(x) << (j * w)
        out += stream.to_bytes(8 * w, "little")
    return bytes(out)


def _frame(e, limbs, fmt):
    limbs = np.ascontiguousarray(limbs, dtype="<u8")
    if fmt == RAW:
        return limbs.tobytes()
    return b"".join(_pack_model(vec, int(e.q[l]).bit_length()) for comp in limbs for l, vec in enumerate(comp))


def test_transport_import_of_interleaved_frames(fa, client):
    import torch
    e = client
    # (2, ell 3) and (3, ell 2) in turn; raw and packed in turn, the other way round in the second half: each shape in both formats
    shapes = [(2, 3), (3, 2)] * 4
    fmts = [RAW, PACKED] * 2 + [PACKED, RAW] * 2
    limbs = [_rand_limbs(e, npoly, ell, 20 + k) for k, (npoly, ell) in enumerate(shapes)]

    def on_device(frames, stride):
        t = torch.from_numpy(np.frombuffer(b"".join(f.ljust(stride, b"\xA5") for f in frames), dtype=np.uint8).copy()).cuda()
        torch.cuda.synchronize()                                               # a call without a stream expects finished frames
        return t

    frames = [_frame(e, l, f) for l, f in zip(limbs, fmts)]
    stride = -(-max(map(len, frames)) // 16) * 16
    meta = np.array([[npoly, ell, 1 + k % 2, 1 << (3 + k), 2.0 ** 52 + 2 * k, 0.0, len(frames[k]), fmts[k]]
                     for k, (npoly, ell) in enumerate(shapes)], dtype=np.float64)
    buf = on_device(frames, stride)
    got = e.import_device_many(buf.data_ptr(), stride, meta, check=True)
    for k, g in enumerate(got):
        i = g.info()
        assert (i["npoly"], i["ell"], i["deg"], i["slots"]) == (*shapes[k], 1 + k % 2, 1 << (3 + k))
        assert g.scale_parts() == (2.0 ** 52 + 2 * k, 0.0)
        assert np.array_equal(g.export(), limbs[k]), k
    # one residue of frame 2 equal to its modulus
    bad = limbs[2].copy()
    bad[1, 2, 77] = e.q[2]
    buf = on_device(frames[:2] + [_frame(e, bad, fmts[2])] + frames[3:], stride)
    with pytest.raises(fa.FhelinError) as ei:
        e.import_device_many(buf.data_ptr(), stride, meta, check=True)
    assert ei.value.code == ERR_ARG and "frame 2" in str(ei.value) and "range" in str(ei.value)
