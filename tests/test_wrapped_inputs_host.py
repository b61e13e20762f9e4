"""Wrapped inputs on the host (include/fhelin.h "Wrapped inputs"): the compact form version 2, built here byte for byte from the
documented layout, read back by fhelin_compact_info with its refusals; the new entry points exist and refuse what they must without
a device.  No device needed."""
import ctypes as C
import struct

import numpy as np
import pytest

ERR_ARG = 1


def wrapped_blob(log_n, moduli, c0, positions, total, slots=16384, scale=(2.0 ** 52, 0.0), header=None, count=None):
    """a version 2 blob: 104-byte fixed header (version 1's 96 + count, total), the ell moduli, the u32 positions padded to 8 bytes, c0"""
    N, ell = 1 << log_n, len(moduli)
    count = len(positions) if count is None else count
    H = 104 + 8 * ell + 8 * ((len(positions) + 1) // 2)
    b = bytearray(b"FHELINCC")
    b += struct.pack("<II", 2, H if header is None else header)
    b += struct.pack("<iiii", log_n, ell, 1, slots)
    b += struct.pack("<dd", *scale)
    b += struct.pack("<Q", 5) + bytes(range(32)) + struct.pack("<Q", 0)
    b += struct.pack("<II", count, total)
    b += struct.pack(f"<{ell}Q", *moduli)
    b += struct.pack(f"<{len(positions)}I", *positions)
    b += bytes(H - len(b))
    b += np.ascontiguousarray(c0, dtype="<u8").tobytes()
    assert len(b) == H + 8 * ell * N
    return bytes(b)


def info(fa, blob):
    lib = fa.load_library()
    v = [C.c_int32() for _ in range(4)]
    rc = lib.fhelin_compact_info(C.c_char_p(blob), len(blob), *[C.byref(x) for x in v])
    return rc, [x.value for x in v]


def test_entry_points_exist(fa):
    lib = fa.load_library()
    for name in ("fhelin_client_ingest_wrapped", "fhelin_unwrap_inputs", "fhelin_wrapped_info"):
        assert hasattr(lib, name), name
    assert hasattr(fa.Engine, "client_ingest_wrapped") and hasattr(fa.Engine, "unwrap_inputs")


def test_version_2_header_is_read(fa):
    log_n, moduli = 12, [1000003, 1000033, 1000037]
    c0 = np.zeros((3, 1 << 12), dtype=np.uint64)
    for pos in ([0], [0, 5, 7], list(range(1, 129))):
        rc, v = info(fa, wrapped_blob(log_n, moduli, c0, pos, total=200, slots=2048))
        assert rc == 0 and v == [log_n, 3, 1, 2048], pos


def test_version_2_refusals(fa):
    log_n, moduli = 12, [1000003, 1000033, 1000037]
    c0 = np.zeros((3, 1 << 12), dtype=np.uint64)
    good = wrapped_blob(log_n, moduli, c0, [1, 4, 9], total=20, slots=2048)
    assert info(fa, good)[0] == 0
    bad = {
        "count above positions": wrapped_blob(log_n, moduli, c0, [1, 4, 9], total=20, slots=2048, count=4),
        "count zero": wrapped_blob(log_n, moduli, c0, [1, 4, 9], total=20, slots=2048, count=0),
        "total below count": wrapped_blob(log_n, moduli, c0, [0, 1, 2], total=2, slots=2048),
        "position outside total": wrapped_blob(log_n, moduli, c0, [1, 4, 20], total=20, slots=2048),
        "positions not increasing": wrapped_blob(log_n, moduli, c0, [4, 1, 9], total=20, slots=2048),
        "one limb": wrapped_blob(log_n, moduli[:1], c0[:1], [1, 4, 9], total=20, slots=2048),
        "header size": wrapped_blob(log_n, moduli, c0, [1, 4, 9], total=20, slots=2048, header=96 + 8 * 3),
        "truncated": good[:-8],
        "padding": good[:104 + 24 + 12] + b"\x01" + good[104 + 24 + 13:],
        "version 3": good[:8] + struct.pack("<I", 3) + good[12:],
    }
    for why, blob in bad.items():
        assert info(fa, blob)[0] == ERR_ARG, why


def test_wrapped_calls_need_a_device(fa):
    e = fa.Engine("toy", device=-1)
    try:
        lib = fa.load_library()
        outs = (C.c_void_p * 1)()
        assert lib.fhelin_unwrap_inputs(e.h, outs, 1, outs) != 0
        assert lib.fhelin_wrapped_info(None, None, None, None, None, 0) == ERR_ARG
    finally:
        e.close()
