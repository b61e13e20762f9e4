"""csrc/decode_lift.h on the host, against tests/decode_model.py, bit for bit.

The header is host/device code (like modarith.h): the device decoder (decode_lift_kernel) runs exactly this function per coefficient.  Here
it is compiled with g++ into a small stand-alone program (tests/shim/decode_lift_host.cpp), fed every generated case as residues, and its
doubles are compared as bit patterns with the model's - and, where numpy.longdouble is the x87 format, with the arithmetic
Client::decrypt_physical runs on the host: (long double)hi * 2^64 + lo, divided by the scale, converted to double.  The census holds the
generator to at least 4 cases of every edge.  The same file pins the status codes fhelin_decrypt_batch gives without a device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import decode_model as dm
import encode_model as em

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG, ERR_NO_DEVICE = 1, 2


@pytest.fixture(scope="module")
def lift_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("decode_lift") / "decode_lift_host")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", os.path.join(ROOT, "tests", "shim", "decode_lift_host.cpp"), "-o", exe])
    return exe


@pytest.fixture(scope="module")
def toy(fa):
    """(the toy chain's Q moduli, its Delta per level as (ms, es), the generated cases)"""
    e = fa.Engine("toy", device=-1)
    try:
        q = [int(x) for x in e.q]
    finally:
        e.close()
    deltas = em.delta_chain(q)
    return q, deltas, dm.cases(q, deltas)


def _bits(d):
    return int(np.float64(d).view(np.uint64))


def _ld(x):
    """a non-negative integer below 2^64 as a numpy.longdouble, exactly (two 32-bit halves: no pass through a double)"""
    return np.longdouble(x >> 32) * np.longdouble(4294967296.0) + np.longdouble(x & 0xFFFFFFFF)


def _x87(K, read, ms, es):
    """Client::decrypt_physical's host arithmetic restated in numpy.longdouble"""
    M = 1
    for m in read:
        M *= m
    v = em.centred(K, M)
    mag = abs(v)
    lift = _ld(mag >> 64) * np.longdouble(18446744073709551616.0) + _ld(mag & ((1 << 64) - 1))
    if v < 0:
        lift = -lift
    return np.float64(lift / np.ldexp(_ld(ms), es))


def test_census_reaches_every_edge(toy):
    _, _, cases = toy
    cnt, one_limb_lift = dm.census(cases)
    print(len(cases), "cases:", cnt)
    assert set(cnt) == set(dm.TRACE_ALL)
    short = {k: v for k, v in cnt.items() if v < 4}
    assert not short, short
    assert one_limb_lift == 0                      # the lift rounds with two limbs only


def test_host_build_equals_the_model_and_x87(toy, lift_exe):
    q, _, cases = toy
    lines = []
    for read, K, ms, es in cases:
        two = len(read) == 2
        lines.append("%d %d %d %d %d %d %d\n" % (len(read), read[0], read[1] if two else 0, K % read[0], K % read[1] if two else 0, ms, es))
    r = subprocess.run([lift_exe], input="".join(lines), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    got = [int(w, 16) for w in r.stdout.split()]
    assert len(got) == len(cases)
    want = [dm.case_trace(K, read, ms, es) for read, K, ms, es in cases]
    bad = [(c, hex(g), w[0].hex(), sorted(w[1])) for c, g, w in zip(cases, got, want) if g != _bits(w[0])]
    assert not bad, (len(bad), bad[:4])
    assert _bits(0.0) in got and all(g != _bits(-0.0) for g in got)      # zero is +0.0
    if np.finfo(np.longdouble).nmant != 63:
        pytest.skip("numpy.longdouble is not the x87 format here: the model and the host build agree; the x87 leg is skipped")
    bad = [(c, hex(g)) for c, g in zip(cases, got) if g != _bits(_x87(c[1], c[0], c[2], c[3]))]
    assert not bad, (len(bad), bad[:4])


def test_decrypt_batch_needs_a_device_and_its_arguments(fa):
    lib = fa.load_library()
    assert hasattr(lib, "fhelin_decrypt_batch") and hasattr(lib, "fhelin_ctx_set_device_decode")
    assert hasattr(fa.Engine, "decrypt_batch") and hasattr(fa.Engine, "set_device_decode")
    e = fa.Engine("toy", device=-1)
    try:
        out = np.zeros(16)
        op = out.ctypes.data_as(C.POINTER(C.c_double))
        arr = (C.c_void_p * 2)()                  # null entries
        one = (C.c_void_p * 1)(1)                 # a non-null entry that is never dereferenced: the device check comes first
        idx = (C.c_int32 * 2)(0, 1)
        f = lib.fhelin_decrypt_batch
        assert f(None, arr, 1, 0, 0, None, 0, op, 8) == ERR_ARG
        assert f(e.h, arr, -1, 0, 0, None, 0, op, 8) == ERR_ARG
        assert f(e.h, None, 0, 0, 0, None, 0, None, 8) == 0            # n = 0 touches nothing
        assert f(e.h, None, 1, 0, 0, None, 0, op, 8) == ERR_ARG
        assert f(e.h, one, 1, 0, 0, None, 0, None, 8) == ERR_ARG
        assert f(e.h, arr, 2, 0, 0, None, 0, op, 8) == ERR_ARG         # a null entry
        assert f(e.h, one, 1, 63, 0, None, 0, op, 8) == ERR_ARG
        assert f(e.h, one, 1, -1, 0, None, 0, op, 8) == ERR_ARG
        assert f(e.h, one, 1, 0, 0, idx, 0, op, 8) == ERR_ARG          # an index list without entries
        assert f(e.h, one, 1, 0, 0, (C.c_int32 * 2)(0, 8), 2, op, 8) == ERR_ARG
        assert f(e.h, one, 1, 0, 0, (C.c_int32 * 2)(-1, 0), 2, op, 8) == ERR_ARG
        assert f(e.h, one, 1, 0, 0, idx, 2, op, 8) == ERR_NO_DEVICE
        assert f(e.h, one, 1, 0, 0, None, 0, op, 8) == ERR_NO_DEVICE
        assert np.array_equal(out, np.zeros(16))
        assert lib.fhelin_ctx_set_device_decode(None, 1) == ERR_ARG
        assert lib.fhelin_ctx_set_device_decode(e.h, 1) == 0
        assert lib.fhelin_ctx_set_device_decode(e.h, 0) == 0
    finally:
        e.close()
