"""Host-side checks that go with tests/test_dot_kernels_gpu.py.

ew_dot_kernel and ew_dot_groups_kernel sum up to 32 products of residues below 2^60 in an Acc128 and reduce once; the cyclic and window
kernels reduce running sums whose high word is not below q either.  All of them rest on barrett_reduce128 (csrc/modarith.h) taking ANY
128-bit value, hi >= q included, as its comment claims.  The function is host/device code (FHE_HD): here it is compiled for the host
into a small stand-alone program and compared with Python integers at the edges of both words."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M64 = (1 << 64) - 1
ERR_ARG, ERR_NO_DEVICE = 1, 2


@pytest.fixture(scope="module")
def barrett_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("barrett") / "barrett_host")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", os.path.join(ROOT, "tests", "shim", "barrett_host.cpp"), "-o", exe])
    return exe


def _prime(orc, bits, k=0):
    """the k-th prime below 2^bits"""
    m = (1 << bits) - 1
    while True:
        if orc.is_prime(m):
            if k == 0:
                return m
            k -= 1
        m -= 2


@pytest.mark.parametrize("bits", [24, 53, 60])
def test_barrett_reduce128_takes_any_128_bit_value(orc, barrett_exe, bits):
    q = _prime(orc, bits)
    assert q.bit_length() == bits
    rng = np.random.default_rng(bits)
    rand = [int(v) for v in rng.integers(0, 1 << 63, size=24, dtype=np.uint64)] + [int(v) | (1 << 63) for v in
                                                                                   rng.integers(0, 1 << 63, size=24, dtype=np.uint64)]
    his = [0, q - 1, q, M64] + rand[:8]
    los = [0, M64] + rand[8:]
    # the largest sum the 32-term kernels form: 32 (q - 1)^2, and the value one below a multiple of q that is nearest 2^128
    extra = [32 * (q - 1) ** 2, ((1 << 128) // q) * q - 1, ((1 << 128) // q) * q, (1 << 128) - 1]
    cases = [(lo, hi) for hi in his for lo in los] + [(v & M64, v >> 64) for v in extra]
    assert all(hi <= M64 and lo <= M64 for lo, hi in cases)
    text = "".join(f"{q} {lo} {hi}\n" for lo, hi in cases)
    r = subprocess.run([barrett_exe], input=text, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    got = [int(v) for v in r.stdout.split()]
    want = [((hi << 64) | lo) % q for lo, hi in cases]
    assert len(got) == len(want)
    bad = [(c, g, w) for c, g, w in zip(cases, got, want) if g != w]
    assert not bad, bad[:4]


def test_debug_dot_entry_points_need_a_device_and_their_arguments(fa):
    lib = fa.load_library()
    for name in ("debug_pt_from_residues", "debug_dot_plain", "debug_dot_groups", "debug_dot_cyclic", "debug_dot_window"):
        assert hasattr(lib, "fhelin_" + name) and hasattr(fa.Engine, name), name
    e = fa.Engine("toy", device=-1)
    try:
        words = np.zeros((1, e.N), dtype=np.uint64)
        wp = words.ctypes.data_as(C.c_void_p)
        h = C.c_void_p()
        outs = (C.c_void_p * 32)()
        arr = (C.c_void_p * 32)()
        assert lib.fhelin_debug_pt_from_residues(e.h, wp, 1, C.byref(h)) == ERR_NO_DEVICE
        assert lib.fhelin_debug_pt_from_residues(None, wp, 1, C.byref(h)) == ERR_ARG
        assert lib.fhelin_debug_pt_from_residues(e.h, None, 1, C.byref(h)) == ERR_ARG
        assert lib.fhelin_debug_pt_from_residues(e.h, wp, 1, None) == ERR_ARG
        assert lib.fhelin_debug_dot_plain(e.h, None, arr, 1, C.byref(h)) == ERR_ARG
        assert lib.fhelin_debug_dot_plain(e.h, arr, arr, 0, C.byref(h)) == ERR_ARG
        assert lib.fhelin_debug_dot_groups(e.h, arr, 1, 17, arr, 1, outs) == ERR_ARG
        assert lib.fhelin_debug_dot_groups(e.h, arr, 1, 1, arr, 9, outs) == ERR_ARG
        assert lib.fhelin_debug_dot_cyclic(e.h, arr, 33, arr, outs) == ERR_ARG
        assert lib.fhelin_debug_dot_cyclic(e.h, arr, 1, arr, outs) == ERR_ARG          # a null ciphertext in the array
        assert lib.fhelin_debug_dot_window(e.h, arr, arr, arr, None, 0) == ERR_ARG
        assert lib.fhelin_debug_dot_window(e.h, arr, arr, arr, arr, 0) == ERR_ARG      # a null destination
    finally:
        e.close()


def test_debug_rotate_many_batch_checks_its_arguments(fa):
    lib = fa.load_library()
    assert hasattr(lib, "fhelin_debug_rotate_many_batch") and hasattr(fa.Engine, "debug_rotate_many_batch")
    e = fa.Engine("toy", device=-1)
    try:
        outs = (C.c_void_p * 4)()
        arr = (C.c_void_p * 2)()
        idx = (C.c_int32 * 2)(1, 2)
        assert lib.fhelin_debug_rotate_many_batch(None, arr, 2, idx, 2, outs) == ERR_ARG
        assert lib.fhelin_debug_rotate_many_batch(e.h, None, 2, idx, 2, outs) == ERR_ARG
        assert lib.fhelin_debug_rotate_many_batch(e.h, arr, 2, None, 2, outs) == ERR_ARG
        assert lib.fhelin_debug_rotate_many_batch(e.h, arr, 2, idx, 2, None) == ERR_ARG
        assert lib.fhelin_debug_rotate_many_batch(e.h, arr, 0, idx, 2, outs) == ERR_ARG
        assert lib.fhelin_debug_rotate_many_batch(e.h, arr, 2, idx, 0, outs) == ERR_ARG
        assert lib.fhelin_debug_rotate_many_batch(e.h, arr, 2, idx, 2, outs) == ERR_ARG          # a null ciphertext in the array
        assert not any(outs)
    finally:
        e.close()
