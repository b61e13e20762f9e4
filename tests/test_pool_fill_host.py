"""FHELIN_POOL_FILL (csrc/pool.cpp, DESIGN.md "Pool fill") without a GPU.

The knob makes the device pool hand out every block with one word w in each of its 32-bit words, so that a result which depends on memory
nobody wrote depends on w (tests/test_stale_memory_gpu.py).  Here the knob itself is tested, on host memory: the pool's backend is host
malloc and the fill writes host memory (fhelin_debug_pool_fill_selftest / pool_fill_selftest).  The self-test fails unless, at every
hand-out, every word of the ROUNDED block is w, every other live block still holds its own marker (checked word for word on both address
neighbours at each hand-out, on the block itself when it is freed, and on all live blocks every 64th operation), and with w = 0 nothing
is written anywhere.  The same code is tests/shim/pool_fill_host.cpp as a stand-alone program, which is the form to build with
-fsanitize=address,undefined (the command is in that file); this module builds and runs it without sanitizers."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = 1
KNOB = "FHELIN_POOL_FILL"


def _selftest(lib, seed, n_ops, w):
    out = np.zeros(6, dtype=np.uint64)
    rc = lib.fhelin_debug_pool_fill_selftest(seed, n_ops, w, out.ctypes.data_as(C.POINTER(C.c_uint64)), 6)
    assert rc == 0, lib.fhelin_last_error()
    return [int(v) for v in out]


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_every_handed_out_word_is_w_and_no_other_block_changes(fa, seed):
    lib = fa.load_library()
    off = _selftest(lib, seed, 1500, 0)
    blocks, rounded, filled_blocks, filled_bytes, slabs, big = off
    assert (filled_blocks, filled_bytes) == (0, 0)                 # off: no fill ran (the self-test also checks that no byte changed)
    assert slabs >= 2 and big >= 50 and blocks - big >= 50         # growth past one slab; both granule classes
    for w in (1, 2, 4095):
        on = _selftest(lib, seed, 1500, w)
        assert on[:2] == off[:2] and on[4:] == off[4:]             # the same sequence, whatever w
        assert on[2] == blocks and on[3] == rounded                # the counters: every block, the sum of the ROUNDED sizes
        assert rounded % 256 == 0


def test_selftest_refuses_a_word_above_the_cap(fa):
    lib = fa.load_library()
    out = np.zeros(6, dtype=np.uint64)
    assert lib.fhelin_debug_pool_fill_selftest(1, 10, 4096, out.ctypes.data_as(C.POINTER(C.c_uint64)), 6) == ERR_ARG
    assert lib.fhelin_debug_pool_fill_selftest(1, 10, 1, out.ctypes.data_as(C.POINTER(C.c_uint64)), 5) == ERR_ARG


@pytest.fixture
def knob():
    """set / unset the variable for one context creation, and put back what was there"""
    saved = os.environ.get(KNOB)

    def put(v):
        if v is None:
            os.environ.pop(KNOB, None)
        else:
            os.environ[KNOB] = v
    yield put
    put(saved)


@pytest.mark.parametrize("text", ["4096", "4294967295", "0xFFFFFFFF", "-1", "one", "7x", " 7", "99999999999999999999999"])
def test_context_creation_refuses_a_bad_word(fa, knob, text):
    """the pool's knob is read before the host-only return of the Context's constructor: a host-only context refuses it too"""
    knob(text)
    with pytest.raises(fa.FhelinError) as ei:
        fa.Engine("toy", device=-1)
    assert ei.value.code == ERR_ARG and KNOB in str(ei.value)


@pytest.mark.parametrize("text", [None, "", "0", "1", "2", "4095"])
def test_context_creation_accepts_the_range(fa, knob, text):
    knob(text)
    e = fa.Engine("toy", device=-1)
    try:
        assert e.pool_fill_stats() == (0, 0)                        # nothing is allocated without a device
        b = C.c_uint64()
        assert e.lib.fhelin_debug_pool_fill_stats(None, C.byref(b), C.byref(b)) == ERR_ARG
        assert e.lib.fhelin_debug_pool_fill_stats(e.h, None, C.byref(b)) == ERR_ARG
    finally:
        e.close()


def test_stand_alone_program(tmp_path):
    """tests/shim/pool_fill_host.cpp + csrc/pool.cpp alone (its HIP entry points abort: the host path never reaches the runtime):
    the self-test at w = 0, 1, 2, 4095 over three seeds, and the knob's parser on every accepted and refused text"""
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    exe = str(tmp_path / "pool_fill_host")
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(rocm, "include"),
                        os.path.join(ROOT, "tests", "shim", "pool_fill_host.cpp"), os.path.join(ROOT, "fhe-linformer_amd", "csrc", "pool.cpp"),
                        "-o", exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe, "600"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    lines = r.stdout.strip().split("\n")
    assert lines[-1] == "pool_fill_host: all ok" and len(lines) == 13 and all(ln.startswith("ok ") for ln in lines[:-1])
