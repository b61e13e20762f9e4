"""CPU-side checks of the iterative bootstrap's interface (include/fhelin.h fhelin_bootstrap_iter*): the library exports the three
entry points with the signatures capi.py declares, and the shims offer EvalBootstrap(c, 2, precision).  A device-less context
cannot hold a ciphertext, so the range check on the precision runs in tests/test_bootstrap_iter_gpu.py."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {
    "fhelin_bootstrap_iter": 4,          # ctx, ct, precision, out
    "fhelin_bootstrap_iter_batch": 5,    # ctx, cts, n, precision, outs
    "fhelin_bootstrap_iter_drop": 5,     # ctx, ct, precision, drop, out
}


def test_library_exports_and_capi_declares_bootstrap_iter(fa):
    lib = fa.load_library()
    header = open(os.path.join(ROOT, "include", "fhelin.h")).read()
    for name, nargs in NEW.items():
        assert hasattr(lib, name), f"libfhelin_amd.so does not export {name}"
        assert f"int {name}(" in header
        fn = getattr(lib, name)
        assert fn.restype is C.c_int32 and fn.argtypes is not None and len(fn.argtypes) == nargs, name
    for meth in ("bootstrap_iter", "bootstrap_iter_batch", "bootstrap_iter_drop"):
        assert callable(getattr(fa.Engine, meth))


def test_controllers_take_a_precision(fa):
    import inspect
    from fhe_linformer_amd import linformer as lf
    for cls in (lf.GpuController, lf.BatchedController):
        sig = inspect.signature(cls.bootstrap)
        assert "precision" in sig.parameters and sig.parameters["precision"].default is None, cls


def test_shim_bootstrap_with_precision_compiles_and_links(tmp_path):
    """the driver of tests/test_shim_bootstrap_iter_gpu.py, with the g++ line __graft_entry__.build() uses for the shim drivers;
    FHEControllerBatch's bootstrap(batch, precision) overload next to it"""
    lib_dir = os.path.join(ROOT, "fhe-linformer_amd")
    exe = str(tmp_path / "shim_bootstrap_iter")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "shim", "shim_bootstrap_iter.cpp"), "-L", lib_dir, "-lfhelin_amd",
                           "-Wl,-rpath," + lib_dir, "-o", exe])
    assert os.path.exists(exe)
    src = tmp_path / "batch.cpp"
    src.write_text('#include "FHEControllerBatch.h"\n'
                   "CtxtBatch f(FHEControllerBatch& b, const CtxtBatch& x) { return b.bootstrap(x, 12, false); }\n"
                   "CtxtBatch g(FHEControllerBatch& b, const CtxtBatch& x) { return b.bootstrap(x, true); }\n")
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])
