"""CPU-side checks of paired bootstrapping's interface (include/fhelin.h "Paired bootstrapping"): the library exports the entry points with
the signatures capi.py declares, NULL arguments are FHELIN_ERR_ARG, and the runtime knob is off unless somebody turns it on.  Everything
that needs a ciphertext runs in tests/test_boot_pair_gpu.py."""
import ctypes as C
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = 1
NEW = {
    "fhelin_bootstrap_pair": 5,              # ctx, a, b, out_a, out_b
    "fhelin_bootstrap_paired_batch": 4,      # ctx, cts, n, outs
    "fhelin_bootstrap_pair_drop": 6,         # ctx, a, b, drop, out_a, out_b
    "fhelin_bootstrap_pair_partial": 5,      # ctx, a, b, stage, out
    "fhelin_ctx_set_bootstrap_pairing": 2,   # ctx, on
    "fhelin_ctx_bootstrap_pairing": 2,       # ctx, on*
    "fhelin_debug_pair_pack": 7,             # ctx, a[], b[], k0_a[], k0_b[], n, outs
    "fhelin_debug_pair_split": 6,            # ctx, w[], wc[], n, out_a[], out_b[]
}


def test_library_exports_and_capi_declares_the_pair_entries(fa):
    lib = fa.load_library()
    header = open(os.path.join(ROOT, "include", "fhelin.h")).read()
    for name, nargs in NEW.items():
        assert hasattr(lib, name), f"libfhelin_amd.so does not export {name}"
        assert f"int {name}(" in header
        fn = getattr(lib, name)
        assert fn.restype is C.c_int32 and fn.argtypes is not None and len(fn.argtypes) == nargs, name
    for meth in ("bootstrap_pair", "bootstrap_paired_batch", "bootstrap_pair_drop", "bootstrap_pair_partial", "set_bootstrap_pairing",
                 "bootstrap_pairing", "debug_pair_pack", "debug_pair_split"):
        assert callable(getattr(fa.Engine, meth))


def test_null_arguments_are_refused_and_the_knob_defaults_to_off(fa, monkeypatch):
    monkeypatch.delenv("FHELIN_BOOT_PAIRS", raising=False)
    lib = fa.load_library()
    e = fa.Engine("toy", device=-1)
    try:
        h, null = e.h, None
        out = C.c_void_p()
        outs = (C.c_void_p * 2)()
        assert lib.fhelin_bootstrap_pair(h, null, null, C.byref(out), C.byref(out)) == ERR_ARG
        assert lib.fhelin_bootstrap_pair(null, null, null, None, None) == ERR_ARG
        assert lib.fhelin_bootstrap_paired_batch(h, None, 2, outs) == ERR_ARG
        assert lib.fhelin_bootstrap_paired_batch(null, None, 0, None) == ERR_ARG
        assert lib.fhelin_bootstrap_pair_drop(h, null, null, 0, C.byref(out), C.byref(out)) == ERR_ARG
        assert lib.fhelin_bootstrap_pair_partial(h, null, null, 1, C.byref(out)) == ERR_ARG
        assert lib.fhelin_debug_pair_pack(h, None, None, None, None, 1, outs) == ERR_ARG
        assert lib.fhelin_debug_pair_split(h, None, None, 1, outs, outs) == ERR_ARG
        assert lib.fhelin_ctx_set_bootstrap_pairing(null, 1) == ERR_ARG
        assert lib.fhelin_ctx_bootstrap_pairing(h, None) == ERR_ARG
        assert e.bootstrap_pairing() is False
        e.set_bootstrap_pairing(True)
        assert e.bootstrap_pairing() is True
        e.set_bootstrap_pairing(False)
        assert e.bootstrap_pairing() is False
    finally:
        e.close()
    monkeypatch.setenv("FHELIN_BOOT_PAIRS", "1")
    e = fa.Engine("toy", device=-1)
    try:
        assert e.bootstrap_pairing() is True
    finally:
        e.close()


def test_controllers_take_pair_bootstraps(fa):
    import inspect
    from fhe_linformer_amd import linformer as lf
    for cls in (lf.GpuController, lf.BatchedController, lf.LanedBatchedController):
        p = inspect.signature(cls.__init__).parameters
        assert "pair_bootstraps" in p and p["pair_bootstraps"].default is False, cls
