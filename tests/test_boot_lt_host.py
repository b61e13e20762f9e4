"""CPU-side checks of the bootstrap's linear-stage knob (include/fhelin.h "Bootstrap linear stages"): the library exports the entry points
with the signatures capi.py declares, the knob is off unless somebody turns it on, the environment variables are honoured, a bad n1 is
refused without a device, and the probe says "not measured" where there is no GPU.  Everything that needs a ciphertext runs in
tests/test_boot_lt_gpu.py."""
import ctypes as C
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = 1
NEW = {
    "fhelin_ctx_set_bootstrap_lt": 3,    # ctx, on, n1
    "fhelin_ctx_bootstrap_lt": 3,        # ctx, on*, n1*
    "fhelin_lt_encoding_bytes": 2,       # plan, bytes*
}


def test_library_exports_and_capi_declares_the_entries(fa):
    lib = fa.load_library()
    header = open(os.path.join(ROOT, "include", "fhelin.h")).read()
    for name, nargs in NEW.items():
        assert hasattr(lib, name), f"libfhelin_amd.so does not export {name}"
        assert f"int {name}(" in header
        fn = getattr(lib, name)
        assert fn.restype is C.c_int32 and fn.argtypes is not None and len(fn.argtypes) == nargs, name
    for meth in ("set_bootstrap_lt", "bootstrap_lt"):
        assert callable(getattr(fa.Engine, meth))
    from fhe_linformer_amd import capi
    assert callable(capi.LinearTransform.encoding_bytes)


def test_defaults_environment_and_refusals_without_a_device(fa, monkeypatch):
    monkeypatch.delenv("FHELIN_BOOT_LT", raising=False)
    monkeypatch.delenv("FHELIN_BOOT_LT_N1", raising=False)
    lib = fa.load_library()
    e = fa.Engine("toy", device=-1)
    try:
        assert e.bootstrap_lt() == (False, 0)
        on, n1 = C.c_int32(), C.c_int32()
        assert lib.fhelin_ctx_set_bootstrap_lt(None, 1, 0) == ERR_ARG
        assert lib.fhelin_ctx_bootstrap_lt(e.h, None, C.byref(n1)) == ERR_ARG
        assert lib.fhelin_ctx_bootstrap_lt(e.h, C.byref(on), None) == ERR_ARG
        assert lib.fhelin_lt_encoding_bytes(None, None) == ERR_ARG
        for bad in (-1, 33, 1 << 20):
            with pytest.raises(fa.FhelinError) as ei:
                e.set_bootstrap_lt(True, bad)
            assert ei.value.code == ERR_ARG
            assert e.bootstrap_lt() == (False, 0)                 # a refused call changes nothing
        for on_, n1_ in ((True, 0), (True, 1), (True, 32), (False, 7), (False, 0)):
            e.set_bootstrap_lt(on_, n1_)
            assert e.bootstrap_lt() == (on_, n1_)
    finally:
        e.close()
    for env, want in (({"FHELIN_BOOT_LT": "1"}, (True, 0)), ({"FHELIN_BOOT_LT": "1", "FHELIN_BOOT_LT_N1": "16"}, (True, 16)),
                      ({"FHELIN_BOOT_LT": "0", "FHELIN_BOOT_LT_N1": "4"}, (False, 4)), ({"FHELIN_BOOT_LT": "1", "FHELIN_BOOT_LT_N1": "99"}, (True, 0))):
        for k in ("FHELIN_BOOT_LT", "FHELIN_BOOT_LT_N1"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        e = fa.Engine("toy", device=-1)
        try:
            assert e.bootstrap_lt() == want, env
        finally:
            e.close()


def test_controllers_take_the_knob(fa):
    import inspect
    from fhe_linformer_amd import linformer as lf
    for cls in (lf.GpuController, lf.BatchedController, lf.LanedBatchedController):
        p = inspect.signature(cls.__init__).parameters
        assert "bootstrap_lt" in p and p["bootstrap_lt"].default is False, cls


def test_probe_says_not_measured_without_a_gpu(tmp_path):
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    out = tmp_path / "probe.json"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "boot_lt_probe.py"), "--out", str(out)], env=env, capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert "not measured" in r.stdout
    assert not out.exists()
