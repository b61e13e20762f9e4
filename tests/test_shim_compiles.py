"""The C++ drivers of the FHEController shim compile against include/FHEController.h and link against libfhelin_amd.so
(drop-in boundary): this repo's own drivers (tests/shim/*.cpp), and the reference's main.cpp / main_2.cpp
as build() links them unchanged into oracle/_ref/ wherever the reference tree is present (oracle/Makefile `ref`)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_shim_driver_builds():
    out = os.path.join(ROOT, "tests", "shim", "shim_driver")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "shim", "shim_driver.cpp"),
                        "-L", os.path.join(ROOT, "fhe-linformer_amd"), "-lfhelin_amd", "-Wl,-rpath,$ORIGIN/../../fhe-linformer_amd",
                        "-o", out + ".tmp"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    os.replace(out + ".tmp", out)      # atomically: a snapshot of the tree taken meanwhile never sees a half-written binary
    assert os.path.exists(out)


@pytest.mark.parametrize("driver", ["main.cpp", "main_2.cpp"])
def test_reference_driver_links_and_starts(driver):
    """the reference's drivers, linked unchanged against the shim + libfhelin_amd.so by build() (oracle/_ref/), start (usage
    text, exit 0: no GPU touched) and reach the engine through the C ABI only"""
    exe = os.path.join(ROOT, "oracle", "_ref", "ref_" + driver[:-4])
    if not os.path.exists(exe):
        pytest.skip("oracle/_ref/ not built: build() links it only where the reference tree is present")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60, cwd=os.path.join(ROOT, "oracle", "_ref"))
    assert r.returncode == 0 and "FHE-Linformer" in r.stdout
    syms = subprocess.run(["nm", "-D", "--undefined-only", exe], capture_output=True, text=True).stdout
    assert "fhelin_bootstrap" in syms and "fhelin_fc_matmulRElarge" in syms     # the engine is reached through the C ABI only


def test_shim_forward_builds():
    out = os.path.join(ROOT, "tests", "shim", "shim_forward")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "shim", "shim_forward.cpp"),
                        "-L", os.path.join(ROOT, "fhe-linformer_amd"), "-lfhelin_amd", "-Wl,-rpath,$ORIGIN/../../fhe-linformer_amd",
                        "-o", out + ".tmp"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    os.replace(out + ".tmp", out)      # atomically: a snapshot of the tree taken meanwhile never sees a half-written binary
