"""include/FHEController.h's bootstrap(c, precision) is the reference's EvalBootstrap(c, 2, precision) (src/FHEController.cpp:454-469):
tests/shim/shim_bootstrap_iter.cpp, compiled with the g++ line __graft_entry__.build() uses, bootstraps one encrypted vector at
N=2^15 / 16384 slots once and iteratively (precision 12).  The second is at least 2^8 times more precise and has one limb fewer."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_shim_bootstrap_with_precision(tmp_path):
    lib_dir = os.path.join(ROOT, "fhe-linformer_amd")
    exe = str(tmp_path / "shim_bootstrap_iter")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "shim", "shim_bootstrap_iter.cpp"), "-L", lib_dir, "-lfhelin_amd",
                           "-Wl,-rpath," + lib_dir, "-o", exe])
    env = dict(os.environ, LD_LIBRARY_PATH=lib_dir + ":" + os.environ.get("LD_LIBRARY_PATH", ""))
    env.pop("FHELIN_LEVEL_PLAN", None)
    r = subprocess.run([exe, "12"], env=env, capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "Double Bootstrapping 16384 slots" in r.stdout
    line = next(l for l in r.stdout.splitlines() if l.startswith("single_err"))
    f = line.split()
    v = dict(zip(f[0::2], f[1::2]))
    e1, e2 = float(v["single_err"]), float(v["iter_err"])
    print(line)
    assert e2 * 2 ** 8 <= e1, line
    assert int(v["iter_level"]) == int(v["single_level"]) + 1, line
