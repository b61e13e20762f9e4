"""include/FHEController.h's seeded evaluation keys: tests/shim/shim_seeded_keys.cpp, compiled here with the g++ line
__graft_entry__.build() uses, runs as three processes at the reference ring (N=2^15, 16384 slots).  The client makes its keys in
seeded-key mode and writes the compact evaluation-key set; the server, in a directory whose keys/ holds no secret-key.txt and no
full set, loads the compact one, bootstraps, rotates and multiplies, and cannot decrypt; the server's saved result equals the
client's own computation of the same steps byte for byte, and the client decrypts it."""
import os
import shutil
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_shim_server_from_a_compact_key_set(tmp_path):
    lib_dir = os.path.join(ROOT, "fhe-linformer_amd")
    exe = str(tmp_path / "shim_seeded_keys")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "shim", "shim_seeded_keys.cpp"), "-L", lib_dir, "-lfhelin_amd",
                           "-Wl,-rpath," + lib_dir, "-o", exe])
    env = dict(os.environ, LD_LIBRARY_PATH=lib_dir + ":" + os.environ.get("LD_LIBRARY_PATH", ""))
    for k in ("FHELIN_LEVEL_PLAN", "FHELIN_PRESET", "FHELIN_SEED"):
        env.pop(k, None)
    client, server = tmp_path / "client", tmp_path / "server"
    for d in (client / "run", client / "keys", server / "run", server / "keys"):
        d.mkdir(parents=True)

    def run(mode, where):
        r = subprocess.run([exe, mode], env=env, capture_output=True, text=True, timeout=900, cwd=str(where / "run"))
        assert r.returncode == 0, (mode, r.stdout[-2000:] + r.stderr[-2000:])
        return r.stdout

    try:
        run("client", client)
        ck = client / "keys"
        full, cmp_ = (ck / "evk.bin").stat().st_size, (ck / "evk.cmp").stat().st_size
        print(f"compact set {cmp_ / 1e9:.3f} GB, full set {full / 1e9:.3f} GB")
        assert 0.49 < cmp_ / full < 0.51
        for name in ("crypto-context.txt", "rot_rk.txt", "evk.cmp", "in.bin"):
            shutil.copy(ck / name, server / "keys" / name)
        assert not (server / "keys" / "secret-key.txt").exists()
        out = run("server", server)
        assert "decrypt refused" in out, out[-2000:]
        got = (server / "keys" / "out.bin").read_bytes()
        assert got == (ck / "own.bin").read_bytes()
        shutil.copy(server / "keys" / "out.bin", ck / "out.bin")
        line = next(l for l in run("check", client).splitlines() if l.startswith("err "))
        print(line)
        assert float(line.split()[1]) < 1e-3, line
    finally:
        shutil.rmtree(tmp_path, ignore_errors=True)
