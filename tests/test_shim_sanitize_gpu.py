"""include/FHEController.h's sanitised replies: tests/shim/shim_sanitize.cpp, compiled here with the g++ line __graft_entry__.build()
uses, runs as three processes at the reference ring (N=2^15, 16384 slots).  The client writes its keys and two inputs; the server, in a
directory whose keys/ holds no secret-key.txt, rotates, multiplies and calls sanitize(keep = {0..19}, flood_bits = 24); the client
decrypts the reply: the kept slots are the product, every other slot is empty, and the reply file holds two limbs."""
import os
import shutil
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_shim_server_without_the_secret_hands_back_a_sanitised_reply(tmp_path):
    lib_dir = os.path.join(ROOT, "fhe-linformer_amd")
    exe = str(tmp_path / "shim_sanitize")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "shim", "shim_sanitize.cpp"), "-L", lib_dir, "-lfhelin_amd",
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
        for name in ("crypto-context.txt", "rot_rk.txt", "evk.bin", "in.bin"):
            shutil.copy(ck / name, server / "keys" / name)
        assert not (server / "keys" / "secret-key.txt").exists()
        sizes = next(l for l in run("server", server).splitlines() if l.startswith("bytes "))
        print(sizes)
        w = sizes.split()
        raw, reply, limbs, ring = int(w[2]), int(w[4]), int(w[6]), int(w[8])
        assert limbs == 2
        assert reply == os.path.getsize(server / "keys" / "reply.bin")
        assert reply <= 2 * 2 * ring * 8 + 256 and reply < raw      # two components of two limbs and a small header
        shutil.copy(server / "keys" / "reply.bin", ck / "reply.bin")
        line = next(l for l in run("check", client).splitlines() if l.startswith("err "))
        print(line)
        assert float(line.split()[1]) < 1e-3, line
        assert float(line.split()[3]) < 1e-3, line
    finally:
        shutil.rmtree(tmp_path, ignore_errors=True)
