#!/usr/bin/env python3
"""Device transport at the scale of the row gather: N=2^16, 28+7 limbs, 130 rows at 12 limbs, on ONE GPU.
Three ways of moving the rows through a device buffer and back into handles alternate in one process, --reps rounds each:
  old     the path before the device transport: one fhelin_ct_export_device per row into a tensor of its own (a host
          synchronisation each), a zero-filled (rows, size) buffer filled row by row, torch's stream synchronised, one
          fhelin_ct_import_device per row (a host synchronisation each);
  raw     fhelin_ct_export_device_many into the (rows, stride) buffer and fhelin_ct_import_device_many out of it, 64-bit words;
  packed  the same with every residue at its modulus width.
Per way: wall ms (the device idle before and after), device-event ms on torch's stream, the context's host synchronisations, the bytes
a collective would put on the wire, and whether the imported residues equal the exported ones.  No collective runs and no link is
involved: this measures the two ends of the gather, not the gather.  --nccl-world1 adds ONE run of shard._all_gather_indexed over a
world-size-1 nccl process group (FileStore in a temporary directory) in a child process under --nccl-timeout; a failure to initialise
is recorded, not retried.  It prints what it measures; --json writes the record.  Without a GPU it prints "not measured" and exits 0.
  python tools/transport_probe.py [--reps 5] [--rows 130] [--ell 12] [--json profiles/transport_probe_n16.json] [--nccl-world1]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KW = dict(n_q=28, n_p=7)


def make_rows(eng, rows, ell, distinct=13):
    """`rows` handles at `ell` limbs: `distinct` different random residue sets, repeated"""
    rng = np.random.default_rng(71)
    limbs = [np.stack([np.stack([rng.integers(0, int(q), eng.N, dtype=np.uint64) for q in eng.q[:ell]]) for _ in range(2)])
             for _ in range(min(distinct, rows))]
    n = 1 << eng.params.log_slots
    return [eng.ct_import(limbs[i % len(limbs)], slots=n) for i in range(rows)], limbs


def old_path(torch, transport, cts):
    """what shard._all_gather_indexed did on the device before pack_many: returns (handles, bytes on the wire)"""
    packed = [transport.pack(c) for c in cts]
    size = max(int(p.numel()) for p, _ in packed)
    buf = torch.zeros((len(cts), size), dtype=torch.uint8, device="cuda")
    for k, (p, _) in enumerate(packed):
        buf[k, : p.numel()] = p
    torch.cuda.current_stream().synchronize()
    return [transport.unpack(buf[k], m) for k, (_, m) in enumerate(packed)], buf.numel()


def new_path(torch, transport, cts):
    buf = torch.empty((len(cts), transport.frame_stride(cts)), dtype=torch.uint8, device="cuda")
    _, meta = transport.pack_many(cts, out=buf)
    return transport.unpack_many(buf, meta), buf.numel()


def same_bytes(got, limbs):
    return all(np.array_equal(g.export(), limbs[i % len(limbs)]) for i, g in enumerate(got))


def nccl_child(a):
    """one _all_gather_indexed over a world of one nccl rank; prints one JSON line"""
    import torch
    import torch.distributed as dist
    import fhe_linformer_amd as fa
    from fhe_linformer_amd import shard
    rec = {"ran": False}
    with tempfile.TemporaryDirectory() as d:
        try:
            dist.init_process_group("nccl", store=dist.FileStore(os.path.join(d, "store"), 1), rank=0, world_size=1)
        except Exception as ex:                                   # recorded, not retried
            rec["error"] = f"{type(ex).__name__}: {ex}"[:600]
            print(json.dumps(rec))
            return 0
        try:
            eng = fa.Engine("bench", seed=1, **KW)
            cts, limbs = make_rows(eng, a.nccl_rows, a.ell, distinct=a.nccl_rows)
            for packed in (True, False):
                transport = shard.EngineTransport(eng, device=True, packed=packed)
                before = eng.sync_count()
                t0 = time.perf_counter()
                got = shard._all_gather_indexed(dist, transport, dict(enumerate(cts)), [list(range(len(cts)))])
                torch.cuda.synchronize()
                rec["packed" if packed else "raw"] = dict(wall_ms=1e3 * (time.perf_counter() - t0), host_syncs=eng.sync_count() - before,
                                                         bytes_equal=same_bytes([got[i] for i in range(len(cts))], limbs))
            rec.update(ran=True, rows=len(cts), ell=a.ell)
            eng.close()
        except Exception as ex:
            rec["error"] = f"{type(ex).__name__}: {ex}"[:600]
        finally:
            dist.destroy_process_group()
    print(json.dumps(rec))
    return 0


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rows", type=int, default=130)
    ap.add_argument("--ell", type=int, default=12)
    ap.add_argument("--json", default="")
    ap.add_argument("--nccl-world1", action="store_true")
    ap.add_argument("--nccl-rows", type=int, default=10)
    ap.add_argument("--nccl-timeout", type=int, default=240)
    ap.add_argument("--nccl-child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    import fhe_linformer_amd as fa
    try:
        import torch
        has_dev = torch.cuda.is_available()
    except Exception as ex:
        has_dev = False
        print(f"no device: {ex}")
    if not has_dev:
        print("not measured: no GPU")
        return 0
    if a.nccl_child:
        return nccl_child(a)
    from fhe_linformer_amd import shard
    eng = fa.Engine("bench", seed=1, **KW)
    cts, limbs = make_rows(eng, a.rows, a.ell)
    ways = {"old": (old_path, shard.EngineTransport(eng, device=True, packed=False)),
            "raw": (new_path, shard.EngineTransport(eng, device=True, packed=False)),
            "packed": (new_path, shard.EngineTransport(eng, device=True, packed=True))}
    rec = {name: dict(wall_ms=[], event_ms=[], host_syncs=[], wire_bytes=0, bytes_equal=None) for name in ways}
    for rep in range(-1, a.reps):                                 # one untimed round first
        print(f"round {rep + 1} of {a.reps + 1}", flush=True)
        for name, (fn, transport) in ways.items():
            torch.cuda.synchronize()
            eng.sync()
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            before = eng.sync_count()
            t0 = time.perf_counter()
            start.record()
            got, wire = fn(torch, transport, cts)
            stop.record()
            syncs = eng.sync_count() - before                     # before the closing synchronisation below, which is the probe's
            torch.cuda.synchronize()
            eng.sync()
            wall = 1e3 * (time.perf_counter() - t0)
            r = rec[name]
            if rep < 0:
                r["bytes_equal"] = same_bytes(got, limbs)
                r["wire_bytes"] = wire
            else:
                r["wall_ms"].append(wall)
                r["event_ms"].append(start.elapsed_time(stop))
                r["host_syncs"].append(syncs)
            del got
    out = dict(shape=dict(log_n=eng.log_n, n_q=eng.n_q, n_p=eng.n_p, rows=a.rows, ell=a.ell), reps=a.reps,
               note="one GPU, no collective and no link: the two ends of the row gather only; no multi-GPU scaling is measured")
    for name, r in rec.items():
        out[name] = dict(wall_ms_median=statistics.median(r["wall_ms"]), wall_ms=r["wall_ms"], event_ms_median=statistics.median(r["event_ms"]),
                         event_ms=r["event_ms"], host_syncs=r["host_syncs"][0], host_syncs_all_equal=len(set(r["host_syncs"])) == 1,
                         wire_bytes=r["wire_bytes"], bytes_equal=r["bytes_equal"])
        print(f"{name:7s} wall {out[name]['wall_ms_median']:9.2f} ms   events {out[name]['event_ms_median']:9.2f} ms   host syncs "
              f"{out[name]['host_syncs']:4d}   wire {r['wire_bytes'] / 2 ** 20:9.1f} MiB   bytes equal {r['bytes_equal']}")
    eng.close()
    if a.nccl_world1:
        cmd = [sys.executable, os.path.abspath(__file__), "--nccl-child", "--nccl-rows", str(a.nccl_rows), "--ell", str(a.ell)]
        try:
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=a.nccl_timeout)
            lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
            out["nccl_world1"] = json.loads(lines[-1]) if lines else dict(ran=False, error=f"exit {p.returncode}: {p.stderr[-600:]}")
        except subprocess.TimeoutExpired:
            out["nccl_world1"] = dict(ran=False, error=f"no result within {a.nccl_timeout} s")
        print("nccl world of one:", json.dumps(out["nccl_world1"]))
    else:
        out["nccl_world1"] = dict(ran=False, error="not asked for")
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
