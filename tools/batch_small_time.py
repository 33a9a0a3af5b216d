#!/usr/bin/env python3
"""Batches of one-workgroup instances against the same handles driven one after another.

K identical-shape members (the 8 x 8 assignment problem, float and double), K in 1, 16, 64, 256, 1024; 1000 iterations per run after
3 warm-up calls.  For each K:
  batch   bddmma_batch_iterations: hipEvents on the batch's stream from its first launch to its last (bddmma_batch_time_iterations), and
          the host's wall clock around the whole call up to the members' synchronisation — the difference is the ordering mechanism
          (two event calls per member on entry, one on exit) and the launch path
  serial  the same K handles driven one after another by bddmma_iterations, one synchronisation at the end (wall clock)
Writes profiles/batch_small_time.txt (or --out).  Usage: python3 tools/batch_small_time.py [--out FILE] [--iters 1000] [--ks 1,16,64,256,1024]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bdd_amd import to_bdd_collection  # noqa: E402
from bdd_amd.instances import assignment_ilp  # noqa: E402
from bdd_amd.solver import bdd_hip_batch, bdd_hip_parallel_mma  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_small_time.txt"))
    ap.add_argument("--iters", type=int, default=1000)
    ap.add_argument("--ks", default="1,16,64,256,1024")
    a = ap.parse_args()
    ks = [int(k) for k in a.ks.split(",")]
    ilp = assignment_ilp(8)
    col = to_bdd_collection(ilp)
    lines = [f"# tools/batch_small_time.py --iters {a.iters} --ks {a.ks}",
             f"# 8 x 8 assignment problem, {a.iters} iterations per run after 3 warm-up calls; times in ms",
             "# batch_dev: hipEvents on the batch stream, first launch to last; batch_wall / serial_wall: host clock, call to synchronised",
             f"{'precision':9s} {'K':>5s} {'batch_dev':>10s} {'batch_wall':>11s} {'serial_wall':>12s} {'serial/batch':>13s} {'batch_dev/K=1':>14s}"]
    for precision in ("float", "double"):
        solvers = [bdd_hip_parallel_mma(col, ilp.objective, precision=precision) for _ in range(max(ks))]
        assert solvers[0].fused_small()
        dev1 = None
        for k in ks:
            ms = solvers[:k]
            batch = bdd_hip_batch(ms)
            for _ in range(3):
                batch.iterations(a.iters)
            for s in ms:
                s.synchronize()
            dev = batch.time_iterations(a.iters)
            for s in ms:
                s.synchronize()
            t0 = time.perf_counter()
            batch.iterations(a.iters)
            for s in ms:
                s.synchronize()
            wall = (time.perf_counter() - t0) * 1e3
            batch.close()
            for _ in range(3):
                for s in ms:
                    s.iterations(a.iters)
            for s in ms:
                s.synchronize()
            t0 = time.perf_counter()
            for s in ms:
                s.iterations(a.iters)
            for s in ms:
                s.synchronize()
            serial = (time.perf_counter() - t0) * 1e3
            dev1 = dev if dev1 is None else dev1
            lines.append(f"{precision:9s} {k:5d} {dev:10.3f} {wall:11.3f} {serial:12.3f} {serial / wall:13.2f} {dev / dev1:14.2f}")
            print(lines[-1], flush=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
