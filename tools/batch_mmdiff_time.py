"""Timing of ComputeAllMinMarginalsDiff, forward and backward, on a bdd_hip_batch — the per-layer feature the learned solver's network reads
after every block of iterations, and what the primal-rounding loss differentiates through.
  python tools/batch_mmdiff_time.py [--package DIR] [--label NAME] [--out FILE]        on an MI355X
--package: the directory that holds the bdd_amd package to measure (default: this tree) — run it once on this tree and once on a build of
the parent commit, alternating, to compare the batch calls with the per-member loops the parent runs there.

The two member sets of tools/batch_bounds_time.py (32 assignment problems; the mixed set), both precisions.  Per set and precision, by
host wall clock with a device synchronisation behind each part (3 warm-up steps, 10 repetitions: median / min / max, microseconds), as
one JSON line: forward, backward, step (their sum)."""
import argparse
import json
import os
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--package", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--label", default="tree")
ap.add_argument("--out", default=None)
args = ap.parse_args()
sys.path[:0] = [args.package]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from bdd_amd import to_bdd_collection  # noqa: E402
from bdd_amd.autograd import ComputeAllMinMarginalsDiff  # noqa: E402
from bdd_amd.instances import assignment_ilp, random_set_cover  # noqa: E402
from bdd_amd.solver import bdd_hip_batch, bdd_hip_parallel_mma  # noqa: E402

WARMUP, REPS = 3, 10
COVERS = {"cover40x60": (40, 60, 5), "cover67x100": (67, 100, 7), "cover147x220": (147, 220, 8), "cover200x300": (200, 300, 9)}


def problems(kind, precision):
    """tools/batch_bounds_time.py's two sets"""
    out = []
    if kind == "assign":
        ilp = assignment_ilp(8)
        col, costs = to_bdd_collection(ilp), np.asarray(ilp.objective, np.float64)
        return [(col, costs * np.random.default_rng(100 + k).uniform(0.5, 1.5, costs.shape)) for k in range(32)]
    names = ["assign8", "cover40x60", "cover67x100", "cover147x220"] + (["cover200x300"] if precision == "float" else [])
    for k in range(3):
        for name in names:
            if name == "assign8":
                ilp = assignment_ilp(8)
                col, costs = to_bdd_collection(ilp), np.asarray(ilp.objective, np.float64)
            else:
                v, r, per_row = COVERS[name]
                col, costs = random_set_cover(v, r, per_row, seed=r)
            out.append((col, costs * np.random.default_rng(200 + k).uniform(0.5, 1.5, np.shape(costs))))
    return out


def stats(xs):
    return dict(median=round(statistics.median(xs), 1), min=round(min(xs), 1), max=round(max(xs), 1))


def timed(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = f()
    torch.cuda.synchronize()
    return r, (time.perf_counter() - t0) * 1e6


def run(kind, precision):
    solvers = [bdd_hip_parallel_mma(col, costs, precision=precision) for col, costs in problems(kind, precision)]
    assert all(s.fused_small() for s in solvers)
    batch = bdd_hip_batch(solvers)
    tdt = torch.float64 if precision == "double" else torch.float32
    costs = [s.get_solver_costs() for s in solvers]
    lo, hi = (torch.tensor(np.concatenate([c[k] for c in costs]), dtype=tdt, device="cuda") for k in range(2))
    g = torch.sin(torch.arange(lo.numel(), device="cuda", dtype=tdt))
    walls = {k: [] for k in ("forward", "backward", "step")}
    for rep in range(WARMUP + REPS):
        u = [lo.clone().requires_grad_(True), hi.clone().requires_grad_(True)]
        mm, t_f = timed(lambda: ComputeAllMinMarginalsDiff.apply(batch, *u))
        _, t_b = timed(lambda: mm.backward(g))
        if rep >= WARMUP:
            for k, v in zip(walls, (t_f, t_b, t_f + t_b)):
                walls[k].append(v)
    assert bool(torch.isfinite(mm).all()) and bool((u[0].grad != 0).any()) and bool((u[1].grad != 0).any())
    res = dict(label=args.label, set=kind, precision=precision, members=len(solvers), layers=int(lo.numel()),
               **{k + "_us": stats(v) for k, v in walls.items()})
    batch.close()
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


for kind in ("assign", "mixed"):
    for precision in ("float", "double"):
        run(kind, precision)
