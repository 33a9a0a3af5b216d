"""Timing of a batch's lower bounds (bddmma_batch_lower_bounds) and of the rounding loop that calls them once per round.
  python tools/batch_bound_time.py [--package DIR] [--label NAME] [--out FILE] [--only SET:PRECISION] [--reps R]    on an MI355X
--package: the directory that holds the bdd_amd package to measure (default: this tree) — run it once on this tree and once on a build of
the parent commit, alternating: the parent sweeps and reduces member by member (a backward sweep, a k_lb_reduce launch and a polled host
wait each), this tree in one launch per wave count present and one wait.  --only: one leg, e.g. assign:float, for a kernel trace.

The two member sets of tools/batch_round_time.py (32 assignment problems; the mixed set of 15 members in float, 12 in double).  Per set
and precision, by host wall clock around the call (it waits on the host itself), 2 warm-up calls and R = 10 repetitions (median / min /
max, microseconds), as one JSON line:
  stale    every member's costs-to-terminal stale (update_costs on every member in front of each call, waited for)
  swept    every member swept but no bound cached (one batch iteration in front of each call, waited for)
  rounding bddmma_incremental_mm_agreement_rounding_batch with init_delta 0.1, growth 1.2, num_itr_lb 20, 500 rounds, from the same costs"""
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
ap.add_argument("--only", default=None)
ap.add_argument("--reps", type=int, default=10)
args = ap.parse_args()
sys.path[:0] = [args.package]

import numpy as np  # noqa: E402

from bdd_amd import to_bdd_collection  # noqa: E402
from bdd_amd.instances import assignment_ilp, random_set_cover  # noqa: E402
from bdd_amd.solver import bdd_hip_batch, bdd_hip_parallel_mma  # noqa: E402

COVERS = {"cover40x60": (40, 60, 5), "cover67x100": (67, 100, 7), "cover147x220": (147, 220, 8), "cover200x300": (200, 300, 9)}
WARMUP = 2


def problems(kind, precision):
    if kind == "assign":
        ilp = assignment_ilp(8)
        col, costs = to_bdd_collection(ilp), np.asarray(ilp.objective, np.float64)
        return [(col, costs * np.random.default_rng(100 + k).uniform(0.5, 1.5, costs.shape)) for k in range(32)]
    out = []
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


def stats(us):
    return dict(median=round(statistics.median(us), 1), min=round(min(us), 1), max=round(max(us), 1))


def timed(prepare, call, reps):
    us = []
    for r in range(WARMUP + reps):
        prepare()
        t0 = time.perf_counter()
        call()
        if r >= WARMUP:
            us.append((time.perf_counter() - t0) * 1e6)
    return stats(us)


def leg(kind, precision):
    solvers = [bdd_hip_parallel_mma(col, costs, precision=precision) for col, costs in problems(kind, precision)]
    assert all(s.fused_small() for s in solvers)
    batch = bdd_hip_batch(solvers)
    rng = np.random.default_rng(7)
    start = batch.get_solver_costs()

    def make_stale():
        for s in solvers:
            s.update_costs([], rng.uniform(-0.01, 0.01, s.nr_variables()))
        for s in solvers:
            s.synchronize()

    def make_swept():
        batch.iterations(1)
        for s in solvers:
            s.synchronize()

    def reset():
        batch.set_solver_costs(*start)
        for s in solvers:
            s.synchronize()

    out = dict(label=args.label, set=kind, precision=precision, members=len(solvers))
    out["stale"] = timed(make_stale, batch.lower_bounds, args.reps)
    out["swept"] = timed(make_swept, batch.lower_bounds, args.reps)
    out["rounding"] = timed(reset, lambda: batch.primal_rounding_incremental(0.1, 1.2, 20, num_rounds=500, seed=0), args.reps)
    batch.close()
    return out


lines = []
for kind in ("assign", "mixed"):
    for precision in ("float", "double"):
        if args.only and args.only != f"{kind}:{precision}":
            continue
        lines.append(json.dumps(leg(kind, precision)))
        print(lines[-1], flush=True)
if args.out:
    with open(args.out, "a") as f:
        f.write("\n".join(lines) + "\n")
