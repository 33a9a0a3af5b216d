"""Timing of primal rounding on a bdd_hip_batch: ComputePrimalSolution (init_delta 0.1, growth 1.2, num_itr_lb 20, the default 500 rounds)
— what every evaluation of the learned solver ends with.
  python tools/batch_round_time.py [--package DIR] [--label NAME] [--out FILE] [--only SET:PRECISION] [--warmup W] [--reps R]    on an MI355X
--package: the directory that holds the bdd_amd package to measure (default: this tree) — run it once on this tree and once on a build of
the parent commit, alternating, to compare the batch loop (one launch per round and wave count present) with the per-member loop the
parent runs there.  --only: one leg, e.g. assign:float, for a kernel trace.

The two member sets of tools/batch_mmdiff_time.py (32 assignment problems; the mixed set: 1-10 packs in float, 1-7 in double), both
precisions.  Per set and precision, by host wall clock with a device synchronisation behind each call (2 warm-up calls, 10 repetitions:
median / min / max, microseconds), as one JSON line; every call starts from the same costs.  The time scales with the rounds the members
need, so where the package's batch reports them (this tree) the line also has, per member, the index of the round in which its agreement
was seen (500: none) and their maximum — the number of rounds the batch loop ran is that maximum + 1, capped at 500."""
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
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--reps", type=int, default=10)
args = ap.parse_args()
sys.path[:0] = [args.package]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from bdd_amd import to_bdd_collection  # noqa: E402
from bdd_amd.autograd import ComputePrimalSolution  # noqa: E402
from bdd_amd.instances import assignment_ilp, random_set_cover  # noqa: E402
from bdd_amd.solver import bdd_hip_batch, bdd_hip_parallel_mma  # noqa: E402

INIT_DELTA, GROWTH, NUM_ITR_LB, NUM_ROUNDS = 0.1, 1.2, 20, 500
COVERS = {"cover40x60": (40, 60, 5), "cover67x100": (67, 100, 7), "cover147x220": (147, 220, 8), "cover200x300": (200, 300, 9)}


def problems(kind, precision):
    """tools/batch_mmdiff_time.py's two sets"""
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
    zero = torch.zeros_like(lo)
    walls, sols = [], None
    for rep in range(args.warmup + args.reps):
        sols, t = timed(lambda: ComputePrimalSolution(batch, lo, hi, zero, INIT_DELTA, GROWTH, NUM_ITR_LB))
        if rep >= args.warmup:
            walls.append(t)
    res = dict(label=args.label, set=kind, precision=precision, members=len(solvers), layers=int(lo.numel()), found=sum(1 for x in sols if x),
               call_us=stats(walls))
    if hasattr(batch, "primal_rounding_incremental"):
        batch.set_solver_costs(lo, hi, zero)
        again, rounds = batch.primal_rounding_incremental(INIT_DELTA, GROWTH, NUM_ITR_LB, NUM_ROUNDS, return_rounds=True)
        assert again == sols
        res.update(rounds=rounds, rounds_max=max(rounds))
    batch.close()
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


for kind in ("assign", "mixed"):
    for precision in ("float", "double"):
        if args.only in (None, f"{kind}:{precision}"):
            run(kind, precision)
