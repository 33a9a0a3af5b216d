"""Timing of a training step through DualIterations on a bdd_hip_batch in the configuration the learned solver is trained in: 20 iterations,
compute_history_for_itrs = 20 (every iteration a history iteration), improvement_slope = 0, the gradient through all 20.
  python tools/batch_history_time.py [--package DIR] [--label NAME] [--out FILE]        on an MI355X
--package: the directory that holds the bdd_amd package to measure (default: this tree) — run it once on this tree and once on a build of
the parent commit, alternating, to compare the fused history launch with the list form the parent falls back to.

Two member sets, both precisions:
  assign   32 assignment problems of 8 x 8 (one pack each, different costs)
  mixed    set covers and assignment problems of 1, 2, 4 and 7 packs (10 packs too in float), three of each, interleaved
Per set and precision: forward, backward and the whole step by host wall clock with a device synchronisation behind each (3 warm-up steps,
10 repetitions: median / min / max, microseconds) as one JSON line.  Where the package has bdd_hip_batch.learned_iterations_history, also the
device time (events around the call on the current stream, ordered against the batch stream) of the 20 iterations with a history of 20
against the same call without a history: the price of 20 history steps."""
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
from bdd_amd.autograd import DualIterations  # noqa: E402
from bdd_amd.instances import assignment_ilp, random_set_cover  # noqa: E402
from bdd_amd.solver import bdd_hip_batch, bdd_hip_parallel_mma  # noqa: E402

ITERATIONS, HISTORY, WARMUP, REPS, BETA = 20, 20, 3, 10, 0.9
COVERS = {"cover40x60": (40, 60, 5), "cover67x100": (67, 100, 7), "cover147x220": (147, 220, 8), "cover200x300": (200, 300, 9)}


def problems(kind, precision):
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


def run(kind, precision):
    solvers = [bdd_hip_parallel_mma(col, costs, precision=precision) for col, costs in problems(kind, precision)]
    assert all(s.fused_small_learned() for s in solvers)
    batch = bdd_hip_batch(solvers)
    tdt = torch.float64 if precision == "double" else torch.float32
    costs = [s.get_solver_costs() for s in solvers]
    lo, hi, mm = (torch.tensor(np.concatenate([c[k] for c in costs]), dtype=tdt, device="cuda") for k in range(3))
    w = torch.tensor(np.concatenate([s.get_isotropic_dist_weights() for s in solvers]), dtype=tdt, device="cuda")
    omega = torch.full((1,), 0.5, dtype=tdt, device="cuda")
    leaves = [x.clone().requires_grad_(True) for x in (lo, hi, mm, w, omega)]
    g = [torch.ones_like(lo) for _ in range(3)]
    walls = {"forward": [], "backward": [], "step": []}
    for rep in range(WARMUP + REPS):
        for x in leaves:
            x.grad = None
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = DualIterations.apply(batch, *leaves[:4], ITERATIONS, leaves[4], ITERATIONS, 0.0, 1, HISTORY, BETA)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        torch.autograd.backward(out[:3], g)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        if rep >= WARMUP:
            walls["forward"].append((t1 - t0) * 1e6)
            walls["backward"].append((t2 - t1) * 1e6)
            walls["step"].append((t2 - t0) * 1e6)
    res = dict(label=args.label, set=kind, precision=precision, members=len(solvers), layers=int(lo.numel()),
               **{k + "_us": stats(v) for k, v in walls.items()})
    if hasattr(batch, "learned_iterations_history"):
        nb = sum(s.nr_bdds() for s in solvers)
        outs = [torch.zeros(lo.numel(), dtype=tdt, device="cuda"), torch.zeros(nb, dtype=tdt, device="cuda"), torch.zeros(nb, dtype=tdt, device="cuda")]
        cur = torch.cuda.current_stream()
        dev = {0: [], HISTORY: []}
        for rep in range(WARMUP + REPS):
            for history in (0, HISTORY):
                batch.set_solver_costs(lo, hi, mm)
                batch.stream_signal(cur.cuda_stream)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(cur)
                batch.stream_wait(cur.cuda_stream)
                batch.learned_iterations_history(w, ITERATIONS, omega=0.5, compute_history_for_itr=history, history_avg_beta=BETA, sol_avg=outs[0],
                                                 lb_first_diff_avg=outs[1], lb_second_diff_avg=outs[2])
                batch.stream_signal(cur.cuda_stream)
                e1.record(cur)
                torch.cuda.synchronize()
                if rep >= WARMUP:
                    dev[history].append(e0.elapsed_time(e1) * 1e3)
        res["device_no_history_us"] = stats(dev[0])
        res["device_history_us"] = stats(dev[HISTORY])
    batch.close()
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


for kind in ("assign", "mixed"):
    for precision in ("float", "double"):
        run(kind, precision)
