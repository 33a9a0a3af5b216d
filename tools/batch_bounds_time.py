"""Timing of one whole training step on a bdd_hip_batch — the loss chain of the learned solver and its backward:
    DualIterations -> DistributeDeferredDelta -> ComputeLowerBoundperBDD -> backward()
with 20 iterations, compute_history_for_itrs = 20, improvement_slope = 0 and the gradient through all 20.
  python tools/batch_bounds_time.py [--package DIR] [--label NAME] [--out FILE]        on an MI355X
--package: the directory that holds the bdd_amd package to measure (default: this tree) — run it once on this tree and once on a build of
the parent commit, alternating, to compare the batched tail with the per-member loops the parent runs there.

The two member sets of tools/batch_history_time.py (32 assignment problems; the mixed set), both precisions.  Per set and precision, by
host wall clock with a device synchronisation behind each part (3 warm-up steps, 10 repetitions: median / min / max, microseconds), as
one JSON line:
  forward, backward, step          the whole chain
  dd_forward, lb_forward, lb_backward    the tail's three Functions by themselves, on inputs of their own
Where the package has bdd_hip_batch.distribute_delta, also the step batch call by batch call: every call of the step in order with the
host time of the call itself and the time until the device is idle behind it (a synchronisation behind every call, so the parts do not
overlap as they do in the step proper; medians of the 10 repetitions)."""
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
from bdd_amd.autograd import ComputeLowerBoundperBDD, DistributeDeferredDelta, DualIterations  # noqa: E402
from bdd_amd.instances import assignment_ilp, random_set_cover  # noqa: E402
from bdd_amd.solver import bdd_hip_batch, bdd_hip_parallel_mma  # noqa: E402

ITERATIONS, HISTORY, WARMUP, REPS, BETA = 20, 20, 3, 10, 0.9
COVERS = {"cover40x60": (40, 60, 5), "cover67x100": (67, 100, 7), "cover147x220": (147, 220, 8), "cover200x300": (200, 300, 9)}
BATCH_CALLS = ("stream_wait", "set_solver_costs", "learned_iterations_history", "get_solver_costs", "distribute_delta", "lower_bound_per_bdd",
               "grad_lower_bound_per_bdd", "grad_iterations", "stream_signal")


def problems(kind, precision):
    """tools/batch_history_time.py's two sets"""
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
    assert all(s.fused_small_learned() for s in solvers)
    batch = bdd_hip_batch(solvers)
    tdt = torch.float64 if precision == "double" else torch.float32
    costs = [s.get_solver_costs() for s in solvers]
    lo, hi, mm = (torch.tensor(np.concatenate([c[k] for c in costs]), dtype=tdt, device="cuda") for k in range(3))
    mm = mm + 0.125 * torch.sign(torch.sin(torch.arange(mm.numel(), device="cuda", dtype=tdt)))   # deferred differences of both signs for the tail alone
    w = torch.tensor(np.concatenate([s.get_isotropic_dist_weights() for s in solvers]), dtype=tdt, device="cuda")
    omega = torch.full((1,), 0.5, dtype=tdt, device="cuda")
    nb = sum(s.nr_bdds() for s in solvers)
    g_lb = torch.ones(nb, dtype=tdt, device="cuda")
    leaves = [x.clone().requires_grad_(True) for x in (lo, hi, mm, w, omega)]

    def forward():
        out = DualIterations.apply(batch, *leaves[:4], ITERATIONS, leaves[4], ITERATIONS, 0.0, 1, HISTORY, BETA)
        lo2, hi2 = DistributeDeferredDelta.apply(batch, *out[:3])
        return ComputeLowerBoundperBDD.apply(batch, lo2, hi2)

    walls = {k: [] for k in ("forward", "backward", "step", "dd_forward", "lb_forward", "lb_backward")}
    for rep in range(WARMUP + REPS):
        for x in leaves:
            x.grad = None
        lb, t_f = timed(forward)
        _, t_b = timed(lambda: lb.backward(g_lb))
        # the tail's Functions by themselves
        _, t_dd = timed(lambda: DistributeDeferredDelta.apply(batch, lo, hi, mm))
        u = [lo.clone().requires_grad_(True), hi.clone().requires_grad_(True)]
        lb2, t_lf = timed(lambda: ComputeLowerBoundperBDD.apply(batch, *u))
        _, t_lb = timed(lambda: lb2.backward(g_lb))
        if rep >= WARMUP:
            for k, v in zip(walls, (t_f, t_b, t_f + t_b, t_dd, t_lf, t_lb)):
                walls[k].append(v)
    res = dict(label=args.label, set=kind, precision=precision, members=len(solvers), layers=int(lo.numel()), bdds=int(nb),
               **{k + "_us": stats(v) for k, v in walls.items()})
    if hasattr(bdd_hip_batch, "distribute_delta"):
        # the step batch call by batch call: (name, host time of the call, time until the device is idle behind it)
        log, originals = [], {}

        def wrap(name):
            f = getattr(bdd_hip_batch, name)
            originals[name] = f

            def wrapper(*a, **kw):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                r = f(*a, **kw)
                t1 = time.perf_counter()
                torch.cuda.synchronize()
                log.append((name, (t1 - t0) * 1e6, (time.perf_counter() - t0) * 1e6))
                return r
            setattr(bdd_hip_batch, name, wrapper)

        for name in BATCH_CALLS:
            wrap(name)
        seqs = []
        for rep in range(WARMUP + REPS):
            for x in leaves:
                x.grad = None
            del log[:]
            forward().backward(g_lb)
            torch.cuda.synchronize()
            if rep >= WARMUP:
                seqs.append(list(log))
        for name, f in originals.items():
            setattr(bdd_hip_batch, name, f)
        assert all([c[0] for c in s] == [c[0] for c in seqs[0]] for s in seqs)
        res["calls"] = [dict(call=seqs[0][i][0], host_us=round(statistics.median(s[i][1] for s in seqs), 1),
                             idle_us=round(statistics.median(s[i][2] for s in seqs), 1)) for i in range(len(seqs[0]))]
    batch.close()
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


for kind in ("assign", "mixed"):
    for precision in ("float", "double"):
        run(kind, precision)
