"""Timing of the log-sum-exp family on a bdd_hip_batch: GetSumMarginals (logits), GetMarginalProbability — the learned solver's sum-marginal
and probability features — and the gradient of the smooth per-BDD bounds, its smooth loss gradient.
  python tools/batch_smooth_time.py [--package DIR] [--label NAME] [--out FILE]        on an MI355X
--package: the directory that holds the bdd_amd package to measure (default: this tree) — run it once on this tree and once on a build of
the parent commit, alternating, to compare the batch calls with the per-member loops the parent runs there.

The gradient is timed as the step the backward of ComputeLowerBoundperBDD with smooth_gradients_temp > 0 makes: the costs are set, then
the gradient is taken — with one batch.set_solver_costs and one batch.grad_smooth_lower_bound_per_bdd where the package's batch has that
method, with that backward's per-member loop where it has not (the parent).

The two member sets of tools/batch_mmdiff_time.py (32 assignment problems; the mixed set: 1-10 packs in float, 1-7 in double), both
precisions.  Per set and precision, by host wall clock with a device synchronisation behind each part (3 warm-up steps, 10 repetitions:
median / min / max, microseconds), as one JSON line: sum_marginals, probability, gradient."""
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
from bdd_amd.autograd import GetMarginalProbability, GetSumMarginals, _batch_set_costs, _Ordered  # noqa: E402
from bdd_amd.instances import assignment_ilp, random_set_cover  # noqa: E402
from bdd_amd.solver import bdd_hip_batch, bdd_hip_parallel_mma  # noqa: E402

WARMUP, REPS = 3, 10
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


def smooth_gradient(batch, lo, hi, zero, g, g_lo, g_hi):
    """the smooth backward of ComputeLowerBoundperBDD on a batch: batch calls where the package has them, else its per-member loop"""
    if hasattr(batch, "grad_smooth_lower_bound_per_bdd"):
        with _Ordered([batch]):
            assert _batch_set_costs(batch, lo, hi, zero)
            batch.grad_smooth_lower_bound_per_bdd(g, out=(g_lo, g_hi))
        return g_lo, g_hi
    solvers = batch.solvers
    off = np.cumsum([0] + [s.nr_layers() for s in solvers])
    ob = np.cumsum([0] + [s.nr_bdds() for s in solvers])
    with _Ordered(solvers):
        for i, s in enumerate(solvers):
            l, b = slice(off[i], off[i + 1]), slice(ob[i], ob[i + 1])
            s.set_solver_costs(lo[l], hi[l], zero[l])
            s.grad_smooth_lower_bound_per_bdd(g[b], out=(g_lo[l], g_hi[l]))
    return g_lo, g_hi


def run(kind, precision):
    solvers = [bdd_hip_parallel_mma(col, costs, precision=precision) for col, costs in problems(kind, precision)]
    assert all(s.fused_small() for s in solvers)
    batch = bdd_hip_batch(solvers)
    tdt = torch.float64 if precision == "double" else torch.float32
    costs = [s.get_solver_costs() for s in solvers]
    lo, hi = (torch.tensor(np.concatenate([c[k] for c in costs]), dtype=tdt, device="cuda") for k in range(2))
    zero = torch.zeros_like(lo)
    g = torch.sin(torch.arange(sum(s.nr_bdds() for s in solvers), device="cuda", dtype=tdt))
    g_lo, g_hi = torch.empty_like(lo), torch.empty_like(hi)
    walls = {k: [] for k in ("sum_marginals", "probability", "gradient")}
    for rep in range(WARMUP + REPS):
        sm, t_s = timed(lambda: GetSumMarginals(batch, lo, hi, True))
        x, t_p = timed(lambda: GetMarginalProbability(batch, lo, hi))
        gr, t_g = timed(lambda: smooth_gradient(batch, lo, hi, zero, g, g_lo, g_hi))
        if rep >= WARMUP:
            for k, v in zip(walls, (t_s, t_p, t_g)):
                walls[k].append(v)
    assert bool(torch.isfinite(sm[0]).all()) and bool(((x >= 0) & (x <= 1)).all()) and bool((gr[0] != 0).any()) and bool((gr[1] != 0).any())
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
