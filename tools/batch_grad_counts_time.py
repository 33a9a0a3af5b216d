"""Timing of DualIterations' backward on a bdd_hip_batch whose members stopped at their own counts: the forward the way the learned solver
is run (100 iterations, compute_history_for_itrs = 20, improvement_slope = 1e-9), then the backward with grad_dual_itr_max_itr = 20.
  python tools/batch_grad_counts_time.py [--package DIR] [--label NAME] [--out FILE] [--slope-mixed X]     on an MI355X
  python tools/batch_grad_counts_time.py --table FILE                                                     anywhere: the table of the collected lines
--package: the directory that holds the bdd_amd package to measure (default: this tree) — run it on this tree and on a build of the parent
commit, alternating, three runs each (labels parent1, tree1, parent2, ...), to compare the one batch call with per-member counts
(bddmma_grad_learned_iterations_counts_batch) with the per-solver loop the parent runs whenever the counts differ: per member a
set_solver_costs and a host wait, and per tracked iteration about 25 launches and copies.

The two member sets of tools/batch_stop_time.py (32 assignment problems of 8 x 8; the mixed set: set covers and assignment problems of 1-10
packs in float, 1-7 in double, three of each), both precisions.  Per set and precision: the backward alone by host wall clock between two
device synchronisations (2 warm-up calls, 10 calls, each behind a forward of its own that is not timed: median / min / max, microseconds)
as one JSON line, with the members' counts of iterations run.  Should every member of a set stop at the same count, the line says so
(distinct_counts = 1) and --slope-assign / --slope-mixed raise the slope for that set.

--table: per row the median of the runs' medians, every sample's range, the ratio and "gap / spread" — the parent's fastest sample minus the
tree's slowest, over the parent's slowest minus its fastest.  A row is claimed only if every tree sample lies below every parent sample
and the gap is at least three of the parent's own spreads."""
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
ap.add_argument("--table", default=None)
ap.add_argument("--slope-assign", type=float, default=1e-9)
ap.add_argument("--slope-mixed", type=float, default=1e-9)
args = ap.parse_args()

ITERATIONS, HISTORY, TRACKED, WARMUP, REPS, BETA = 100, 20, 20, 2, 10, 0.9
COVERS = {"cover40x60": (40, 60, 5), "cover67x100": (67, 100, 7), "cover147x220": (147, 220, 8), "cover200x300": (200, 300, 9)}


def table(path):
    rows = {}
    for line in open(path):
        line = line.strip()
        if line.startswith("{"):
            r = json.loads(line)
            rows.setdefault((r["set"], r["precision"]), {}).setdefault(r["label"].rstrip("0123456789"), []).append(r)
    print(f"{'set / precision':18s} {'members':>7s}  {'parent: median of medians [min .. max] us':46s} {'tree':40s} {'ratio':>6s} {'gap / spread':>13s}  claimed   counts equal  distinct")
    for (kind, precision), by in rows.items():
        p, t = by["parent"], by["tree"]
        pm, tm = (statistics.median(r["backward_us"]["median"] for r in x) for x in (p, t))
        pmin, pmax = min(r["backward_us"]["min"] for r in p), max(r["backward_us"]["max"] for r in p)
        tmin, tmax = min(r["backward_us"]["min"] for r in t), max(r["backward_us"]["max"] for r in t)
        spreads = (pmin - tmax) / (pmax - pmin)
        claimed = tmax < pmin and spreads >= 3
        same = all(r["iterations_done"] == p[0]["iterations_done"] for r in p + t)
        print(f"{kind + ' ' + precision:18s} {p[0]['members']:7d}  {pm:10.1f} [{pmin:10.1f} .. {pmax:10.1f}]{'':11s} {tm:10.1f} [{tmin:10.1f} .. {tmax:10.1f}]{'':5s} "
              f"{pm / tm:6.2f} {spreads:13.1f}  {'yes' if claimed else 'no':7s}   {'yes' if same else 'no':12s}  {t[0]['distinct_counts']}")
    print("\nThe raw lines (label, set, precision, slope, median / min / max in microseconds, the members' iteration counts):")
    for by in rows.values():
        for rs in by.values():
            for r in rs:
                f = r["backward_us"]
                print(f"  {r['label']:8s} {r['set']:7s} {r['precision']:7s} {r['slope']:g} {f['median']:10.1f} {f['min']:10.1f} {f['max']:10.1f}   {r['iterations_done']}")


if args.table:
    table(args.table)
    sys.exit(0)

sys.path[:0] = [args.package]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from bdd_amd import to_bdd_collection  # noqa: E402
from bdd_amd.autograd import DualIterations  # noqa: E402
from bdd_amd.instances import assignment_ilp, random_set_cover  # noqa: E402
from bdd_amd.solver import bdd_hip_batch, bdd_hip_parallel_mma  # noqa: E402


def problems(kind, precision):
    """tools/batch_stop_time.py's two sets"""
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
    slope = args.slope_assign if kind == "assign" else args.slope_mixed
    solvers = [bdd_hip_parallel_mma(col, costs, precision=precision) for col, costs in problems(kind, precision)]
    assert all(s.fused_small_learned() and s.fused_small_stop() for s in solvers)
    batch = bdd_hip_batch(solvers)
    tdt = torch.float64 if precision == "double" else torch.float32
    costs = [s.get_solver_costs() for s in solvers]
    lo, hi, mm = (torch.tensor(np.concatenate([c[k] for c in costs]), dtype=tdt, device="cuda") for k in range(3))
    w = torch.tensor(np.concatenate([s.get_isotropic_dist_weights() for s in solvers]), dtype=tdt, device="cuda")
    omega = torch.full((1,), 0.5, dtype=tdt, device="cuda")
    g = [torch.tensor(np.random.default_rng(300 + k).normal(0, 1, lo.numel()), dtype=tdt, device="cuda") for k in range(3)]
    walls, done = [], None
    for rep in range(WARMUP + REPS):
        leaves = [x.clone().requires_grad_(True) for x in (lo, hi, mm, w, omega)]
        out = DualIterations.apply(batch, *leaves[:4], ITERATIONS, leaves[4], TRACKED, slope, 1, HISTORY, BETA)
        done = [int(x) for x in out[0].grad_fn.iterations_done]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        torch.autograd.backward(out[:3], g)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        if rep >= WARMUP:
            walls.append((t1 - t0) * 1e6)
        del out, leaves
    res = dict(label=args.label, set=kind, precision=precision, slope=slope, members=len(solvers), layers=int(lo.numel()), backward_us=stats(walls),
               iterations_done=done, distinct_counts=len(set(done)))
    batch.close()
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


for kind in ("assign", "mixed"):
    for precision in ("float", "double"):
        run(kind, precision)
