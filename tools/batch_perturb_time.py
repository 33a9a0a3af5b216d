"""Timing of the last three operators of bdd_amd/autograd.py on a bdd_hip_batch: ComputePerBDDSolutions, PerturbPrimalCosts forward and
its backward.
  python tools/batch_perturb_time.py [--package DIR] [--label NAME] [--out FILE] [--only SET:PRECISION] [--warmup W] [--reps R]    on an MI355X
  python tools/batch_perturb_time.py --table FILE                                                                  anywhere
--package: the directory that holds the bdd_amd package to measure (default: this tree) — run it once on this tree and once on a build of
the parent commit, alternating, to compare the batch calls (one launch per operator and wave count present) with the per-member loop the
parent runs there.  --only: one leg, e.g. assign:float, for a kernel trace.  --table: the comparison of the lines collected in FILE
(labels parentN / treeN) under the three-spreads rule of profiles/batch_round_time.txt.

The two member sets of tools/batch_mmdiff_time.py (32 assignment problems; the mixed set: 1-10 packs in float, 1-7 in double), both
precisions.  Per set, precision and operator, by host wall clock with a device synchronisation behind each call (2 warm-up calls, 10
repetitions: median / min / max, microseconds), as one JSON line per set and precision.  The backward is timed alone: its forward runs
untimed in front of it."""
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
ap.add_argument("--table", default=None)
args = ap.parse_args()

ROWS = ("ComputePerBDDSolutions", "PerturbPrimalCosts forward", "PerturbPrimalCosts backward")


def table(path):
    """per set, precision and operator: the median of the runs' medians and the range of all samples for parent and tree, and whether the
    row meets the rule — every tree sample below every parent sample and the gap at least three of the parent's spreads"""
    runs = {}
    for ln in open(path):
        ln = ln.strip()
        if not ln.startswith("{"):
            continue
        r = json.loads(ln)
        side = "parent" if r["label"].startswith("parent") else "tree"
        for row in ROWS:
            runs.setdefault((r["set"], r["precision"], r["members"], row), {}).setdefault(side, []).append(r["rows"][row])
    print(f"{'set / precision':22s} {'members':>7s}  {'operator':28s} {'parent: median of medians [min .. max] us':44s} {'tree':36s} {'ratio':>6s}  gap / spread  claimed")
    for (kind, precision, members, row), sides in runs.items():
        fig = {}
        for side in ("parent", "tree"):
            xs = sides.get(side, [])
            fig[side] = (statistics.median(x["median"] for x in xs), min(x["min"] for x in xs), max(x["max"] for x in xs)) if xs else None
        if not fig["parent"] or not fig["tree"]:
            continue
        (pm, plo, phi), (tm, tlo, thi) = fig["parent"], fig["tree"]
        spread = phi - plo
        gap = plo - thi
        claimed = gap > 0 and gap >= 3 * spread
        print(f"{kind + ' ' + precision:22s} {members:7d}  {row:28s} {pm:9.1f} [{plo:9.1f} .. {phi:9.1f}]         {tm:9.1f} [{tlo:9.1f} .. {thi:9.1f}]   "
              f"{pm / tm:6.2f}  {gap / spread if spread > 0 else float('inf'):10.1f}    {'yes' if claimed else 'no'}")


if args.table:
    table(args.table)
    sys.exit(0)

sys.path[:0] = [args.package]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from bdd_amd import to_bdd_collection  # noqa: E402
from bdd_amd.autograd import ComputePerBDDSolutions, PerturbPrimalCosts  # noqa: E402
from bdd_amd.instances import assignment_ilp, random_set_cover  # noqa: E402
from bdd_amd.solver import bdd_hip_batch, bdd_hip_parallel_mma  # noqa: E402

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
    nv = sum(s.nr_variables() for s in solvers)
    rng = np.random.default_rng(7)
    p_lo, p_hi = (torch.tensor(rng.uniform(-1, 1, nv), dtype=tdt, device="cuda", requires_grad=True) for _ in range(2))
    w_lo, w_hi = (torch.tensor(rng.normal(0, 1, lo.numel()), dtype=tdt, device="cuda") for _ in range(2))
    walls = {row: [] for row in ROWS}
    for rep in range(args.warmup + args.reps):
        _, t_sol = timed(lambda: ComputePerBDDSolutions(batch, lo, hi))
        out, t_fwd = timed(lambda: PerturbPrimalCosts.apply(batch, p_lo, p_hi, lo, hi))
        loss = (out[0] * w_lo).sum() + (out[1] * w_hi).sum()
        _, t_bwd = timed(lambda: torch.autograd.grad(loss, (p_lo, p_hi)))
        if rep >= args.warmup:
            for row, t in zip(ROWS, (t_sol, t_fwd, t_bwd)):
                walls[row].append(t)
    res = dict(label=args.label, set=kind, precision=precision, members=len(solvers), layers=int(lo.numel()), variables=int(nv),
               rows={row: stats(walls[row]) for row in ROWS})
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
