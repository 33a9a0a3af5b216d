"""Wall clock of the batch farm's command line on many small instances, construction included.
  python tools/batch_farm_time.py --exe PATH/bdd_solver_cl [--fuse-small] [--label NAME] [--out FILE] [--runs R]    on an MI355X
Run it on the parent commit's bdd_solver_cl without --fuse-small and on this tree's with it, alternating.

Two sets, written as config files into a temporary directory: 256 assignment problems (8 x 8) with distinct costs, float, 200 iterations;
and a mixed set of 48 (assignment 3 x 3 and 8 x 8, coverings of 67 x 100 rows of 7 and 200 x 300 rows of 9, both precisions, half with
perturbation rounding).  Per set: R = 3 runs of `bdd_solver_cl --batch <configs> --devices 0 --quiet`, the wall clock of the whole
command (median / min / max, seconds), and the same with "maximum iterations" 0 and no rounding — process start, reading, BDD construction
and solver set-up, which are not fused and are the same work in both farms."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

from bdd_amd.instances import assignment_ilp  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--exe", required=True)
ap.add_argument("--fuse-small", action="store_true")
ap.add_argument("--label", default="tree")
ap.add_argument("--out", default=None)
ap.add_argument("--runs", type=int, default=3)
args = ap.parse_args()

ROUNDING = {"initial perturbation": 0.1, "perturbation growth rate": 1.2, "inner iterations": 20, "outer iterations": 30}


def covering_lp(n_vars, n_rows, k, seed):
    rng = np.random.default_rng(seed)
    costs = rng.uniform(0.5, 2.0, n_vars)
    lines = ["Minimize", " + ".join(f"{c:.6f} x{v + 1}" for v, c in enumerate(costs)), "Subject To"]
    for _ in range(n_rows):
        lines.append(" + ".join(f"x{v + 1}" for v in sorted(rng.choice(n_vars, size=k, replace=False))) + " >= 1")
    return "\n".join(lines + ["Bounds", "Binaries"] + [f"x{v + 1}" for v in range(n_vars)] + ["End", ""])


def cfg(lp, precision, max_iter, rounding):
    c = {"precision": precision, "relaxation solver": "cuda parallel mma", "input": lp,
         "termination criteria": {"maximum iterations": max_iter, "improvement slope": 0.0, "minimum improvement": 0.0, "time limit": 1e10}}
    if rounding:
        c["perturbation rounding"] = dict(ROUNDING)
    return c


def sets(construct_only):
    it = 0 if construct_only else 200
    rng = np.random.default_rng(5)
    assign = [cfg(assignment_ilp(8, rng.uniform(-3, 1, (8, 8))).write_lp(), "float", it, False) for _ in range(256)]
    mixed = []
    for k in range(6):
        for precision in ("float", "double"):
            lps = [assignment_ilp(3, rng.uniform(-3, 1, (3, 3))).write_lp(), assignment_ilp(8, rng.uniform(-3, 1, (8, 8))).write_lp(),
                   covering_lp(67, 100, 7, 10 + k), covering_lp(200, 300, 9, 20 + k)]
            mixed += [cfg(lp, precision, it, rounding=(i % 2 == 1) and not construct_only) for i, lp in enumerate(lps)]
    return {"assign256": assign, "mixed48": mixed}


def run(paths):
    cmd = [args.exe, "--batch", *paths, "--devices", "0", "--quiet"] + (["--fuse-small"] if args.fuse_small else [])
    t0 = time.perf_counter()
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    wall = time.perf_counter() - t0
    rows = [json.loads(l) for l in out.stdout.splitlines() if l.startswith("{")]
    assert out.returncode == 0 and len(rows) == len(paths) and all(r["ok"] for r in rows), out.stderr[-2000:]
    return wall, sum(1 for r in rows if r.get("fused"))


lines = []
with tempfile.TemporaryDirectory() as tmp:
    for construct_only in (False, True):
        for name, configs in sets(construct_only).items():
            paths = []
            for i, c in enumerate(configs):
                p = os.path.join(tmp, f"{name}_{int(construct_only)}_{i}.json")
                with open(p, "w") as f:
                    json.dump(c, f)
                paths.append(p)
            walls, fused = [], 0
            for _ in range(args.runs):
                w, fused = run(paths)
                walls.append(w)
            lines.append(json.dumps(dict(label=args.label, set=name, what="construct only" if construct_only else "solve", configs=len(paths), fused=fused,
                                         median=round(statistics.median(walls), 3), min=round(min(walls), 3), max=round(max(walls), 3))))
            print(lines[-1], flush=True)
if args.out:
    with open(args.out, "a") as f:
        f.write("\n".join(lines) + "\n")
