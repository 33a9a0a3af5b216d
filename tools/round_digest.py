"""SHA-256 digests of what the entry points print whose kernels share device functions with the round kernel of a batch
(kernels/batchround.hpp): bddmma_perturb_primal_costs (k_round_perturb, then k_cost_quotients / k_update_costs), bddmma_update_costs with
full and with shorter vectors, and bddmma_set_solver_costs_batch (k_small_set_batch).
  python tools/round_digest.py [--package DIR]        on an MI355X
Run it with the parent's package and with this tree's and compare the printouts byte for byte: one line per (precision, problem, output)."""
import argparse
import hashlib
import os
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--package", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
args = ap.parse_args()
sys.path[:0] = [args.package]

import numpy as np  # noqa: E402

from bdd_amd import to_bdd_collection  # noqa: E402
from bdd_amd.instances import assignment_ilp, random_set_cover  # noqa: E402
from bdd_amd.solver import bdd_hip_batch, bdd_hip_parallel_mma  # noqa: E402

COVERS = {"cover40x60": (40, 60, 5), "cover67x100": (67, 100, 7), "cover147x220": (147, 220, 8), "cover200x300": (200, 300, 9)}


def problems(precision):
    ilp = assignment_ilp(8)
    out = [("assign8", to_bdd_collection(ilp), np.asarray(ilp.objective, np.float64))]
    for name, (v, r, per_row) in COVERS.items():
        if name != "cover200x300" or precision == "float":
            out.append((name,) + tuple(random_set_cover(v, r, per_row, seed=r)))
    return out


def line(precision, name, what, *arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    print(precision, name, what, h.hexdigest(), flush=True)


for precision in ("float", "double"):
    rng = np.random.default_rng(5)
    solvers = []
    for name, col, costs in problems(precision):
        s = bdd_hip_parallel_mma(col, costs, precision=precision)
        assert s.fused_small()
        solvers.append((name, s))
        s.iterations(3)
        for round_index, seed in ((0, 0), (4, 11)):
            r = s.perturb_primal_costs(0.1 * (1 + round_index), round_index, seed)
            line(precision, name, f"perturb {round_index} {seed}", np.asarray(r["counts"], np.uint32), r["sol"], r["cost_delta_0"], r["cost_delta_1"])
            line(precision, name, f"costs behind perturb {round_index} {seed}", *s.get_solver_costs())
            s.iterations(2)
        v = s.nr_variables()
        for n_lo, n_hi in ((v, v), (v // 2, v), (v, 0)):
            s.update_costs(rng.uniform(-1, 1, n_lo), rng.uniform(-1, 1, n_hi))
            line(precision, name, f"update_costs {n_lo == v} {n_hi == v}", *s.get_solver_costs())
    members = [s for _, s in solvers]
    batch = bdd_hip_batch(members)
    n, dt = sum(s.nr_layers() for s in members), members[0].value_type
    for given in ((1, 1, 1), (1, 0, 0), (0, 1, 1)):
        arrays = [rng.uniform(-1, 3, n).astype(dt) if g else None for g in given]
        batch.set_solver_costs(*arrays)
        line(precision, "batch", f"set {given}", batch.lower_bounds(), *[s.lower_bound_per_bdd() for s in members], *[x for s in members for x in s.get_solver_costs()])
    batch.close()
