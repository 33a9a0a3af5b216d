"""Digests of what the pull sweeps (kernels/pull.hpp: sum-marginals, gradient of the min-marginal differences) compute, to compare two
builds of the library bit for bit: a change of a fold's order of operations changes a line.
  BDDMMA_LIB=<library> python tools/pull_digest.py [--out FILE]        on an MI355X, once per build, each in a process of its own
Per family of tests/test_gpu_sum_marginals.py FAMILIES and precision, one line per output with the SHA-256 of its bytes:
  in the family's seeded tie-free state (tests/test_gpu_gradients.py: _tie_free_solver), set through set_solver_costs:
    sm_lo / sm_hi       the log sum-marginals, layer order        smooth      the smooth solution
    grad_lo / grad_hi   grad_all_min_marginal_differences of the state's seeded gradient
  after 20 iterations from the instance's own costs, where ties are frequent:
    grad20_lo / grad20_hi   the same gradient through grad_all_min_marginal_differences
The lines name no library, so the printouts of two builds are compared as they are."""
import argparse
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from bdd_amd.solver import bdd_hip_parallel_mma  # noqa: E402


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def run(out):
    import test_gpu_gradients as G
    import test_gpu_sum_marginals as T
    for family in sorted(T.FAMILIES):
        make, opts = T.FAMILIES[family]
        for precision in ("double", "float"):
            s, _, g, perm = G._tie_free_solver(family, precision)
            gp = G._to_public(g, perm)
            _, sm_lo, sm_hi = s.sum_marginals_cuda(get_sorted=False, get_log_probs=True)
            res = [("sm_lo", sm_lo), ("sm_hi", sm_hi), ("smooth", s.smooth_solution_per_bdd())]
            res += zip(("grad_lo", "grad_hi"), s.grad_all_min_marginal_differences(gp))
            s.close()
            col, costs = make()
            s = bdd_hip_parallel_mma(col, costs, precision=precision, **opts)
            s.iterations(20)
            res += zip(("grad20_lo", "grad20_hi"), s.grad_all_min_marginal_differences(gp))
            s.close()
            for name, a in res:
                assert a.dtype == s.value_type and a.shape == gp.shape, (family, precision, name)
                out.append(f"{family:16s} {precision:7s} {name:10s} {len(a):7d} values  {digest(a)}")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    a = ap.parse_args()
    lines = []
    run(lines)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
