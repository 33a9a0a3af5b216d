"""Timing of the backward operator of the min-marginal differences (bddmma_grad_min_marginal_diff) next to sum-marginals, the closest
existing pair of pull sweeps over the parent tables, on the benchmark's default instance (10.5 M nodes), both precisions.
  python tools/grad_time.py [--out FILE] [--label TEXT --append]        on an MI355X
(--label names the run in its first line and --append adds it to FILE: the rounds of two builds of the library, chosen with BDDMMA_LIB, side
by side in one file)
Per precision, after 3 warm-up calls of each entry point: hipEvents around 20 repetitions (bddmma_time_kernel) of the two gradient
launches (kinds 10 / 11, and 12 = both back to back) and of the two sum sweeps (kinds 8 / 9); the ratio is (gradient pair) / (sum pair).
Whole calls into device buffers (host wall clock, synchronous: they include the plain sweeps a call recomputes, the copy and the finiteness
check of the incoming gradient and the output copies) are listed beside them."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
from bdd_amd.instances import random_set_cover_mt  # noqa: E402
from bdd_amd.solver import bdd_hip_parallel_mma  # noqa: E402

REPS = 20


def run(precision, out):
    import torch
    col, costs = random_set_cover_mt(1_000_000, 500_000, 10, seed=12345)
    s = bdd_hip_parallel_mma(col, costs, precision=precision)
    s.iterations(200)   # warm clocks, costs as in the middle of a solve
    L = s.nr_layers()
    tdt = torch.float64 if precision == "double" else torch.float32
    g = torch.randn(L, dtype=tdt, device="cuda")
    bufs = (torch.zeros(L, dtype=torch.int32, device="cuda"), torch.zeros(L, dtype=tdt, device="cuda"), torch.zeros(L, dtype=tdt, device="cuda"))
    for _ in range(3):
        s.grad_all_min_marginal_differences(g, out=bufs[1:])
        s.sum_marginals_cuda(False, True, out=bufs)
    out.append(f"{precision}: {col.nr_bdd_nodes()} nodes, {L} layers, {s.nr_packs()} packs, {s.nr_hops()} hops")
    t = {}
    for kind, name in ((10, "gradient, root -> terminal"), (11, "gradient, terminal -> root"), (12, "gradient, both launches"), (8, "forward sum sweep"),
                       (9, "backward sum sweep")):
        t[kind] = s.time_kernel(kind, REPS) * 1e3
        out.append(f"  {name:28s} {t[kind]:8.1f} us per launch group (hipEvents around {REPS})")
    ratio = t[12] / (t[8] + t[9])
    out.append(f"  gradient pair / sum-marginals pair: {t[12]:.1f} / {t[8] + t[9]:.1f} us = {ratio:.2f}")
    for name, fn in (("grad_all_min_marginal_differences call", lambda: s.grad_all_min_marginal_differences(g, out=bufs[1:])),
                     ("sum_marginals_cuda call", lambda: s.sum_marginals_cuda(False, True, out=bufs))):
        xs = []
        for _ in range(REPS):
            t0 = time.perf_counter()
            fn()
            xs.append((time.perf_counter() - t0) * 1e6)
        out.append(f"  {name:40s} median {statistics.median(xs):8.1f} us (min {min(xs):.1f}, max {max(xs):.1f}; host wall clock, synchronous)")
    s.close()
    return ratio


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grad_time.txt"))
    ap.add_argument("--label", default="")
    ap.add_argument("--append", action="store_true")
    a = ap.parse_args()
    lines = [f"{a.label + ': ' if a.label else ''}bddmma_grad_min_marginal_diff against bddmma_sum_marginals on one MI355X — written by tools/grad_time.py "
             "(see its docstring).", ""]
    for p in ("float", "double"):
        run(p, lines)
    with open(a.out, "a" if a.append else "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
