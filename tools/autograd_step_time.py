"""Timing of one training step through bdd_amd.autograd on the benchmark's default instance (10.5 M nodes), both precisions: DualIterations with
20 iterations of which the last one is tracked, ComputeLowerBoundperBDD, the sum of the bounds as the loss, backward().
  python tools/autograd_step_time.py [--out FILE]        on an MI355X
Per precision: the step by host wall clock with a device synchronisation behind it (after 3 warm-up steps, 10 repetitions, median / min / max),
its forward and its backward alone, and next to them the sum of the device times of the launch groups the step consists of, each measured
with hipEvents around 20 repetitions (bddmma_time_kernel):
  forward   20 learned iterations (kinds 2 + 3 + 2 x 4 each), the plain backward sweep of the bound (1)
  backward  the bound's gradient (the plain backward sweep 1 and a forward sweep 0 for the arg-min paths), 19 untracked iterations replayed,
            one reversed iteration (13 + 14 + 15 + 16 + 17 and its replay 1 + 2 + 3 + 2 x 4)
What the step pays beyond its launch groups is on the host side of the calls: set_solver_costs / get_solver_costs copies with a
synchronisation each, the checked load of the arguments, the state and cache copies and the output copies of grad_iterations, and torch's
own allocations and fills."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
from bdd_amd.instances import random_set_cover_mt  # noqa: E402
from bdd_amd.solver import bdd_hip_parallel_mma  # noqa: E402

ITERATIONS, TRACKED, REPS, KERNEL_REPS = 20, 1, 10, 20


def run(precision, out):
    import torch

    from bdd_amd.autograd import ComputeLowerBoundperBDD, DualIterations
    col, costs = random_set_cover_mt(1_000_000, 500_000, 10, seed=12345)
    s = bdd_hip_parallel_mma(col, costs, precision=precision)
    s.iterations(200)   # warm clocks, costs as in the middle of a solve
    L = s.nr_layers()
    tdt = torch.float64 if precision == "double" else torch.float32
    state = [torch.zeros(L, dtype=tdt, device="cuda") for _ in range(3)]
    s.get_solver_costs(out=state)
    w = torch.from_numpy(s.get_isotropic_dist_weights()).to("cuda")
    omega = torch.full((1,), 0.5, dtype=tdt, device="cuda")
    leaves = [x.clone().requires_grad_(True) for x in state + [w, omega]]
    walls = {"forward": [], "backward": [], "step": []}

    def step(record):
        for x in leaves:
            x.grad = None
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        lo, hi, mm, _, _, _ = DualIterations.apply([s], *leaves[:4], ITERATIONS, leaves[4], TRACKED, 0.0, 1, 0, 0.9)
        loss = ComputeLowerBoundperBDD.apply([s], lo, hi).sum()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        loss.backward()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        if record:
            walls["forward"].append((t1 - t0) * 1e6)
            walls["backward"].append((t2 - t1) * 1e6)
            walls["step"].append((t2 - t0) * 1e6)

    for _ in range(3):
        step(False)
    for _ in range(REPS):
        step(True)
    assert all(x.grad is not None and bool(torch.isfinite(x.grad).all()) for x in leaves)
    out.append(f"{precision}: {col.nr_bdd_nodes()} nodes, {L} layers, {s.nr_packs()} packs; DualIterations {ITERATIONS} iterations ({TRACKED} tracked), "
               "per-BDD bound, backward")
    for k in ("step", "forward", "backward"):
        xs = walls[k]
        out.append(f"  {k:9s} median {statistics.median(xs):10.1f} us (min {min(xs):.1f}, max {max(xs):.1f}; host wall clock, synchronised)")
    t = {kind: s.time_kernel(kind, KERNEL_REPS) * 1e3 for kind in (0, 1, 2, 3, 4, 13, 14, 15, 16, 17)}
    it = t[2] + t[3] + 2 * t[4]
    fwd = ITERATIONS * it + t[1]
    bwd = t[1] + t[0] + (ITERATIONS - TRACKED) * it + TRACKED * (t[13] + t[14] + t[16] + t[17] + t[1] + it) + t[15]
    out.append(f"  launch groups (hipEvents around {KERNEL_REPS}): iteration {it:.1f} us, reversed iteration {t[13] + t[14] + t[16] + t[17] + t[1] + it:.1f} us, "
               f"through T {t[15]:.1f} us, plain sweeps {t[0]:.1f} / {t[1]:.1f} us")
    out.append(f"  sum of the launch groups: forward {fwd:.1f} us, backward {bwd:.1f} us, step {fwd + bwd:.1f} us")
    med = statistics.median(walls["step"])
    out.append(f"  step by wall clock / sum of its launch groups: {med:.1f} / {fwd + bwd:.1f} us = {med / (fwd + bwd):.2f}")
    s.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "autograd_step_time.txt"))
    a = ap.parse_args()
    lines = ["One training step through bdd_amd.autograd on one MI355X — written by tools/autograd_step_time.py (see its docstring).", ""]
    for p in ("float", "double"):
        run(p, lines)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
