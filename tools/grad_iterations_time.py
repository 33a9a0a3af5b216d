"""Timing of one reversed learned iteration (bddmma_grad_learned_iterations with one tracked iteration and one cache) next to what exists
without it: one bddmma_learned_iterations iteration and the single-shot gradient pair (bddmma_time_kernel kind 12), on the benchmark's
default instance (10.5 M nodes), both precisions.
  python tools/grad_iterations_time.py [--out FILE]        on an MI355X
Per precision: hipEvents around 20 repetitions (bddmma_time_kernel) of every launch group of a reversed iteration — kinds 13 (k_gi_down,
the reverse of the backward pass), 14 (k_gi_up, the reverse of the forward pass), 15 (the final sweep through T), 16 (the copies and
memsets that keep what the reverse reads), 17 (its six elementwise launches) —, of the solve sweeps and the exchange it replays (kinds 1 - 4)
and of the single-shot gradient pair (kinds 10 - 12).  From these: reversed iteration = 13 + 14 + 16 + 17 + replay (1 + 2 + 3 + 2 x 4), and
the ratio to (replay + gradient pair).  Whole calls on device buffers by host wall clock with a synchronisation behind each (after 3
warm-up calls, 20 repetitions, median / min / max) are listed beside them; a whole grad_iterations call also pays the finiteness checks of
its inputs, the cache and state copies and the restore; the lines "whole call, ..." split it: no tracked iteration against one, the scalar omega
(whose gradient is summed over the layers by one workgroup, k_gi_omega_sum) against omega_vec."""
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
    w = torch.from_numpy(s.get_isotropic_dist_weights()).to("cuda")
    g = [torch.randn(L, dtype=tdt, device="cuda") for _ in range(3)]
    outs = (torch.zeros(L, dtype=tdt, device="cuda"), torch.zeros(1, dtype=tdt, device="cuda"))
    bufs = (torch.zeros(L, dtype=tdt, device="cuda"), torch.zeros(L, dtype=tdt, device="cuda"))

    def reversed_iteration():
        s.grad_iterations(w, g[0], g[1], g[2], 0.5, 0, 1, 1, out=outs)
        for x in g:   # keep the incoming gradients bounded from call to call
            x.clamp_(-1, 1)

    def iteration():
        s.learned_iterations(w, 1, 0.5, improvement_slope=0.0)
        s.synchronize()

    out.append(f"{precision}: {col.nr_bdd_nodes()} nodes, {L} layers, {s.nr_packs()} packs, {s.nr_hops()} hops")
    med = {}
    for name, fn in (("grad_iterations call, 1 tracked iteration", reversed_iteration), ("learned_iterations call, 1 iteration", iteration)):
        for _ in range(3):
            fn()
        xs = []
        for _ in range(REPS):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            xs.append((time.perf_counter() - t0) * 1e6)
        med[name] = statistics.median(xs)
        out.append(f"  {name:44s} median {med[name]:9.1f} us (min {min(xs):.1f}, max {max(xs):.1f}; host wall clock, synchronous)")
    # what a whole call consists of: no tracked iteration (argument loads, memsets, two output copies, one synchronisation) and one, for the
    # scalar omega and for omega_vec — the scalar's extra is k_gi_omega_sum, its fixed-order sum over the layers
    ov = torch.full((L,), 0.5, dtype=tdt, device="cuda")
    for vec in (False, True):
        o = (outs[0], torch.zeros(L, dtype=tdt, device="cuda") if vec else outs[1])
        for n in (0, 1):
            xs = []
            for i in range(3 + REPS):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                s.grad_iterations(w, g[0], g[1], g[2], 0.5, 0, n, 1, omega_vec=ov if vec else None, out=o)
                xs.append((time.perf_counter() - t0) * 1e6)
                for x in g:
                    x.clamp_(-1, 1)
            xs = xs[3:]
            name = f"whole call, {'omega_vec' if vec else 'scalar omega'}, {n} tracked"
            out.append(f"  {name:44s} median {statistics.median(xs):9.1f} us (min {min(xs):.1f}, max {max(xs):.1f}; host wall clock, synchronous)")
    for _ in range(3):
        s.grad_all_min_marginal_differences(g[0], out=bufs)
    t = {}
    for kind, name in ((13, "k_gi_down (reverse of the backward pass)"), (14, "k_gi_up (reverse of the forward pass)"), (15, "k_gi_down, through T only (once per call)"),
                       (16, "copies and memsets kept for the reverse"), (17, "six elementwise launches"), (1, "plain backward sweep"), (2, "forward solve sweep"),
                       (3, "backward solve sweep"), (4, "exchange"), (10, "single-shot gradient, root -> terminal"), (11, "single-shot gradient, terminal -> root"),
                       (12, "single-shot gradient pair")):
        t[kind] = s.time_kernel(kind, REPS) * 1e3
        out.append(f"  {name:44s}        {t[kind]:9.1f} us per launch group (hipEvents around {REPS})")
    replay = t[1] + t[2] + t[3] + 2 * t[4]
    rev = t[13] + t[14] + t[16] + t[17] + replay
    out.append(f"  replayed iteration (1 + 2 + 3 + 2 x 4): {replay:.1f} us;  reverse sweeps 13 + 14: {t[13] + t[14]:.1f} us = {(t[13] + t[14]) / t[12]:.2f} x the gradient pair")
    out.append(f"  reversed iteration / (replay + gradient pair), launch groups: {rev:.1f} / {replay + t[12]:.1f} us = {rev / (replay + t[12]):.2f}")
    a, b = med["grad_iterations call, 1 tracked iteration"], med["learned_iterations call, 1 iteration"] + t[12]
    out.append(f"  whole calls: grad_iterations / (learned_iterations + gradient pair): {a:.1f} / {b:.1f} us = {a / b:.2f}")
    s.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grad_iterations_time.txt"))
    a = ap.parse_args()
    lines = ["bddmma_grad_learned_iterations against bddmma_learned_iterations and the single-shot gradient pair on one MI355X — written by "
             "tools/grad_iterations_time.py (see its docstring).", ""]
    for p in ("float", "double"):
        run(p, lines)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
