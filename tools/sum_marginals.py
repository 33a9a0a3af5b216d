"""Sum-marginals (bddmma_sum_marginals): accuracy table and timing, written to profiles/sum_marginals.txt.
  python tools/sum_marginals.py [--out FILE] [--no-full-size]        on an MI355X
Per family and precision: `yardstick` = largest absolute deviation of the log values between the NumPy restatement (tests/
sum_marginals_restatement.py) in the solver's precision and in the next wider type; `device` = largest deviation of the device from the
wider run; `allowed` = the smallest allowance of the test (4 x yardstick, floor 16 ulp of max(1, |log|)).
Full size (the benchmark's instance, 10.5 M nodes, float): bddmma_time_kernel of the forward / backward sum sweeps (kinds 8 / 9) and of the
plain sweeps (0 / 1), and whole calls of sum_marginals_cuda / min_marginals_cuda into device buffers, 20 repetitions each after warm-up.
  python tools/sum_marginals.py --trace-child      one solver, three sum_marginals calls: the program to run under
                                                   rocprofv3 --kernel-trace --stats (counts and durations of k_sm_fwd / k_sm_bwd)"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from bdd_amd.instances import random_set_cover_mt  # noqa: E402
from bdd_amd.solver import bdd_hip_parallel_mma  # noqa: E402


def accuracy(out):
    import test_gpu_sum_marginals as T
    from sum_marginals_restatement import restatement_of
    out.append(f"{'family':16s} {'precision':9s} {'itr':>3s} {'yardstick':>10s} {'device':>10s} {'allowed':>10s}")
    worst = {}
    for family in sorted(T.FAMILIES):
        make, opts = T.FAMILIES[family]
        col, costs = make()
        for precision in ("double", "float"):
            s = bdd_hip_parallel_mma(col, costs, precision=precision, **opts)
            m = restatement_of(col, costs, precision)
            perm = s.bdd_major_order()
            for n_itr in (0, 5):
                if n_itr:
                    s.iterations(n_itr)
                T._sync_costs(s, m, perm)
                (r0, r1), (t0, t1), dev = T._tolerance(m, s.value_type)
                _, lo, hi = s.sum_marginals_cuda(False, True)
                e = 0.0
                for g, r in ((lo[perm], r0), (hi[perm], r1)):
                    f = np.isfinite(r)
                    e = max(e, float(np.abs(g[f].astype(np.float64) - r[f]).max(initial=0.0)))
                out.append(f"{family:16s} {precision:9s} {n_itr:3d} {dev:10.3e} {e:10.3e} {min(t0.min(), t1.min()):10.3e}")
                w = worst.setdefault(precision, [0.0, 0.0])
                w[0], w[1] = max(w[0], dev), max(w[1], e)
            s.close()
    for p, (d, e) in worst.items():
        out.append(f"largest over all families, {p}: yardstick {d:.3e}, device {e:.3e}")


def med(xs):
    return f"median {statistics.median(xs) * 1e3:8.1f} us  (min {min(xs) * 1e3:.1f}, max {max(xs) * 1e3:.1f}, n = {len(xs)})"


def full_size(out):
    import torch
    col, costs = random_set_cover_mt(1_000_000, 500_000, 10, seed=12345)
    s = bdd_hip_parallel_mma(col, costs, precision="float")
    s.iterations(200)   # warm clocks
    L = s.nr_layers()
    bufs = (torch.zeros(L, dtype=torch.int32, device="cuda"), torch.zeros(L, dtype=torch.float32, device="cuda"), torch.zeros(L, dtype=torch.float32, device="cuda"))
    s.sum_marginals_cuda(False, True, out=bufs)
    s.min_marginals_cuda(False, out=bufs)
    out.append(f"full size: {col.nr_bdd_nodes()} nodes, {L} layers, float, {s.nr_packs()} packs, {s.nr_hops()} hops")
    t = {}
    for kind, name in ((8, "forward sum sweep"), (9, "backward sum sweep"), (0, "forward plain sweep"), (1, "backward plain sweep")):
        t[kind] = [s.time_kernel(kind, 1) for _ in range(20)]
        out.append(f"  {name:24s} {med(t[kind])}")
    for name, fn in (("sum_marginals_cuda call", lambda: s.sum_marginals_cuda(False, True, out=bufs)), ("min_marginals_cuda call", lambda: s.min_marginals_cuda(False, out=bufs))):
        xs = []
        for _ in range(20):
            t0 = time.perf_counter()
            fn()
            xs.append((time.perf_counter() - t0) * 1e3)
        t[name] = xs
        out.append(f"  {name:24s} {med(xs)}   (host wall clock, synchronous)")
    r = (statistics.median(t[8]) + statistics.median(t[9])) / (statistics.median(t[0]) + statistics.median(t[1]))
    out.append(f"  sum sweeps / plain sweeps (medians): {r:.2f};  calls: {statistics.median(t['sum_marginals_cuda call']) / statistics.median(t['min_marginals_cuda call']):.2f}")
    s.set_profiling(1)
    s.sum_marginals_cuda(False, True, out=bufs)
    out.append(f"  profiled launches of one call (class other): {s.get_profile()['launches'][3]}  (one per direction and pack family)")
    s.close()


def trace_child():
    col, costs = random_set_cover_mt(1_000_000, 500_000, 10, seed=12345)
    s = bdd_hip_parallel_mma(col, costs, precision="float")
    s.iterations(50)
    for _ in range(3):
        s.sum_marginals_cuda(False, True)
    print("hops", s.nr_hops(), "packs", s.nr_packs())
    s.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sum_marginals.txt"))
    ap.add_argument("--no-full-size", action="store_true")
    ap.add_argument("--trace-child", action="store_true")
    a = ap.parse_args()
    if a.trace_child:
        trace_child()
        sys.exit(0)
    lines = ["Sum-marginals (bddmma_sum_marginals) on one MI355X — written by tools/sum_marginals.py (see its docstring for the columns).", ""]
    accuracy(lines)
    if not a.no_full_size:
        lines.append("")
        full_size(lines)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
