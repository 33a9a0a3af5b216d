"""Rate of learned_iterations (per-layer distribution weights: the weighted exchange, bddmma_learned_iterations) against the plain
iterations on the headline instance (random set cover k = 10, V = 1e6, B = 5e5: 10.5 M nodes), both precisions, improvement_slope = 0 (no
host synchronisation inside the loop).  Isotropic and random weights run the same kernels; isotropic ones are used.
python tools/learned_vs_plain.py [--iters N] [--reps R]"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bdd_amd.instances import random_set_cover_mt  # noqa: E402
from bdd_amd.solver import bdd_hip_parallel_mma  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=500)
ap.add_argument("--reps", type=int, default=5)
args = ap.parse_args()
col, costs = random_set_cover_mt(1_000_000, 500_000, 10, 12345)
print(f"instance: random set cover k=10, V=1e6, B=5e5, {col.nr_bdd_nodes()} BDD nodes; {args.reps} alternating runs of {args.iters} iterations")
for prec in ("float", "double"):
    s = bdd_hip_parallel_mma(col, costs, precision=prec)
    w = s.get_isotropic_dist_weights()
    s.iterations(50)
    s.learned_iterations(w, 50, 0.5, improvement_slope=0.0)
    s.synchronize()
    plain, learned = [], []
    for _ in range(args.reps):   # alternating, so that clock / neighbour drift hits both alike
        t0 = time.perf_counter(); s.iterations(args.iters); s.synchronize(); plain.append(args.iters / (time.perf_counter() - t0))
        t0 = time.perf_counter(); s.learned_iterations(w, args.iters, 0.5, improvement_slope=0.0); s.synchronize()
        learned.append(args.iters / (time.perf_counter() - t0))
    s.set_profiling(True, stride=1)
    s.learned_iterations(w, 100, 0.5, improvement_slope=0.0); s.synchronize()
    pl = s.get_profile(); s.set_profiling(False)
    s.set_profiling(True, stride=1)
    s.iterations(100); s.synchronize()
    pp = s.get_profile(); s.set_profiling(False)
    ex = lambda p: p["total_ms"][2] / max(p["launches"][2], 1) * 1e3
    pm, lm = sorted(plain)[len(plain) // 2], sorted(learned)[len(learned) // 2]
    print(f"{prec:6s}: plain {pm:8.1f} it/s (runs {' '.join(f'{x:.0f}' for x in plain)})  learned {lm:8.1f} it/s "
          f"(runs {' '.join(f'{x:.0f}' for x in learned)})  ratio {lm / pm:.3f};  exchange per launch: plain {ex(pp):.1f} us, weighted {ex(pl):.1f} us "
          f"(device bytes {s.device_bytes() / 1e6:.0f} MB)", flush=True)
    s.close()
