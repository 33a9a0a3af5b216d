"""Rate of learned_iterations with one omega per layer (omega_vec: the solve sweeps' OV instantiation, bddmma_learned_iterations_omega_vec)
against the scalar-omega learned iterations and the plain iterations on the headline instance (random set cover k = 10, V = 1e6, B = 5e5:
10.5 M nodes), both precisions, improvement_slope = 0.  Three runs alternate: plain, learned with omega 0.5, learned with a random omega per
layer in [0.3, 0.7]; medians are reported with the ratio of the omega_vec rate to the scalar learned rate, and the sweeps' times per launch
from the solver's profile.
python tools/learned_omega_vec.py [--iters N] [--reps R] > profiles/learned_omega_vec.txt"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bdd_amd.instances import random_set_cover_mt  # noqa: E402
from bdd_amd.solver import bdd_hip_parallel_mma  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=500)
ap.add_argument("--reps", type=int, default=5)
args = ap.parse_args()
col, costs = random_set_cover_mt(1_000_000, 500_000, 10, 12345)
print(f"instance: random set cover k=10, V=1e6, B=5e5, {col.nr_bdd_nodes()} BDD nodes; {args.reps} alternating runs of {args.iters} iterations")
TARGET = 0.85


def median(x):
    return sorted(x)[len(x) // 2]


def sweeps(s, run):
    """per-launch times (us) of the forward and backward solve sweeps over 100 profiled iterations"""
    s.set_profiling(True, stride=1)
    run(100)
    s.synchronize()
    p = s.get_profile()
    s.set_profiling(False)
    return [p["total_ms"][k] / max(p["launches"][k], 1) * 1e3 for k in (0, 1)]


for prec in ("float", "double"):
    s = bdd_hip_parallel_mma(col, costs, precision=prec)
    w = s.get_isotropic_dist_weights()
    rng = np.random.Generator(np.random.PCG64(1))
    vec = rng.uniform(0.3, 0.7, s.nr_layers()).astype(s.value_type)
    runs = {
        "plain": lambda n: s.iterations(n),
        "learned": lambda n: s.learned_iterations(w, n, 0.5, improvement_slope=0.0),
        "omega_vec": lambda n: s.learned_iterations(w, n, improvement_slope=0.0, omega_vec=vec),
    }
    for run in runs.values():   # warm-up
        run(50)
    s.synchronize()
    rates = {k: [] for k in runs}
    for _ in range(args.reps):   # alternating, so that clock / neighbour drift hits all three alike
        for k, run in runs.items():
            t0 = time.perf_counter()
            run(args.iters)
            s.synchronize()
            rates[k].append(args.iters / (time.perf_counter() - t0))
    med = {k: median(v) for k, v in rates.items()}
    ratio = med["omega_vec"] / med["learned"]
    print(f"{prec:6s} (solve sweeps: {s.solve_sweep_kind()}{', non-temporal loads' if s.nontemporal_loads() else ''}; "
          f"device bytes {s.device_bytes() / 1e6:.0f} MB)")
    for k in runs:
        print(f"    {k:9s} {med[k]:8.1f} it/s  (runs {' '.join(f'{x:.0f}' for x in rates[k])})")
    print(f"    omega_vec / learned {ratio:.3f} (target {TARGET}: {'met' if ratio >= TARGET else 'MISSED'});  "
          f"learned / plain {med['learned'] / med['plain']:.3f}")
    for k in ("learned", "omega_vec"):
        f, b = sweeps(s, runs[k])
        print(f"    {k:9s} sweeps per launch: forward {f:.1f} us, backward {b:.1f} us", flush=True)
    s.close()
