#!/usr/bin/env python3
"""One bdd_hip_batch.grad_iterations call against the loop of per-member grad_iterations calls, and one DualIterations forward + backward
step on a batch against the list of its members.

Member sets: 32 x the 8 x 8 assignment problem, and the 20-member float set of tests/test_gpu_small_learned.py (1 to 10 packs; 17 members
in double).  20 iterations of which 1 and 5 are tracked, float and double, host wall clock from the call to all members synchronised.
Every sample is a process of its own, batch and loop alternating on the same device; a process builds its members, makes one warm-up call
per case and times the next.  --loop-lib: the library the loop's processes load (a build of the parent commit; default: the tree's own —
the per-member call is the same code in both).
Writes profiles/grad_small_time.txt (or --out).  Usage: python3 tools/grad_small_time.py [--samples 5] [--loop-lib PATH] [--out FILE]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
NEW = "bddmma_grad_learned_iterations_batch"
ITERS, TRACKED = 20, (1, 5)


def child(mode, lib):
    import numpy as np
    import torch
    from bdd_amd import capi
    if lib:
        capi.LIB_PATH = lib
        if mode == "loop":
            capi.SIGNATURES.pop(NEW, None)   # a build of the parent commit does not export it
    from bdd_amd.autograd import DualIterations
    from bdd_amd.solver import bdd_hip_batch, bdd_hip_parallel_mma
    from test_gpu_small_learned import SHAPES, dirichlet_weights, instance

    def members_of(which, precision):
        if which == "assign8x32":
            return [bdd_hip_parallel_mma(*instance("assign8", 1 + i % 3), precision=precision) for i in range(32)]
        out = []
        for pos in range(4):
            for name, _, fused_in, seeds in SHAPES:
                if precision in fused_in and pos < len(seeds):
                    out.append(bdd_hip_parallel_mma(*instance(name, seeds[pos]), precision=precision))
        return out

    res = {}
    for which in ("assign8x32", "mixed_set"):
        for precision in ("float", "double"):
            ms = members_of(which, precision)
            assert all(s.fused_small_learned() for s in ms)
            dt = ms[0].value_type
            rng = np.random.default_rng(5)
            w = [dirichlet_weights(s, rng) for s in ms]
            g = [[rng.normal(0, 1, s.nr_layers()).astype(dt) for s in ms] for _ in range(3)]
            batch = bdd_hip_batch(ms) if mode == "batch" else None
            cat = np.concatenate
            args = (cat(w), cat(g[0]), cat(g[1]), cat(g[2]))

            def sync():
                for s in ms:
                    s.synchronize()

            for n in TRACKED:
                kw = dict(omega=0.5, track_grad_after_itr=ITERS - n, track_grad_for_num_itr=n)

                def call():
                    if batch is not None:
                        batch.grad_iterations(*args, **kw)
                    else:
                        for i, s in enumerate(ms):
                            s.grad_iterations(w[i], g[0][i], g[1][i], g[2][i], **kw)
                    sync()

                call()
                t0 = time.perf_counter()
                call()
                res[f"{which} {precision} grad_iterations {n}"] = (time.perf_counter() - t0) * 1e3
            # one training step through DualIterations: forward of 20 iterations, backward over the last 5
            tdt = torch.float64 if precision == "double" else torch.float32
            costs = [s.get_solver_costs() for s in ms]
            lo, hi = (cat([c[k] for c in costs]) for k in range(2))
            t = [torch.tensor(v, dtype=tdt, device="cuda", requires_grad=True) for v in (lo, hi, np.zeros_like(lo), cat(w), np.asarray([0.5], dt))]
            go = [torch.tensor(cat(a), dtype=tdt, device="cuda") for a in g]

            def step():
                out = DualIterations.apply(batch if batch is not None else ms, *t[:4], ITERS, t[4], 5, 0.0, 1, 0, 0.9)
                torch.autograd.backward(out[:3], go)
                torch.cuda.synchronize()

            step()
            t0 = time.perf_counter()
            step()
            res[f"{which} {precision} DualIterations step"] = (time.perf_counter() - t0) * 1e3
            if batch is not None:
                batch.close()
            for s in ms:
                s.close()
    print("RESULT " + json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grad_small_time.txt"))
    ap.add_argument("--samples", type=int, default=5)
    ap.add_argument("--loop-lib", default="")
    ap.add_argument("--child", default="")
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.loop_lib if a.child == "loop" else "")
    samples = {"batch": [], "loop": []}
    for _ in range(a.samples):
        for mode in ("batch", "loop"):
            cmd = [sys.executable, os.path.abspath(__file__), "--child", mode] + (["--loop-lib", a.loop_lib] if a.loop_lib else [])
            out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
            if out.returncode != 0:   # no further process on the device behind a failed one
                sys.exit(f"{mode} process failed ({out.returncode}):\n{out.stdout[-2000:]}\n{out.stderr[-2000:]}")
            samples[mode].append(json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:]))
    lines = [f"# tools/grad_small_time.py --samples {a.samples}" + (" --loop-lib <a build of the parent commit>" if a.loop_lib else ""),
             f"# {ITERS} iterations, the last 1 / 5 tracked; host wall clock in ms, call to all members synchronised; {a.samples} samples each, one process per",
             "# sample, batch and loop alternating.  batch: one bdd_hip_batch.grad_iterations (DualIterations on the batch); loop: per-member",
             "# grad_iterations (DualIterations on the list)",
             f"{'case':50s} {'batch med':>10s} {'batch min':>10s} {'loop med':>10s} {'loop min':>10s} {'loop/batch (med)':>17s}"]
    for case in samples["batch"][0]:
        b = [s[case] for s in samples["batch"]]
        l = [s[case] for s in samples["loop"]]
        lines.append(f"{case:50s} {statistics.median(b):10.3f} {min(b):10.3f} {statistics.median(l):10.3f} {min(l):10.3f} {statistics.median(l) / statistics.median(b):17.2f}")
    text = "\n".join(lines) + "\n"
    with open(a.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
