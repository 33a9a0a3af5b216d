#!/usr/bin/env python3
"""What a batch's set / get of the solver costs (bddmma_set_solver_costs_batch / bddmma_get_solver_costs_batch) saves.

(a) a set + get round trip with device tensors: one bdd_hip_batch.set_solver_costs + get_solver_costs against the loop of per-member
    calls, from the first call to everything synchronised;
(b) one DualIterations forward + backward step on a batch (20 iterations, the last 5 tracked — the step of tools/grad_small_time.py):
    this tree against a library built from the parent commit (--parent-lib), whose processes make the parent's calls: stream_wait,
    set_solver_costs, get_solver_costs and stream_signal per member around the same batch kernels;
(c) tree only, where the step's time goes: each of its five batch calls alone (synchronised behind each), the first learned call of a
    fresh batch (the members' initial bounds) and the step's remainder (torch's side: allocation, clones, autograd).

Member sets: those of tools/grad_small_time.py — 32 x the 8 x 8 assignment problem, and the 20-member float set of
tests/test_gpu_small_learned.py (17 members in double).  Host wall clock; every sample is a process of its own under `timeout`, tree and
parent alternating on the same device; a process builds its members, makes one warm-up call per case and times the next.
Writes profiles/batch_costs_time.txt (or --out).  Usage: python3 tools/batch_costs_time.py --parent-lib PATH [--samples 5] [--out FILE]"""
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
NEW = ("bddmma_set_solver_costs_batch", "bddmma_get_solver_costs_batch", "bddmma_stream_wait_batch", "bddmma_stream_signal_batch")
ITERS, TRACKED = 20, 5
CHILD_LIMIT = 240   # seconds


def as_the_parent(bdd_hip_batch):
    """the four batch methods as the loops the parent commit's DualIterations made in their place"""
    def parts(b, arrays):
        off = 0
        for s in b.solvers:
            n = s.nr_layers()
            yield s, [x[off:off + n] for x in arrays]
            off += n

    def set_solver_costs(b, lo, hi, mm):
        for s, (l, h, m) in parts(b, (lo, hi, mm)):
            s.set_solver_costs(l, h, m)

    def get_solver_costs(b, out=None):
        for s, o in parts(b, out):
            s.get_solver_costs(out=o)
        return out

    def stream_wait(b, hip_stream=0):
        for s in b.solvers:
            s.stream_wait(hip_stream)

    def stream_signal(b, hip_stream=0):
        for s in b.solvers:
            s.stream_signal(hip_stream)

    for f in (set_solver_costs, get_solver_costs, stream_wait, stream_signal):
        setattr(bdd_hip_batch, f.__name__, f)


def child(mode, lib):
    import numpy as np
    import torch
    from bdd_amd import capi
    from bdd_amd.solver import bdd_hip_batch, bdd_hip_parallel_mma
    if mode == "parent":
        capi.LIB_PATH = lib
        for name in NEW:
            capi.SIGNATURES.pop(name, None)   # a build of the parent commit does not export them
        as_the_parent(bdd_hip_batch)
    from bdd_amd.autograd import DualIterations
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

    def timed(f, warm=1):
        for _ in range(warm):
            f()
        t0 = time.perf_counter()
        f()
        return (time.perf_counter() - t0) * 1e3

    res = {}
    cat = np.concatenate
    for which in ("assign8x32", "mixed_set"):
        for precision in ("float", "double"):
            ms = members_of(which, precision)
            assert all(s.fused_small_learned() for s in ms)
            dt = ms[0].value_type
            tdt = torch.float64 if precision == "double" else torch.float32
            rng = np.random.default_rng(5)
            w = [dirichlet_weights(s, rng) for s in ms]
            g = [[rng.normal(0, 1, s.nr_layers()).astype(dt) for s in ms] for _ in range(3)]
            batch = bdd_hip_batch(ms)
            costs = [s.get_solver_costs() for s in ms]
            lo, hi = (cat([c[k] for c in costs]) for k in range(2))
            t = [torch.tensor(v, dtype=tdt, device="cuda", requires_grad=True) for v in (lo, hi, np.zeros_like(lo), cat(w), np.asarray([0.5], dt))]
            go = [torch.tensor(cat(a), dtype=tdt, device="cuda") for a in g]
            src = [x.detach() for x in t[:3]]
            out = [torch.empty_like(x) for x in src]
            off = np.cumsum([0] + [s.nr_layers() for s in ms])
            key = f"{which} {precision}"

            def sync():
                for s in ms:
                    s.synchronize()
                torch.cuda.synchronize()

            def batch_sync():
                batch.stream_signal(torch.cuda.current_stream().cuda_stream)
                torch.cuda.synchronize()

            # ---- (a)
            def loop_round_trip():
                for i, s in enumerate(ms):
                    sl = slice(off[i], off[i + 1])
                    s.set_solver_costs(*(x[sl] for x in src))
                for i, s in enumerate(ms):
                    sl = slice(off[i], off[i + 1])
                    s.get_solver_costs(out=tuple(x[sl] for x in out))
                sync()

            res[f"{key} set + get, loop"] = timed(loop_round_trip)
            if mode == "tree":
                def batch_round_trip():
                    batch.set_solver_costs(*src)
                    batch.get_solver_costs(out=out)
                    batch_sync()

                res[f"{key} set + get, batch"] = timed(batch_round_trip)

            # ---- (b)
            def step():
                o = DualIterations.apply(batch, *t[:4], ITERS, t[4], TRACKED, 0.0, 1, 0, 0.9)
                torch.autograd.backward(o[:3], go)
                torch.cuda.synchronize()

            res[f"{key} DualIterations step"] = timed(step)
            # ---- (c)
            if mode == "tree":
                gr = [x.clone() for x in go]
                gw, gom = torch.zeros_like(src[0]), torch.zeros(len(ms), dtype=tdt, device="cuda")
                wt = t[3].detach()
                calls = [("set", lambda: batch.set_solver_costs(*src)),
                         ("learned_iterations", lambda: batch.learned_iterations(wt, ITERS, omega=0.5)),
                         ("get", lambda: batch.get_solver_costs(out=out)),
                         ("grad_iterations", lambda: batch.grad_iterations(wt, *gr, omega=0.5, track_grad_after_itr=ITERS - TRACKED,
                                                                           track_grad_for_num_itr=TRACKED, out=(gw, gom)))]
                total = 0.0
                for name, f in calls:
                    ms_ = timed(lambda: (f(), batch_sync()))
                    res[f"{key} step part: {name}"] = ms_
                    total += ms_ * (2 if name == "set" else 1)
                res[f"{key} step part: remainder"] = res[f"{key} DualIterations step"] - total
                fresh = [bdd_hip_parallel_mma(*instance("assign8", 1), precision=precision) for _ in range(len(ms))] if which == "assign8x32" else None
                if fresh is not None:   # the first learned call of a batch: every member's two bounds for its initial change
                    fb = bdd_hip_batch(fresh)
                    fb.set_solver_costs(*src)
                    fb.learned_iterations(wt, 1, omega=0.5)   # the buffers and the kernels' first launch
                    fresh2 = [bdd_hip_parallel_mma(*instance("assign8", 1), precision=precision) for _ in range(len(ms))]
                    fb2 = bdd_hip_batch(fresh2)
                    fb2.set_solver_costs(*src)
                    fb2.stream_signal(torch.cuda.current_stream().cuda_stream)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fb2.learned_iterations(wt, ITERS, omega=0.5)
                    fb2.stream_signal(torch.cuda.current_stream().cuda_stream)
                    torch.cuda.synchronize()
                    res[f"{key} step part: learned_iterations, first call of a batch"] = (time.perf_counter() - t0) * 1e3
                    fb.close(), fb2.close()
                    for s in fresh + fresh2:
                        s.close()
            batch.close()
            for s in ms:
                s.close()
    print("RESULT " + json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_costs_time.txt"))
    ap.add_argument("--samples", type=int, default=5)
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--child", default="")
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.parent_lib)
    modes = ("tree", "parent") if a.parent_lib else ("tree",)
    samples = {m: [] for m in modes}
    for _ in range(a.samples):
        for mode in modes:
            cmd = ["timeout", "-k", "10", str(CHILD_LIMIT), sys.executable, os.path.abspath(__file__), "--child", mode]
            if mode == "parent":
                cmd += ["--parent-lib", os.path.abspath(a.parent_lib)]
            out = subprocess.run(cmd, capture_output=True, text=True)
            if out.returncode != 0:   # no further process on the device behind a failed one
                sys.exit(f"{mode} process failed ({out.returncode}):\n{out.stdout[-2000:]}\n{out.stderr[-2000:]}")
            samples[mode].append(json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:]))
    med = {m: {k: statistics.median(s[k] for s in samples[m]) for k in samples[m][0]} for m in modes}
    low = {m: {k: min(s[k] for s in samples[m]) for k in samples[m][0]} for m in modes}
    sets = [k[:-len(" set + get, loop")] for k in med["tree"] if k.endswith(" set + get, loop")]
    lines = [f"# tools/batch_costs_time.py --samples {a.samples}" + (" --parent-lib <a build of the parent commit>" if a.parent_lib else ""),
             f"# host wall clock in ms; {a.samples} samples each, one process per sample, tree and parent alternating; median (minimum)", "",
             "# (a) set + get round trip, device tensors, first call to everything synchronised: one batch call each way against the loop of",
             "#     per-member calls (tree's library)",
             f"{'members':24s} {'batch':>18s} {'loop':>18s} {'loop/batch':>11s}"]
    for k in sets:
        b, l = f"{k} set + get, batch", f"{k} set + get, loop"
        lines.append(f"{k:24s} {med['tree'][b]:9.3f} ({low['tree'][b]:6.3f}) {med['tree'][l]:9.3f} ({low['tree'][l]:6.3f}) {med['tree'][l] / med['tree'][b]:11.2f}")
    if a.parent_lib:
        lines += ["", f"# (b) one DualIterations forward + backward step on the batch, {ITERS} iterations, the last {TRACKED} tracked: the tree against the parent",
                  "#     commit's library and calls (per-member stream_wait, set_solver_costs, get_solver_costs, stream_signal)",
                  f"{'members':24s} {'tree':>18s} {'parent':>18s} {'parent/tree':>11s}"]
        for k in sets:
            c = f"{k} DualIterations step"
            lines.append(f"{k:24s} {med['tree'][c]:9.3f} ({low['tree'][c]:6.3f}) {med['parent'][c]:9.3f} ({low['parent'][c]:6.3f}) {med['parent'][c] / med['tree'][c]:11.2f}")
    lines += ["", "# (c) where the tree's step goes: each batch call alone, synchronised behind it (set is made twice per step); remainder = the step minus",
              "#     those (torch's side: five empty_like / zeros, three clones, the autograd graph, the final synchronisation; negative where",
              "#     the calls overlap inside the step).  first call of a batch: learned_iterations on fresh members, whose initial bound change",
              "#     is still unset (two bounds per member, fetched by the host)"]
    for k in med["tree"]:
        if " step part: " in k:
            lines.append(f"{k:72s} {med['tree'][k]:9.3f} ({low['tree'][k]:6.3f})")
    text = "\n".join(lines) + "\n"
    with open(a.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
