#!/usr/bin/env python3
"""Learned iterations of one-workgroup instances: the fused kernel (k_learned_small) against another build's four launches per iteration,
batches against a loop over their members, and DualIterations.forward on a batch against the list of its members.

(a) per handle   assign8 and cover67x100, float and double: learned_iterations(w, ITERS, 0.5, improvement_slope=0.0) and the same with an
                 omega_vec.  With --parent ROOT (a checkout of the parent commit with its library built) the same calls run in a second
                 process on that tree, the two processes alternating sample by sample; criterion: this tree's median <= half the other's
                 fastest sample.
(b) batch        the 20-member float set of tests/test_gpu_batch_small.py: one batch.learned_iterations of ITERS iterations against the same
                 members looped through learned_iterations; criterion: the batch is faster than the loop's fastest sample.
(c) autograd     DualIterations.forward on that batch against the list, 20 iterations; recorded, no criterion (set_solver_costs /
                 get_solver_costs still synchronise per member).
Every time is a host clock around work that ends in synchronize(); SAMPLES samples per side after one warm-up call per shape.
Writes profiles/learned_small_time.txt (or --out); exits 1 when a criterion is missed.
Usage: python3 tools/learned_small_time.py [--parent ROOT] [--out FILE] [--iters 1000] [--samples 5]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HANDLE_SHAPES = ("assign8", "cover67x100")
BATCH_SHAPES = [("assign3", (0, 1, 2)), ("assign8", (0, 1, 2, 3)), ("cover40x60", (0, 1, 2)), ("cover67x100", (0, 1, 2, 3)),
                ("cover147x220", (0, 1, 2)), ("cover200x300", (0, 1, 2))]


def worker(root, iters):
    """answers each line on stdin with one JSON line: "a" -> {config: ms} of (a); "bc" -> (b) and (c) (this tree only)"""
    sys.path.insert(0, root)
    import numpy as np
    from bdd_amd import to_bdd_collection
    from bdd_amd.instances import assignment_ilp, random_set_cover
    from bdd_amd.solver import bdd_hip_parallel_mma

    made = {}

    def instance(name, seed):
        if name not in made:
            if name.startswith("assign"):
                ilp = assignment_ilp(int(name[6:]))
                made[name] = (to_bdd_collection(ilp), np.asarray(ilp.objective, dtype=np.float64))
            else:
                v, r = (int(x) for x in name[5:].split("x"))
                made[name] = random_set_cover(v, r, {60: 5, 100: 7, 220: 8, 300: 9}[r], seed=r)
        col, costs = made[name]
        if seed:
            costs = costs * np.random.default_rng(1000 + seed).uniform(0.5, 1.5, size=costs.shape)
        return col, costs

    def weights(s, rng):
        var = s.get_primal_variable_index()
        w = np.zeros(var.size)
        for v in np.unique(var):
            idx = np.flatnonzero(var == v)
            w[idx] = rng.dirichlet(np.ones(idx.size))
        return w.astype(s.value_type)

    def timed(f, sync):
        sync()
        t0 = time.perf_counter()
        f()
        sync()
        return (time.perf_counter() - t0) * 1e3

    rng = np.random.default_rng(1)
    handles = {}
    for name in HANDLE_SHAPES:
        for precision in ("float", "double"):
            s = bdd_hip_parallel_mma(*instance(name, 1), precision=precision)
            w = weights(s, rng)
            ov = rng.uniform(0.1, 0.9, s.nr_layers()).astype(s.value_type)
            for mode in ("omega", "omega_vec"):
                call = (lambda s=s, w=w: s.learned_iterations(w, iters, 0.5, improvement_slope=0.0)) if mode == "omega" else \
                       (lambda s=s, w=w, ov=ov: s.learned_iterations(w, iters, improvement_slope=0.0, omega_vec=ov))
                call()   # warm-up
                handles[f"{name} {precision} {mode}"] = (call, s.synchronize)
    extra = None
    print("ready", flush=True)
    for line in sys.stdin:
        what = line.strip()
        if what == "a":
            print(json.dumps({k: timed(c, sy) for k, (c, sy) in handles.items()}), flush=True)
        elif what == "bc":
            if extra is None:
                import torch
                from bdd_amd.autograd import DualIterations
                from bdd_amd.solver import bdd_hip_batch
                ms = [bdd_hip_parallel_mma(*instance(n, seeds[k]), precision="float") for k in range(4) for n, seeds in BATCH_SHAPES if k < len(seeds)]
                assert len(ms) == 20 and all(s.fused_small_learned() for s in ms)
                batch = bdd_hip_batch(ms)
                ws = [weights(s, rng) for s in ms]
                wcat = np.concatenate(ws)

                def sync_all():
                    for s in ms:
                        s.synchronize()

                def loop():
                    for s, w in zip(ms, ws):
                        s.learned_iterations(w, iters, 0.5, improvement_slope=0.0)

                costs = [s.get_solver_costs() for s in ms]
                t = [torch.tensor(np.concatenate([c[k] for c in costs]), device="cuda") for k in range(3)]
                t.append(torch.tensor(wcat, device="cuda"))
                om = torch.tensor([0.5], dtype=torch.float32, device="cuda")
                with torch.no_grad():
                    fwd = {k: (lambda sv=sv: DualIterations.apply(sv, *t, 20, om, 1, 0.0, 1, 0, 0.9)) for k, sv in (("batch", batch), ("list", ms))}
                    extra = {"batch": (lambda: batch.learned_iterations(wcat, iters), sync_all), "loop": (loop, sync_all),
                             "forward batch": (fwd["batch"], torch.cuda.synchronize), "forward list": (fwd["list"], torch.cuda.synchronize)}
                    for c, _ in extra.values():
                        c()   # warm-up
            import torch
            with torch.no_grad():
                print(json.dumps({k: timed(c, sy) for k, (c, sy) in extra.items()}), flush=True)
        else:
            break


class Side:
    def __init__(self, root, iters):
        env = dict(os.environ, PYTHONPATH=root)
        self.p = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--worker", root, "--iters", str(iters)], stdin=subprocess.PIPE,
                                  stdout=subprocess.PIPE, text=True, cwd=root, env=env)
        line = self.p.stdout.readline().strip()
        if line != "ready":
            raise RuntimeError(f"the worker on {root} did not start: {line!r}")

    def ask(self, what):
        self.p.stdin.write(what + "\n")
        self.p.stdin.flush()
        line = self.p.stdout.readline()
        if not line:
            raise RuntimeError("the worker ended")
        return json.loads(line)

    def close(self):
        self.p.stdin.close()
        self.p.wait(timeout=60)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "learned_small_time.txt"))
    ap.add_argument("--iters", type=int, default=1000)
    ap.add_argument("--samples", type=int, default=5)
    ap.add_argument("--worker", default=None)
    a = ap.parse_args()
    if a.worker:
        return worker(a.worker, a.iters) or 0
    head = Side(ROOT, a.iters)
    parent = Side(os.path.abspath(a.parent), a.iters) if a.parent else None
    sa = {"head": [], "parent": []}
    for _ in range(a.samples):   # alternating
        if parent:
            sa["parent"].append(parent.ask("a"))
        sa["head"].append(head.ask("a"))
    if parent:
        parent.close()
    sbc = [head.ask("bc") for _ in range(a.samples)]
    head.close()
    fmt = lambda xs: " ".join(f"{x:9.3f}" for x in xs)
    lines = [f"# tools/learned_small_time.py --iters {a.iters} --samples {a.samples}" + (" --parent <parent checkout>" if parent else ""),
             "# host clock around work that ends in synchronize(); ms per sample; a warm-up call per shape first; the sides alternate",
             f"# (a) learned_iterations(w, {a.iters}, 0.5, improvement_slope=0.0) per handle; criterion: head median <= parent fastest / 2"]
    missed = 0
    for k in sa["head"][0]:
        h = [s[k] for s in sa["head"]]
        lines.append(f"{k:30s} head   {fmt(h)}   median {statistics.median(h):9.3f}  = {statistics.median(h) / a.iters * 1e3:7.2f} us / iteration")
        if parent:
            p = [s[k] for s in sa["parent"]]
            ok = statistics.median(h) <= min(p) / 2
            missed += not ok
            lines.append(f"{'':30s} parent {fmt(p)}   fastest {min(p):8.3f}  = {min(p) / a.iters * 1e3:7.2f} us / iteration   "
                         f"parent fastest / head median {min(p) / statistics.median(h):5.2f}  {'ok' if ok else 'MISSED'}")
    b, lo = [s["batch"] for s in sbc], [s["loop"] for s in sbc]
    ok = statistics.median(b) < min(lo)
    missed += not ok
    lines += [f"# (b) 20 float members, {a.iters} iterations: batch.learned_iterations against the members looped; criterion: batch median < loop fastest",
              f"{'batch':30s}        {fmt(b)}   median {statistics.median(b):9.3f}",
              f"{'loop over the members':30s}        {fmt(lo)}   fastest {min(lo):8.3f}   loop fastest / batch median {min(lo) / statistics.median(b):5.2f}  {'ok' if ok else 'MISSED'}",
              "# (c) DualIterations.forward, the same 20 members, 20 iterations: a batch against the list (no criterion)"]
    for k in ("forward batch", "forward list"):
        x = [s[k] for s in sbc]
        lines.append(f"{k:30s}        {fmt(x)}   median {statistics.median(x):9.3f}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    return 1 if missed else 0


if __name__ == "__main__":
    sys.exit(main())
