"""The batch farm with fuse_small (bdd_amd/csrc/host/bdd_solver.hpp: solve_batch with batch_options; bdd_solver_cl --batch --fuse-small;
bdd_solver_py.solve_batch): instances that fit one workgroup and share their settings run as members of one batch, one launch per step
for all of them.  The batch API promises what the per-member calls give bit for bit, so a fused member's results are compared with the
unfused farm's by ==."""
import json
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from bdd_amd import bdd_solver_py  # noqa: E402
from bdd_amd.bdd_solver import bdd_solver  # noqa: E402
from bdd_amd.instances import GRID_3X3, LONG_CHAIN, assignment_ilp, mrf_ilp  # noqa: E402

EXE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bdd_amd", "csrc", "bdd_solver_cl")
TC = {"maximum iterations": 200, "improvement slope": 0.0, "minimum improvement": 0.0, "time limit": 1e10}
ROUNDING = {"initial perturbation": 0.1, "perturbation growth rate": 1.2, "inner iterations": 20, "outer iterations": 30, "seed": 3}
LOOSE = ("Minimize\nx1 + x2 + x3 + x4 + x5 + x6\nSubject To\nx1 + x2 + x4 >= 1\nx1 + x3 + x5 >= 1\nx2 + x3 + x6 >= 1\n"
         "Bounds\nBinaries\nx1\nx2\nx3\nx4\nx5\nx6\nEnd\n")
INFEASIBLE = "Minimize\nx\nSubject To\nx >= 2\nBounds\nBinaries\nx\nEnd\n"


def covering_lp(n_vars, n_rows, k, seed):
    rng = np.random.default_rng(seed)
    costs = rng.uniform(0.5, 2.0, n_vars)
    lines = ["Minimize", " + ".join(f"{c:.6f} x{v + 1}" for v, c in enumerate(costs)), "Subject To"]
    for _ in range(n_rows):
        lines.append(" + ".join(f"x{v + 1}" for v in sorted(rng.choice(n_vars, size=k, replace=False))) + " >= 1")
    lines += ["Bounds", "Binaries"] + [f"x{v + 1}" for v in range(n_vars)] + ["End", ""]
    return "\n".join(lines)


def cfg(lp, precision, rounding, solver="cuda parallel mma"):
    c = {"precision": precision, "relaxation solver": solver, "termination criteria": dict(TC), "input": lp}
    if rounding:
        c["perturbation rounding"] = dict(ROUNDING)
    return c


_CONFIGS = {}


def configs():
    """[(name, config dict, known bound or None)]: every shape in both precisions, every other config with rounding — four keys — then
    one L-BFGS config and one infeasible one"""
    if not _CONFIGS:
        rng = np.random.default_rng(71)
        shapes = [("assign3", assignment_ilp(3).write_lp(), -6.0), ("assign3b", assignment_ilp(3, rng.uniform(-3, 1, (3, 3))).write_lp(), None),
                  ("assign8", assignment_ilp(8).write_lp(), -16.0), ("assign8b", assignment_ilp(8, rng.uniform(-3, 1, (8, 8))).write_lp(), None),
                  ("chain", mrf_ilp(**LONG_CHAIN).write_lp(), -9.0), ("grid", mrf_ilp(**GRID_3X3).write_lp(), None), ("loose", LOOSE, 1.5),
                  ("cover67x100", covering_lp(67, 100, 7, 1), None), ("cover200x300", covering_lp(200, 300, 9, 2), None)]
        out = []
        for precision in ("double", "float"):
            for i, (name, lp, lb) in enumerate(shapes):
                out.append((f"{name}/{precision}", cfg(lp, precision, rounding=i % 2 == 1), lb))
        out.append(("lbfgs", cfg(assignment_ilp(8).write_lp(), "double", False, solver="lbfgs cuda mma"), -16.0))
        out.append(("infeasible", cfg(INFEASIBLE, "double", False), None))
        _CONFIGS["all"] = out
    return _CONFIGS["all"]


_RUNS = {}


def farm(**kw):
    key = tuple(sorted(kw.items()))
    if key not in _RUNS:
        _RUNS[key] = bdd_solver_py.solve_batch([json.dumps(c) for _, c, _ in configs()], quiet=True,
                                               **{k: (list(v) if isinstance(v, tuple) else v) for k, v in kw.items()})
    return _RUNS[key]


# An instance that comes back unfused ran the same per-instance code in both farms.  Where it needs more than one workgroup its default
# exchange sums a variable's differences with LDS atomics, in an order that changes from run to run (include/bdd_mma.h:
# bddmma_options.deterministic), so two runs of it — with or without the option — agree only up to that reordering: per iteration a sum of
# at most 64 terms reordered, 64 eps relative, over TC's 200 iterations.  Fused members are held to ==.
UNFUSED_REL = 200 * 64 * 2.0 ** -52


def assert_same_results(got, want):
    assert len(got) == len(want) == len(configs())
    for (name, c, _), g, w in zip(configs(), got, want):
        for k in ("ok", "lower_bound", "iterations", "has_primal", "primal"):
            if k == "lower_bound" and g["ok"] and not g["fused"] and not w["fused"]:
                assert c["precision"] == "double" and abs(g[k] - w[k]) <= UNFUSED_REL * abs(w[k]), (name, k, g[k], w[k])
                continue
            assert g[k] == w[k], (name, k, g[k], w[k])
        assert bool(g["error"]) == bool(w["error"]), (name, g["error"], w["error"])
        assert g["config"] == w["config"] and g["device"] == w["device"] == 0


def test_the_fused_farm_gives_the_unfused_farms_results():
    plain, fused = farm(fuse_small=False), farm(fuse_small=True)
    assert_same_results(fused, plain)
    assert len({bdd_solver_py.fuse_key(json.dumps(c)) for _, c, _ in configs()} - {""}) >= 4
    for (name, _, lb), r in zip(configs(), fused):
        print(name, r["ok"], r["fused"], r["lower_bound"], r["iterations"], r["has_primal"], r["primal"], f"{r['seconds']:.3f} s")
        assert r["ok"] == (name != "infeasible"), (name, r["error"])
        if lb is not None:   # the known answers, to the tolerances of tests/test_gpu_bdd_solver.py
            assert abs(r["lower_bound"] - lb) <= (1e-4 if name.endswith("float") or name.startswith("loose") else 1e-6), (name, r["lower_bound"])
    assert not any(r["fused"] for r in plain)
    assert any(r["has_primal"] for r in fused)


def test_fused_is_what_the_instance_alone_says_about_one_workgroup():
    fused = farm(fuse_small=True)
    packs = {}
    n_fused = 0
    for (name, c, _), r in zip(configs(), fused):
        if name in ("lbfgs", "infeasible"):
            assert not r["fused"], name
            continue
        alone = bdd_solver(dict(c), quiet=True).solve().solver
        assert r["fused"] == bool(alone.fused_small()), (name, r["fused"])
        if r["fused"]:
            n_fused += 1
            packs.setdefault(bdd_solver_py.fuse_key(json.dumps(c)), set()).add(alone.nr_packs())
    print(n_fused, packs)
    assert n_fused >= 12
    waves = lambda p: 1 if p <= 1 else 2 if p <= 2 else 4 if p <= 4 else 8 if p <= 8 else 16   # noqa: E731
    assert any(len({waves(p) for p in ps}) >= 2 for ps in packs.values()), packs   # a batch with two wave counts
    assert any(r["ok"] and not r["fused"] for r in fused)                              # a good config solved alone


def test_small_groups_flush_in_the_middle_of_the_queue():
    assert_same_results(farm(fuse_small=True, max_group=2), farm(fuse_small=False))
    assert [r["fused"] for r in farm(fuse_small=True, max_group=2)] == [r["fused"] for r in farm(fuse_small=True)]


def test_two_threads_on_one_device():
    assert_same_results(farm(fuse_small=True, devices=(0, 0)), farm(fuse_small=False))


def test_command_line_flag(tmp_path):
    paths = []
    for i, (_, c, _) in enumerate(configs()):
        p = tmp_path / f"c{i}.json"
        p.write_text(json.dumps(c))
        paths.append(str(p))
    out = subprocess.run([EXE, "--batch", *paths, "--fuse-small", "--devices", "0", "--quiet"], capture_output=True, text=True, timeout=300)
    rows = [json.loads(l) for l in out.stdout.splitlines() if l.startswith("{")]
    assert out.returncode == 1, out.stderr          # the infeasible config
    assert len(rows) == len(paths) and all("fused" in r for r in rows)
    want = farm(fuse_small=True)
    for r, w, p in zip(rows, want, paths):
        assert r["config"] == p and r["ok"] == w["ok"] and r["fused"] == w["fused"] and r["iterations"] == w["iterations"]
        assert r["lower_bound"] == float(f"{w['lower_bound']:.12g}")
    out = subprocess.run([EXE, "--batch", *paths[:3], paths[-1], "--devices", "0", "--quiet"], capture_output=True, text=True, timeout=300)
    rows = [json.loads(l) for l in out.stdout.splitlines() if l.startswith("{")]
    assert out.returncode == 1 and len(rows) == 4 and not any("fused" in r for r in rows)
