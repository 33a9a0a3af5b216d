"""Batches of one-workgroup instances (include/bdd_mma.h: bddmma_batch_*; kernels/small.hpp: k_iterate_small_batch): one workgroup per
member in one launch per kernel instantiation, against THE SAME INSTANCE IN A SECOND HANDLE DRIVEN ALONE through bddmma_iterations /
bddmma_run_solver (that path is pinned to the oracle by test_gpu_small_fused.py).

The batch kernel calls the same device function as k_iterate_small, so every comparison is bit-equal, in float and in double: arc costs,
deferred differences, lower bound, min-marginals.  The member set reaches every instantiation group (1, 2, 4, 8 and 16 waves; records in
LDS or not) with the smallest shapes that do so."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from bdd_amd import capi, to_bdd_collection  # noqa: E402
from bdd_amd.instances import assignment_ilp, random_set_cover  # noqa: E402
from bdd_amd.solver import bdd_hip_batch, bdd_hip_lbfgs, bdd_hip_parallel_mma, run_solver  # noqa: E402

SEQ = 0x80000   # variant_flags bit 19: four launches per iteration (not fused_small)

# (name, packs, precisions it is fused in, cost seeds)
SHAPES = [("assign3", 1, ("float", "double"), (0, 1, 2)),
          ("assign8", 1, ("float", "double"), (0, 1, 2, 3)),
          ("cover40x60", 2, ("float", "double"), (0, 1, 2)),
          ("cover67x100", 4, ("float", "double"), (0, 1, 2, 3)),
          ("cover147x220", 7, ("float", "double"), (0, 1, 2)),
          ("cover200x300", 10, ("float",), (0, 1, 2))]   # 10 packs: 16 waves, the records do not fit the LDS beside the state
_INSTANCES = {}


def instance(name, seed):
    """the shape's BDDs (built once) and the costs of `seed` (seed 0: the generator's own)"""
    if name not in _INSTANCES:
        if name.startswith("assign"):
            ilp = assignment_ilp(int(name[6:]))
            _INSTANCES[name] = (to_bdd_collection(ilp), np.asarray(ilp.objective, dtype=np.float64))
        else:
            v, r = (int(x) for x in name[5:].split("x"))
            _INSTANCES[name] = random_set_cover(v, r, {60: 5, 100: 7, 220: 8, 300: 9}[r], seed=r)
    col, costs = _INSTANCES[name]
    if seed:
        costs = costs * np.random.default_rng(1000 + seed).uniform(0.5, 1.5, size=costs.shape)
    return col, costs


def member_set(precision):
    """[(name, packs, solver, twin)]: about 20 members, shapes interleaved so that no group is contiguous in the caller's order"""
    out = []
    for seed_pos in range(4):
        for name, packs, fused_in, seeds in SHAPES:
            if precision in fused_in and seed_pos < len(seeds):
                col, costs = instance(name, seeds[seed_pos])
                out.append((name, packs, bdd_hip_parallel_mma(col, costs, precision=precision), bdd_hip_parallel_mma(col, costs, precision=precision)))
    for name, packs, s, t in out:   # a layout change must not silently empty a group
        assert s.nr_packs() == packs and s.fused_small() and t.fused_small(), (name, s.nr_packs(), s.fused_small())
    return out


def same_state(a, b, what=""):
    for x, y in zip(a.get_solver_costs(), b.get_solver_costs()):
        np.testing.assert_array_equal(x, y, err_msg=what)
    assert a.lower_bound() == b.lower_bound(), what


def snapshot(solvers):
    return [[x.copy() for x in s.get_solver_costs()] for s in solvers]


def assert_unchanged(solvers, snap):
    for s, before in zip(solvers, snap):
        for x, y in zip(s.get_solver_costs(), before):
            np.testing.assert_array_equal(x, y)


def refused(rc, make):
    with pytest.raises(capi.BddMmaError, match=f"error {rc}:") as e:
        make()
    return str(e.value)


@pytest.mark.parametrize("precision", ["float", "double"])
def test_batch_iterations_equal_each_member_driven_alone(precision):
    ms = member_set(precision)
    assert len(ms) == (20 if precision == "float" else 17)
    assert {p for _, p, _, _ in ms} == ({1, 2, 4, 7, 10} if precision == "float" else {1, 2, 4, 7})   # 1, 2, 4, 8 and 16 waves
    batch = bdd_hip_batch([s for _, _, s, _ in ms])
    assert len(batch) == len(ms)
    np.testing.assert_array_equal(batch.lower_bounds(), [t.lower_bound() for _, _, _, t in ms])
    for k in (1, 2, 17):
        for call in range(2):
            batch.iterations(k)
            for name, _, s, t in ms:
                t.iterations(k)
                same_state(s, t, f"{name}, {k} iterations, call {call}")
    lbs = batch.lower_bounds()
    for i, (name, _, s, t) in enumerate(ms):
        assert lbs[i] == s.lower_bound() == t.lower_bound(), name
        for a, b in zip(s.min_marginals(), t.min_marginals()):
            np.testing.assert_array_equal(a, b, err_msg=name)
    batch.iterations(0)   # nothing, as bddmma_iterations(s, omega, 0)
    batch.iterations(3, omega=0.3)
    for name, _, s, t in ms:
        t.iterations(3, omega=0.3)
        same_state(s, t, name)
    batch.close()


@pytest.mark.parametrize("precision", ["float", "double"])
def test_batch_of_one_member(precision):
    col, costs = instance("assign8", 1)
    s, t = (bdd_hip_parallel_mma(col, costs, precision=precision) for _ in range(2))
    batch = bdd_hip_batch([s])
    assert len(batch) == 1
    for k in (1, 5):
        batch.iterations(k)
        t.iterations(k)
        same_state(s, t)
    assert batch.lower_bounds()[0] == t.lower_bound()
    batch.close()


@pytest.mark.parametrize("precision", ["float", "double"])
def test_batch_calls_interleaved_with_per_member_calls(precision):
    """The ordering contract and the state flags: a batch call is ordered after what is queued on every member's stream (update_costs, a
    member's own iteration) and what a member does afterwards is ordered after it; a member whose costs-to-terminal are stale gets its
    backward run first."""
    ms = member_set(precision)
    batch = bdd_hip_batch([s for _, _, s, _ in ms])
    rng = np.random.default_rng(5)
    batch.iterations(3)
    for i, (_, _, s, t) in enumerate(ms):
        t.iterations(3)
        if i % 3 == 0:      # costs change: both sweep states are stale when the batch runs next
            d = rng.uniform(-0.5, 0.5, size=s.nr_variables())
            s.update_costs([], d)
            t.update_costs([], d)
        elif i % 3 == 1:    # a member's own launch, queued right in front of the batch's
            s.iteration()
            t.iteration()
    batch.iterations(4)
    for i, (name, _, s, t) in enumerate(ms):
        t.iterations(4)
        if i % 2 == 0:      # ... and right behind it, without the host having waited
            s.iteration()
            t.iteration()
    for name, _, s, t in ms:
        same_state(s, t, name)
    batch.iterations(2)
    for name, _, s, t in ms:
        t.iterations(2)
        s.distribute_delta()   # folds the pending pairs and the deferred differences into the arc costs: both were written back
        t.distribute_delta()
        same_state(s, t, name)
    batch.iterations(1)
    for name, _, s, t in ms:
        t.iterations(1)
        same_state(s, t, name)
    batch.close()


# 12 x 12 assignment problems with random costs (every variable sits in two BDDs): uniform costs, whose runs end within the first chunk of
# 64 iterations at different iterations, and integer costs with a small perturbation (near-ties), which converge more slowly — the CPU
# oracle's loop ends after 122 / 179 iterations (tolerance / slope) for seed 10 and after 71 / 85 for seed 13, in later chunks
RUN_MEMBERS = (("uniform", 8), ("integer", 10), ("uniform", 1), ("uniform", 4), ("integer", 13), ("uniform", 5))


def run_members(precision):
    out = []
    for kind, seed in RUN_MEMBERS:
        rng = np.random.default_rng(seed)
        if kind == "uniform":
            costs = rng.uniform(-3.0, 1.0, size=(12, 12))
        else:
            costs = rng.integers(-3, 2, size=(12, 12)).astype(float) + rng.uniform(0, 1e-3, size=(12, 12))
        ilp = assignment_ilp(12, costs)
        col = to_bdd_collection(ilp)
        out.append((bdd_hip_parallel_mma(col, ilp.objective, precision=precision), bdd_hip_parallel_mma(col, ilp.objective, precision=precision)))
    assert all(s.fused_small() and t.fused_small() for s, t in out)
    return out


@pytest.mark.parametrize("precision", ["float", "double"])
@pytest.mark.parametrize("case", [dict(max_iter=1000, tolerance=1e-4, slope=0.0), dict(max_iter=1000, tolerance=0.0, slope=0.02),
                                  dict(max_iter=23, tolerance=0.0, slope=0.0), dict(max_iter=129, tolerance=0.0, slope=0.0)],
                         ids=["tolerance", "slope", "max_iter_23", "max_iter_129_two_chunks_and_one"])
def test_batch_run_solver_equals_each_member_run_alone(precision, case):
    ms = run_members(precision)
    batch = bdd_hip_batch([s for s, _ in ms])
    res = batch.run_solver(max_iter=case["max_iter"], tolerance=case["tolerance"], improvement_slope=case["slope"], time_limit=1e9)
    assert len(res) == len(ms)
    iters = []
    for r, (s, t) in zip(res, ms):
        q = run_solver(t, max_iter=case["max_iter"], tolerance=case["tolerance"], improvement_slope=case["slope"], time_limit=1e9)
        assert (r["iterations"], r["stop_reason"], r["lb_initial"], r["lb_final"]) == (q["iterations"], q["stop_reason"], q["lb_initial"], q["lb_final"])
        assert r["seconds"] == res[0]["seconds"]        # the batch's wall time
        same_state(s, t)                                 # nothing ran behind the iteration that met the member's criterion
        assert s.lower_bound() == r["lb_final"]
        iters.append(r["iterations"])
    if case["tolerance"] or case["slope"]:
        assert all(r["stop_reason"] in (2, 3) and r["iterations"] < case["max_iter"] for r in res)
        assert len(set(iters)) > 1                       # the members stop on their own criteria
        assert len({(n - 1) // 64 for n in iters}) > 1, iters   # ... and at least two of them in different chunks
    else:
        assert iters == [case["max_iter"]] * len(ms) and all(r["stop_reason"] == 0 for r in res)
    batch.iterations(1)   # the batch goes on from the state run_solver left
    for s, t in ms:
        t.iteration()
        same_state(s, t)
    batch.close()


def test_refusals_leave_every_member_untouched():
    col8, c8 = instance("assign8", 0)
    colc, cc = instance("cover40x60", 0)
    a = bdd_hip_parallel_mma(col8, c8, precision="float")
    b = bdd_hip_parallel_mma(colc, cc, precision="float")
    dbl = bdd_hip_parallel_mma(col8, c8, precision="double")
    seq = bdd_hip_parallel_mma(col8, c8, precision="float", variant_flags=SEQ)
    everyone = [a, b, dbl, seq]
    for s in everyone:
        s.iterations(2)
    snap = snapshot(everyone)
    assert not seq.fused_small()
    msg = refused(capi.ERR_UNSUPPORTED, lambda: bdd_hip_batch([a, seq, b]))
    assert "member 1" in msg and "fused_small" in msg
    msg = refused(capi.ERR_UNSUPPORTED, lambda: bdd_hip_batch([a, b, dbl]))
    assert "member 2" in msg and "precision" in msg
    msg = refused(capi.ERR_INVALID_ARGUMENT, lambda: bdd_hip_batch([a, b, a]))
    assert "member 2" in msg and "twice" in msg
    refused(capi.ERR_INVALID_ARGUMENT, lambda: bdd_hip_batch([]))
    assert_unchanged(everyone, snap)

    # an L-BFGS wrapper attached to a member: at creation ...
    wrapper = bdd_hip_lbfgs(b)
    snap = snapshot(everyone)
    msg = refused(capi.ERR_STATE, lambda: bdd_hip_batch([a, b]))
    assert "member 1" in msg and "L-BFGS" in msg
    assert_unchanged(everyone, snap)
    wrapper.close()

    # ... and when it is attached after creation: every call is refused before anything is launched
    a2 = bdd_hip_parallel_mma(col8, c8, precision="float")
    b2 = bdd_hip_parallel_mma(colc, cc, precision="float")
    batch = bdd_hip_batch([a2, b2])
    batch.iterations(2)
    wrapper = bdd_hip_lbfgs(b2)
    snap = snapshot([a2, b2])
    msg = refused(capi.ERR_STATE, lambda: batch.iterations(3))
    assert "member 1" in msg and "L-BFGS" in msg
    refused(capi.ERR_STATE, lambda: batch.run_solver(max_iter=5))
    assert_unchanged([a2, b2], snap)
    # profiling on a member: the same
    a2.set_profiling(True)
    msg = refused(capi.ERR_STATE, lambda: batch.iterations(1))
    assert "member 0" in msg and "profiling" in msg
    a2.set_profiling(False)
    assert_unchanged([a2, b2], snap)
    batch.close()
    wrapper.close()
