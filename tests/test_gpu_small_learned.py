"""Learned MMA iterations inside the one-workgroup kernel (kernels/small.hpp: k_learned_small, k_learned_small_batch; include/bdd_mma.h:
bddmma_fused_small_learned, bddmma_learned_iterations_batch) on the MI355X.

The reference of every comparison is THE SAME INSTANCE IN A SECOND HANDLE ON THE FOUR-LAUNCH PATH (variant_flags bit 19), which
tests/test_gpu_learned_mma.py pins to the NumPy restatement, or — for batches — a second handle driven alone through learned_iterations.
Tolerances: bit-equal in float (the exchange's double sum of floats is exact) and in double wherever every variable sits in two BDDs
(assign*); ISO_TOL's 1e-12 relative in double on cover*, where the fused exchange adds a variable's terms in another order than the LDS
atomics of the four-launch exchange.  Batches are bit-equal in both precisions: the batch kernel calls the per-handle kernel's device function.

The shapes are those of tests/test_gpu_batch_small.py (1, 2, 4, 8 and 16 waves; records in LDS and not) and the 9 x 9 assignment problem:
81 variables on one pack of one wave, so the exchange's strided variable loop runs in its weighted form."""
import os
import tempfile

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from bdd_amd import capi, to_bdd_collection  # noqa: E402
from bdd_amd.instances import assignment_ilp, random_set_cover  # noqa: E402
from bdd_amd.solver import bdd_hip_batch, bdd_hip_lbfgs, bdd_hip_parallel_mma  # noqa: E402
from learned_mma_restatement import LearnedMma  # noqa: E402
from util import load_golden, pad_costs  # noqa: E402

SEQ = 0x80000   # variant_flags bit 19: four launches per iteration (neither fused_small nor fused_small_learned)
ISO_TOL = {"double": 1e-12, "float": 1e-5}        # tests/test_gpu_learned_mma.py: tier 1
REF_TOL = {"double": 1e-9, "float": 1e-5}         # against the restatement

# (name, packs, precisions it is fused in, cost seeds): tests/test_gpu_batch_small.py's, + assign9
SHAPES = [("assign3", 1, ("float", "double"), (0, 1, 2)),
          ("assign8", 1, ("float", "double"), (0, 1, 2, 3)),
          ("cover40x60", 2, ("float", "double"), (0, 1, 2)),
          ("cover67x100", 4, ("float", "double"), (0, 1, 2, 3)),
          ("cover147x220", 7, ("float", "double"), (0, 1, 2)),
          ("cover200x300", 10, ("float",), (0, 1, 2))]   # 10 packs: 16 waves, the records do not fit the LDS beside the state
ASSIGN9 = ("assign9", 1, ("float", "double"), (0,))     # 81 variables > the 64 threads of its one wave
CASES = [(name, precision) for name, _, fused_in, _ in SHAPES + [ASSIGN9] for precision in fused_in]
PACKS = {name: packs for name, packs, _, _ in SHAPES + [ASSIGN9]}
_INSTANCES = {}


def instance(name, seed):
    """the shape's BDDs (built once) and the costs of `seed` (seed 0: the generator's own)"""
    if name not in _INSTANCES:
        if name.startswith("assign"):
            ilp = assignment_ilp(int(name[6:]))
            _INSTANCES[name] = (to_bdd_collection(ilp), np.asarray(ilp.objective, dtype=np.float64))
        else:
            v, r = (int(x) for x in name[5:].split("x"))
            _INSTANCES[name] = random_set_cover(v, r, {60: 5, 100: 7, 220: 8, 240: 8, 300: 9}[r], seed=r)
    col, costs = _INSTANCES[name]
    if seed:
        costs = costs * np.random.default_rng(1000 + seed).uniform(0.5, 1.5, size=costs.shape)
    return col, costs


def fused_and_sequential(name, precision, seed=1):
    """handle f on the fused path and its twin q on the four-launch path; the preconditions of every case are asserted first, so that a
    layout change surfaces as a failed precondition and not as an empty test"""
    col, costs = instance(name, seed)
    f = bdd_hip_parallel_mma(col, costs, precision=precision)
    q = bdd_hip_parallel_mma(col, costs, precision=precision, variant_flags=SEQ)
    assert f.nr_packs() == PACKS[name], (name, f.nr_packs())
    assert f.fused_small() and f.fused_small_learned(), (name, f.fused_small(), f.fused_small_learned())
    assert not q.fused_small() and not q.fused_small_learned()
    if name == "assign9":
        assert f.nr_variables() == 81 > 64 * 1
    return f, q


def dirichlet_weights(s, rng, normalised=True):
    var = s.get_primal_variable_index()
    if not normalised:
        return rng.uniform(0.0, 0.8, var.size).astype(s.value_type)
    w = np.zeros(var.size)
    for v in np.unique(var):
        idx = np.flatnonzero(var == v)
        w[idx] = rng.dirichlet(np.ones(idx.size))
    return w.astype(s.value_type)


def state(s):
    return list(s.get_solver_costs()) + [s.get_delta(), np.float64(s.lower_bound())]


def assert_same(a, b, rel, what=""):
    """rel = 0: bit-equal; otherwise relative to the larger of 1 and the reference's largest magnitude, as tests/test_gpu_learned_mma.py"""
    for x, y, nm in zip(state(a), state(b), ("lo", "hi", "deferred mm", "delta", "lower bound")):
        if rel == 0:
            np.testing.assert_array_equal(x, y, err_msg=f"{what} {nm}")
        else:
            y64 = np.asarray(y, np.float64)
            scale = max(1.0, float(np.abs(y64).max()))
            np.testing.assert_allclose(np.asarray(x, np.float64), y64, rtol=rel, atol=rel * scale, err_msg=f"{what} {nm}")


def tolerance(name, precision):
    return 0 if precision == "float" or name.startswith("assign") else ISO_TOL[precision]


# ---------------------------------------------------------------- 1. fused against four launches
@pytest.mark.parametrize("name,precision", CASES)
def test_fused_learned_equals_the_four_launch_path(name, precision):
    rel = tolerance(name, precision)
    rng = np.random.default_rng(11)
    for mode in (0.5, 0.3, "omega_vec"):
        f, q = fused_and_sequential(name, precision)
        if name.startswith("cover"):
            assert f.get_num_bdds_per_var().max() > 4   # a variable the exchange serves from its generic loop, not from registers
        else:
            assert set(f.get_num_bdds_per_var()) == {2}
        w = dirichlet_weights(f, rng, normalised=not (name == "cover40x60" and mode == 0.3))   # one case with un-normalised weights
        args = dict(omega_vec=rng.uniform(0.1, 0.9, f.nr_layers()).astype(f.value_type)) if mode == "omega_vec" else dict(omega=mode)
        for n in (1, 2, 17):
            for call in range(2):
                assert f.learned_iterations(w, n, improvement_slope=0.0, **args) == n
                assert q.learned_iterations(w, n, improvement_slope=0.0, **args) == n
                assert_same(f, q, rel, f"{name} {precision} {mode}: {n} iterations, call {call}")


@pytest.mark.parametrize("name,precision", CASES)
def test_omega_vec_of_one_value_is_the_scalar_call_bit_for_bit(name, precision):
    col, costs = instance(name, 2 if name != "assign9" else 0)
    a, b = (bdd_hip_parallel_mma(col, costs, precision=precision) for _ in range(2))
    assert a.fused_small_learned() and b.fused_small_learned()
    w = dirichlet_weights(a, np.random.default_rng(12))
    for n in (1, 5):
        a.learned_iterations(w, n, 0.5, improvement_slope=0.0)
        b.learned_iterations(w, n, improvement_slope=0.0, omega_vec=np.full(a.nr_layers(), 0.5, a.value_type))
        assert_same(a, b, 0, f"{name} {precision} {n}")


# ---------------------------------------------------------------- 2. against the NumPy restatement
@pytest.mark.parametrize("name,precision", CASES)
def test_six_fused_iterations_in_one_launch_vs_restatement(name, precision):
    col, costs = instance(name, 1 if name != "assign9" else 0)
    s = bdd_hip_parallel_mma(col, costs, precision=precision)
    assert s.nr_packs() == PACKS[name] and s.fused_small() and s.fused_small_learned()
    m = LearnedMma(col.instr, col.delims, precision)
    m.update_costs_hi(np.asarray(costs, np.float64))
    perm = s.bdd_major_order()
    np.testing.assert_array_equal(m.layer_var, s.get_primal_variable_index()[perm])
    w = dirichlet_weights(s, np.random.default_rng(13))
    # one call: the first iteration is a launch of its own (the set-once initial bound change), iterations 2 to 6 stay inside one launch
    assert s.learned_iterations(w, 6, 0.5, improvement_slope=0.0) == 6
    for _ in range(6):
        m.learned_iteration(w[perm], 0.5)
    rel = REF_TOL[precision]
    lo, hi, mm = s.get_solver_costs()
    for x, y, nm in ((lo[perm], m.lo, "lo"), (hi[perm], m.hi, "hi"), (mm[perm], m.mm, "deferred mm")):
        y = np.asarray(y, np.float64)
        np.testing.assert_allclose(np.asarray(x, np.float64), y, rtol=rel, atol=rel * max(1.0, float(np.abs(y).max())), err_msg=nm)
    lb, ref = s.lower_bound(), m.lower_bound()
    assert abs(lb - ref) <= rel * max(1.0, abs(ref)), (lb, ref)


# ---------------------------------------------------------------- 3. state hand-over on the fused path
HANDOVER = [("assign8", "float"), ("assign8", "double"), ("cover67x100", "float"), ("cover67x100", "double"), ("cover200x300", "float")]


@pytest.mark.parametrize("name,precision", HANDOVER)
def test_plain_learned_plain_equals_plain(name, precision):
    f, q = fused_and_sequential(name, precision)
    f.iterations(2)              # a pending isotropic delta at entry: the learned iterations ignore it
    f.learned_iterations(f.get_isotropic_dist_weights(), 4, 0.5, improvement_slope=0.0)
    f.iterations(3)
    q.iterations(9)
    assert_same(f, q, ISO_TOL[precision], f"{name} {precision}")


@pytest.mark.parametrize("name,precision", HANDOVER)
def test_save_load_and_plain_iterations_after_fused_learned(name, precision):
    f, q = fused_and_sequential(name, precision)
    w = dirichlet_weights(f, np.random.default_rng(14))
    f.learned_iterations(w, 5, 0.5, improvement_slope=0.0)
    q.learned_iterations(w, 5, 0.5, improvement_slope=0.0)
    with tempfile.TemporaryDirectory() as d:
        p = os.path.join(d, "s.bin")
        f.save(p)
        t = bdd_hip_parallel_mma.load(p)
    assert_same(t, f, 0, "loaded")
    t.iterations(3)
    f.iterations(3)
    q.iterations(3)
    assert_same(t, f, 0, "loaded + 3")
    assert_same(t, q, ISO_TOL[precision], f"{name} {precision}")


@pytest.mark.parametrize("name,precision", HANDOVER)
def test_update_costs_between_fused_learned_calls(name, precision):
    f, q = fused_and_sequential(name, precision)
    rng = np.random.default_rng(15)
    w = dirichlet_weights(f, rng)
    d = rng.uniform(-0.5, 0.5, size=f.nr_variables())
    for s in (f, q):
        s.learned_iterations(w, 3, 0.5, improvement_slope=0.0)
        s.update_costs([], d)     # both sweep states are stale when the next launch starts
        s.learned_iterations(w, 3, 0.5, improvement_slope=0.0)
    assert_same(f, q, ISO_TOL[precision], f"{name} {precision}")


@pytest.mark.parametrize("name,precision", HANDOVER)
def test_distribute_delta_after_fused_learned(name, precision):
    f, q = fused_and_sequential(name, precision)
    w = dirichlet_weights(f, np.random.default_rng(16))
    for s in (f, q):
        s.learned_iterations(w, 3, 0.5, improvement_slope=0.0)
        s.distribute_delta()
    assert abs(f.lower_bound() - q.lower_bound()) <= ISO_TOL[precision] * max(1.0, abs(q.lower_bound()))
    assert_same(f, q, ISO_TOL[precision], f"{name} {precision}")


# ---------------------------------------------------------------- 4. history split
@pytest.mark.parametrize("name,precision", [("assign8", "float"), ("assign8", "double"), ("cover67x100", "float"), ("cover67x100", "double")])
def test_history_of_the_last_three_of_ten_iterations(name, precision):
    """7 iterations fused, then the 3 the history reaches through the four-launch loop"""
    f, q = fused_and_sequential(name, precision)
    w = dirichlet_weights(f, np.random.default_rng(17))
    L, B = f.nr_layers(), f.nr_bdds()
    outs = [[np.full(L, 7.0, f.value_type), np.full(B, 7.0, f.value_type), np.full(B, 7.0, f.value_type)] for _ in range(2)]
    for s, o in zip((f, q), outs):
        assert s.learned_iterations(w, 10, 0.5, improvement_slope=0.0, sol_avg=o[0], lb_first_diff_avg=o[1], lb_second_diff_avg=o[2],
                                    compute_history_for_itr=3, history_avg_beta=0.7) == 10
    rel = ISO_TOL[precision]
    assert_same(f, q, rel, f"{name} {precision}")
    for x, y, nm in zip(outs[0], outs[1], ("sol_avg", "lb_first_diff_avg", "lb_second_diff_avg")):
        y64 = np.asarray(y, np.float64)
        np.testing.assert_allclose(np.asarray(x, np.float64), y64, rtol=rel, atol=rel * max(1.0, float(np.abs(y64).max())), err_msg=nm)
    assert not np.all(outs[0][0] == 7.0) and not np.all(outs[0][2] == 7.0)   # three tracked iterations reach all three outputs


# ---------------------------------------------------------------- 5. the set-once initial bound change
def test_initial_lb_change_is_carried_from_a_fused_first_call():
    col, z = load_golden("matching_3x3_first_row")
    f = bdd_hip_parallel_mma(col, None, precision="double")
    q = bdd_hip_parallel_mma(col, None, precision="double", variant_flags=SEQ)
    assert f.fused_small() and f.fused_small_learned() and not q.fused_small_learned()
    ran = []
    for s in (f, q):
        s.update_costs([], pad_costs(z["costs"], s.nr_variables()))
        iso = s.get_isotropic_dist_weights()
        assert s.learned_iterations(iso, 4, 0.5, improvement_slope=0.0) == 4
        ran.append(s.learned_iterations(iso, 200, 0.5, improvement_slope=1e-3))
    assert ran[0] == ran[1] and 1 < ran[0] < 200, ran


# ---------------------------------------------------------------- 6. batches
def member_set(precision):
    """[(name, solver, twin)]: about 20 members, shapes interleaved so that no group is contiguous in the caller's order"""
    out = []
    for seed_pos in range(4):
        for name, packs, fused_in, seeds in SHAPES:
            if precision in fused_in and seed_pos < len(seeds):
                col, costs = instance(name, seeds[seed_pos])
                s, t = (bdd_hip_parallel_mma(col, costs, precision=precision) for _ in range(2))
                assert s.nr_packs() == packs and s.fused_small() and s.fused_small_learned() and t.fused_small_learned(), name
                out.append((name, s, t))
    return out


def batch_inputs(ms, rng, with_omega_vec):
    w = [dirichlet_weights(s, rng) for _, s, _ in ms]
    ov = [rng.uniform(0.1, 0.9, s.nr_layers()).astype(s.value_type) for _, s, _ in ms] if with_omega_vec else None
    return w, ov


def twin_calls(ms, w, ov, n, omega=0.5):
    for i, (_, _, t) in enumerate(ms):
        if ov is None:
            assert t.learned_iterations(w[i], n, omega, improvement_slope=0.0) == n
        else:
            assert t.learned_iterations(w[i], n, improvement_slope=0.0, omega_vec=ov[i]) == n


@pytest.mark.parametrize("device_inputs", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("precision", ["float", "double"])
def test_batch_learned_iterations_equal_each_member_driven_alone(precision, device_inputs):
    import torch
    ms = member_set(precision)
    assert len(ms) == (20 if precision == "float" else 17)
    batch = bdd_hip_batch([s for _, s, _ in ms])
    rng = np.random.default_rng(21)
    put = (lambda xs: torch.tensor(np.concatenate(xs), device="cuda")) if device_inputs else np.concatenate
    for with_ov in (False, True):
        w, ov = batch_inputs(ms, rng, with_ov)
        for n in (1, 2, 17):
            omega = 0.5 if n != 2 else 0.3
            batch.learned_iterations(put(w), n, omega=omega, omega_vec=put(ov) if with_ov else None)
            twin_calls(ms, w, ov, n, omega)
            for name, s, t in ms:
                assert_same(s, t, 0, f"{name} {precision}: {n} iterations, omega_vec {with_ov}")
    # nothing at all
    before = [state(s) for _, s, _ in ms]
    batch.learned_iterations(put(w), 0)
    for (_, s, _), b in zip(ms, before):
        for x, y in zip(state(s), b):
            np.testing.assert_array_equal(x, y)
    # each member's set-once initial bound change was set by the batch's first call as by the twin's: the stopping rule fires alike
    for name, s, t in ms[:4]:
        iso = s.get_isotropic_dist_weights()
        assert s.learned_iterations(iso, 60, 0.5, improvement_slope=1e-2) == t.learned_iterations(iso, 60, 0.5, improvement_slope=1e-2), name
    batch.close()


@pytest.mark.parametrize("precision", ["float", "double"])
def test_batch_learned_of_one_member(precision):
    col, costs = instance("assign8", 1)
    s, t = (bdd_hip_parallel_mma(col, costs, precision=precision) for _ in range(2))
    batch = bdd_hip_batch([s])
    w = dirichlet_weights(s, np.random.default_rng(22))
    for n in (1, 5):
        batch.learned_iterations(w, n)
        t.learned_iterations(w, n, 0.5, improvement_slope=0.0)
        assert_same(s, t, 0)
    batch.close()


@pytest.mark.parametrize("precision", ["float", "double"])
def test_batch_learned_interleaved_with_other_calls(precision):
    """ordered after what is queued on every member's stream (update_costs, a member's own iteration, the batch's plain iterations) and in
    front of what a member does next; a member whose costs-to-terminal are stale gets its backward run first"""
    ms = member_set(precision)
    batch = bdd_hip_batch([s for _, s, _ in ms])
    rng = np.random.default_rng(23)
    w, _ = batch_inputs(ms, rng, False)
    batch.iterations(2)
    for i, (_, s, t) in enumerate(ms):
        t.iterations(2)
        if i % 3 == 0:
            d = rng.uniform(-0.5, 0.5, size=s.nr_variables())
            s.update_costs([], d)
            t.update_costs([], d)
        elif i % 3 == 1:
            s.iteration()
            t.iteration()
    batch.learned_iterations(np.concatenate(w), 4)
    twin_calls(ms, w, None, 4)
    for i, (_, s, t) in enumerate(ms):
        if i % 2 == 0:      # right behind it, without the host having waited
            s.iteration()
            t.iteration()
    for name, s, t in ms:
        assert_same(s, t, 0, name)
    batch.iterations(3)
    batch.learned_iterations(np.concatenate(w), 2, omega=0.4)
    for name, s, t in ms:
        t.iterations(3)
    twin_calls(ms, w, None, 2, 0.4)
    for name, s, t in ms:
        assert_same(s, t, 0, name)
    batch.close()


# ---------------------------------------------------------------- 7. batch refusals
def refused(rc, make):
    with pytest.raises(capi.BddMmaError, match=f"error {rc}:") as e:
        make()
    return str(e.value)


@pytest.mark.parametrize("device_inputs", [False, True], ids=["host", "device"])
def test_batch_refusals_leave_every_member_unchanged(device_inputs):
    """(A member that is fused_small but not learned-fusable: test_a_member_that_is_not_learned_fusable_is_refused.)"""
    import torch
    members = [bdd_hip_parallel_mma(*instance(n, 1), precision="float") for n in ("assign8", "cover40x60", "cover67x100", "assign3")]
    batch = bdd_hip_batch(members)
    rng = np.random.default_rng(24)
    w = [dirichlet_weights(s, rng) for s in members]
    ov = [np.full(s.nr_layers(), 0.5, s.value_type) for s in members]
    put = (lambda xs: torch.tensor(np.concatenate(xs), device="cuda")) if device_inputs else np.concatenate
    batch.learned_iterations(put(w), 2)
    before = [state(s) for s in members]

    def unchanged():
        for s, b in zip(members, before):
            for x, y in zip(state(s), b):
                np.testing.assert_array_equal(x, y)

    bad_w = [x.copy() for x in w]
    bad_w[2][5] = np.nan
    msg = refused(capi.ERR_INVALID_ARGUMENT, lambda: batch.learned_iterations(put(bad_w), 3))
    assert "member 2" in msg and "dist_weights" in msg
    unchanged()
    bad_ov = [x.copy() for x in ov]
    bad_ov[1][0] = -0.25
    msg = refused(capi.ERR_INVALID_ARGUMENT, lambda: batch.learned_iterations(put(w), 3, omega_vec=put(bad_ov)))
    assert "member 1" in msg and "omega_vec" in msg
    unchanged()
    wrapper = bdd_hip_lbfgs(members[3])
    msg = refused(capi.ERR_STATE, lambda: batch.learned_iterations(put(w), 3))
    assert "member 3" in msg and "L-BFGS" in msg
    unchanged()
    wrapper.close()
    batch.close()
    # the members go on as if nothing had been asked
    twin = bdd_hip_parallel_mma(*instance("assign8", 1), precision="float")
    twin.learned_iterations(w[0], 2, 0.5, improvement_slope=0.0)
    assert_same(members[0], twin, 0)


def test_a_member_that_is_not_learned_fusable_is_refused():
    """cover160x240 (8 packs, 8 variables per row) in double: the plain layout fits the CU's LDS (158 KiB with the 512-byte slack) and the
    learned one, an omega per layer more, does not.  bddmma_batch_create takes it; only the learned call refuses it, and on its own it runs
    learned iterations through the four launches."""
    a = bdd_hip_parallel_mma(*instance("assign8", 1), precision="double")
    b = bdd_hip_parallel_mma(*instance("cover160x240", 0), precision="double")
    q = bdd_hip_parallel_mma(*instance("cover160x240", 0), precision="double", variant_flags=SEQ)
    assert b.nr_packs() == 8 and b.fused_small() and not b.fused_small_learned() and a.fused_small_learned()
    batch = bdd_hip_batch([a, b])
    batch.iterations(2)
    q.iterations(2)
    before = [state(s) for s in (a, b)]
    w = np.concatenate([dirichlet_weights(s, np.random.default_rng(26)) for s in (a, b)])
    msg = refused(capi.ERR_UNSUPPORTED, lambda: batch.learned_iterations(w, 3))
    assert "member 1" in msg and "fused_small_learned" in msg
    for s, bf in zip((a, b), before):
        for x, y in zip(state(s), bf):
            np.testing.assert_array_equal(x, y)
    batch.close()
    wb = w[a.nr_layers():]
    assert b.learned_iterations(wb, 3, 0.5, improvement_slope=0.0) == q.learned_iterations(wb, 3, 0.5, improvement_slope=0.0) == 3
    assert_same(b, q, ISO_TOL["double"])


# ---------------------------------------------------------------- 8. autograd
AUTOGRAD_MEMBERS = ("assign8", "cover40x60", "assign3", "cover67x100")


def _autograd_case(precision, per_layer_omega, slope, history):
    import torch
    from bdd_amd.autograd import DualIterations
    tdt = torch.float64 if precision == "double" else torch.float32
    a = [bdd_hip_parallel_mma(*instance(n, 1), precision=precision) for n in AUTOGRAD_MEMBERS]
    b = [bdd_hip_parallel_mma(*instance(n, 1), precision=precision) for n in AUTOGRAD_MEMBERS]
    assert all(s.fused_small_learned() for s in a + b)
    batch = bdd_hip_batch(a)
    rng = np.random.default_rng(25)
    costs = [s.get_solver_costs() for s in a]
    lo, hi = (np.concatenate([c[k] for c in costs]) for k in range(2))
    mm = rng.uniform(-0.25, 0.25, lo.size).astype(a[0].value_type)
    w = np.concatenate([dirichlet_weights(s, rng) for s in a])
    om = rng.uniform(0.1, 0.9, lo.size).astype(a[0].value_type) if per_layer_omega else np.asarray([0.5], a[0].value_type)
    g = [rng.normal(0, 1, lo.size).astype(a[0].value_type) for _ in range(3)]
    results = []
    for solvers in (batch, list(b)):
        t = [torch.tensor(x, dtype=tdt, device="cuda", requires_grad=True) for x in (lo, hi, mm, w, om)]
        out = DualIterations.apply(solvers, *t[:4], 5, t[4], 3, slope, 1, history, 0.9)
        torch.autograd.backward(out[:3], [torch.tensor(x, dtype=tdt, device="cuda") for x in g])
        torch.cuda.synchronize()
        results.append(([o.detach().cpu().numpy() for o in out if o is not None], [x.grad.cpu().numpy() for x in t]))
    batch.close()
    offsets = np.cumsum([0] + [s.nr_layers() for s in a])
    return results, offsets


def _assert_tiered(got, want, off, precision):
    """per-layer batch tensors: bit-equal in float and on the assign* members in double; the cover* members in double, and the one scalar
    omega's gradient (a sum over all members), at tier 1 — there the exchange (forward) and the gradient sweeps' atomics (backward) add a
    variable's terms in an order that is not fixed"""
    n_layers = off[-1]
    exact = np.ones(n_layers, bool)
    if precision == "double":
        for i, n in enumerate(AUTOGRAD_MEMBERS):
            if n.startswith("cover"):
                exact[off[i]:off[i + 1]] = False
    rel = ISO_TOL[precision]
    for x, y in zip(got, want):
        if x.size == n_layers:
            np.testing.assert_array_equal(x[exact], y[exact])
        elif precision == "float":
            np.testing.assert_array_equal(x, y)
        np.testing.assert_allclose(x, y, rtol=rel, atol=rel * max(1.0, float(np.abs(y).max())))


@pytest.mark.parametrize("per_layer_omega", [False, True], ids=["omega", "omega_vec"])
@pytest.mark.parametrize("precision", ["float", "double"])
def test_dual_iterations_of_a_batch_equal_those_of_the_list(precision, per_layer_omega):
    ((out_b, grad_b), (out_l, grad_l)), off = _autograd_case(precision, per_layer_omega, 0.0, 0)
    _assert_tiered(out_b, out_l, off, precision)
    _assert_tiered(grad_b, grad_l, off, precision)


@pytest.mark.parametrize("slope,history", [(0.02, 0), (0.0, 2)], ids=["slope", "history"])
@pytest.mark.parametrize("precision", ["float", "double"])
def test_dual_iterations_of_a_batch_fall_back_to_the_list_form(precision, slope, history):
    """With a stopping rule or a history the batch form makes the list form's calls.  Bit for bit wherever the list form itself is
    reproducible between two handles: in float, and on the assign* members in double.  On the cover* members in double it is not — these
    calls run the four-launch exchange, whose LDS atomics add a variable's (more than two) terms in no fixed order: measured on the MI355X
    with improvement_slope = 0.02, two handles given the same list-form call differ in 192 of the 1146 arc costs by at most 3.5e-16
    (relative 3.7e-14) — so there the comparison is tier 1, as in the test above."""
    ((out_b, grad_b), (out_l, grad_l)), off = _autograd_case(precision, False, slope, history)
    assert len(out_b) == len(out_l) == (6 if history else 3)
    _assert_tiered(out_b, out_l, off, precision)
    _assert_tiered(grad_b, grad_l, off, precision)
