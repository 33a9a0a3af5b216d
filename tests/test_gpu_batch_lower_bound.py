"""A batch's lower bounds in one launch (include/bdd_mma.h: bddmma_lower_bound_batch; kernels/batchlb.hpp: k_small_bound_batch) on the
MI355X: one workgroup per member sweeps where the member's costs-to-terminal are stale and reduces the member's partial sums.

The reference of every comparison is a twin of each member driven alone through lower_bound() (its BWD_PLAIN launch and k_lb_reduce).
Every comparison is bit for bit, in float and in double: the kernel takes one minimum per arc in the sweep's operand order and adds the
partial sums in the reduce kernel's order.  The members are test_gpu_batch_small.py's: every wave-count group (1, 2, 4, 8 and, in float,
16 waves), no group contiguous in the caller's order."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from bdd_amd import capi  # noqa: E402
from bdd_amd.solver import bdd_hip_batch, bdd_hip_lbfgs, run_solver  # noqa: E402
from test_gpu_batch_costs import fused, names_of  # noqa: E402
from test_gpu_batch_costs import member_set as named_set  # noqa: E402
from test_gpu_batch_round import LOOP, twin_loop  # noqa: E402
from test_gpu_batch_small import assert_unchanged, member_set, run_members, snapshot  # noqa: E402

SENTINEL = -12345.5


def bounds_abi(batch, on_device=0, out=None):
    """bddmma_lower_bound_batch with a host array: (rc, the array)"""
    if out is None:
        out = np.full(len(batch), SENTINEL, dtype=np.float64)
    rc = batch._L.bddmma_lower_bound_batch(batch._h, out.ctypes.data_as(C.POINTER(C.c_double)), on_device)
    return rc, out


def host_bounds(batch):
    rc, out = bounds_abi(batch)
    assert rc == capi.OK, batch._L.bddmma_batch_last_error(batch._h)
    return out


def assert_same_sweep(ms, what):
    """the costs-to-terminal the kernel left are the member's own sweep's: what reads them, and iterations that start from them"""
    for name, _, s, t in ms:
        np.testing.assert_array_equal(s.lower_bound_per_bdd(), t.lower_bound_per_bdd(), err_msg=f"{what}, {name}: per BDD")
        np.testing.assert_array_equal(s.min_marginal_diff(), t.min_marginal_diff(), err_msg=f"{what}, {name}: min-marginal differences")
    for name, _, s, t in ms:
        s.iterations(5)
        t.iterations(5)
        assert s.lower_bound() == t.lower_bound(), (what, name)


def sets(precision):
    ms = member_set(precision)
    assert {p for _, p, _, _ in ms} == ({1, 2, 4, 7, 10} if precision == "float" else {1, 2, 4, 7})
    return ms, bdd_hip_batch([s for _, _, s, _ in ms])


# ---------------------------------------------------------------- 1. every member swept
@pytest.mark.parametrize("precision", ["float", "double"])
def test_fresh_members_are_swept_in_the_launch(precision):
    ms, batch = sets(precision)
    got = host_bounds(batch)
    want = np.array([t.lower_bound() for _, _, _, t in ms])
    print(precision, "fresh", got)
    np.testing.assert_array_equal(got, want)
    for i, (name, _, s, _) in enumerate(ms):   # the cached bound is the call's
        assert s.lower_bound() == got[i], name
    np.testing.assert_array_equal(batch.lower_bounds(), want)   # the first batch call's name: the same values
    assert_same_sweep(ms, f"{precision}, fresh")
    batch.close()


# ---------------------------------------------------------------- 2. every member reduce only
@pytest.mark.parametrize("precision", ["float", "double"])
def test_members_behind_batch_iterations_are_reduced_only(precision):
    ms, batch = sets(precision)
    batch.iterations(3, omega=0.5)
    for _, _, _, t in ms:
        t.iterations(3, omega=0.5)
    got = host_bounds(batch)
    want = np.array([t.lower_bound() for _, _, _, t in ms])
    print(precision, "behind 3 iterations", got)
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(host_bounds(batch), want)   # every bound cached: the reduction's results equal the caches
    assert_same_sweep(ms, f"{precision}, behind iterations")
    batch.close()


# ---------------------------------------------------------------- 3. mixed flags in one call
@pytest.mark.parametrize("precision", ["float", "double"])
def test_stale_members_beside_cached_ones_in_one_call(precision):
    ms, batch = sets(precision)
    batch.iterations(2)
    for _, _, _, t in ms:
        t.iterations(2)
    first = host_bounds(batch)   # caches every member's bound
    rng = np.random.default_rng(22)
    changed, seen = [], {}
    for i, (name, _, s, t) in enumerate(ms):
        # a third of the members, of every shape: the k-th member of the j-th shape where (k + j) % 3 == 0
        j = seen.setdefault(name, [len(seen), 0])
        j[1] += 1
        if (j[0] + j[1] - 1) % 3:
            continue
        changed.append(i)
        if len(changed) % 2:   # the arc costs replaced
            lo, hi, mm = (rng.uniform(-1.0, 3.0, s.nr_layers()).astype(s.value_type) for _ in range(3))
            s.set_solver_costs(lo, hi, mm * 0.1)
            t.set_solver_costs(lo, hi, mm * 0.1)
        else:       # ... or shifted: both sweep states stale
            d = rng.uniform(-0.5, 0.5, s.nr_variables())
            s.update_costs([], d)
            t.update_costs([], d)
    assert {ms[i][1] for i in changed} == {p for _, p, _, _ in ms} and 3 * len(changed) <= len(ms) + 3, [ms[i][0] for i in changed]
    got = host_bounds(batch)
    want = np.array([t.lower_bound() for _, _, _, t in ms])
    print(precision, "mixed", got)
    np.testing.assert_array_equal(got, want)
    for i in range(len(ms)):
        assert (got[i] != first[i]) == (i in changed), (ms[i][0], got[i], first[i])
    assert_same_sweep(ms, f"{precision}, mixed")
    batch.close()


# ---------------------------------------------------------------- 4. device output
@pytest.mark.parametrize("precision", ["float", "double"])
def test_device_output_and_ordering_with_member_calls(precision):
    import torch
    ms, batch = sets(precision)
    n = len(ms)
    rng = np.random.default_rng(23)
    # fresh members (swept), into a device array
    out = torch.full((n,), SENTINEL, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    assert batch.lower_bounds(out=out) is out
    batch.stream_signal(torch.cuda.current_stream().cuda_stream)
    want = np.array([t.lower_bound() for _, _, _, t in ms])
    np.testing.assert_array_equal(out.cpu().numpy(), want)
    for (name, _, s, _), w in zip(ms, want):   # no bound was cached by the call: the member reduces what the kernel's sweep left
        assert s.lower_bound() == w, name
    # a member call queued right before the batch call, on the member's stream
    for _, _, s, t in ms:
        d = rng.uniform(-0.5, 0.5, s.nr_variables())
        s.update_costs([], d)
        t.update_costs([], d)
    out.fill_(SENTINEL)
    torch.cuda.synchronize()
    batch.lower_bounds(out=out)
    batch.stream_signal(torch.cuda.current_stream().cuda_stream)
    want2 = np.array([t.lower_bound() for _, _, _, t in ms])
    got2 = out.cpu().numpy()
    print(precision, "device", got2)
    np.testing.assert_array_equal(got2, want2)
    assert np.all(want2 != want)
    # two device calls back to back (the second reduces only), then the host form
    out_b = torch.full((n,), SENTINEL, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    batch.iterations(1)
    batch.lower_bounds(out=out)
    batch.lower_bounds(out=out_b)
    batch.stream_signal(torch.cuda.current_stream().cuda_stream)
    for _, _, _, t in ms:
        t.iterations(1)
    want3 = np.array([t.lower_bound() for _, _, _, t in ms])
    np.testing.assert_array_equal(out.cpu().numpy(), want3)
    np.testing.assert_array_equal(out_b.cpu().numpy(), want3)
    np.testing.assert_array_equal(host_bounds(batch), want3)
    assert_same_sweep(ms, f"{precision}, device")
    with pytest.raises(capi.BddMmaError, match=f"error {capi.ERR_INVALID_ARGUMENT}:"):
        batch.lower_bounds(out=np.zeros(n))
    torch.cuda.synchronize()
    batch.close()


# ---------------------------------------------------------------- 5. the callers inside the batch: run_solver and the rounding loop
@pytest.mark.parametrize("precision", ["float", "double"])
def test_run_solver_of_a_batch_still_equals_each_member_run_alone(precision):
    ms = run_members(precision)
    batch = bdd_hip_batch([s for s, _ in ms])
    res = batch.run_solver(max_iter=1000, tolerance=1e-4, improvement_slope=0.0, time_limit=1e9)
    for r, (s, t) in zip(res, ms):
        q = run_solver(t, max_iter=1000, tolerance=1e-4, improvement_slope=0.0, time_limit=1e9)
        assert (r["iterations"], r["stop_reason"], r["lb_initial"], r["lb_final"]) == (q["iterations"], q["stop_reason"], q["lb_initial"], q["lb_final"])
        assert s.lower_bound() == r["lb_final"] == t.lower_bound()
    np.testing.assert_array_equal(host_bounds(batch), [r["lb_final"] for r in res])
    batch.close()


@pytest.mark.parametrize("precision", ["float", "double"])
def test_the_rounding_loop_of_a_batch_still_equals_each_members_own(precision):
    """40 rounds: members leave the loop at different rounds, so later rounds' bounds run with a mask — a masked member's workgroup
    returns at once and its cached bound stays"""
    names = names_of(precision)
    members, twins = named_set(names, precision), named_set(names, precision)
    batch = bdd_hip_batch(members)
    got, rounds = batch.primal_rounding_incremental(num_rounds=40, seed=9, return_rounds=True, **LOOP)
    want = [twin_loop(q, 40, 9) for q in twins]
    print(precision, rounds, [bool(w) for w in want])
    assert len(set(rounds)) >= 2, rounds
    for n, g, w, s, q in zip(names, got, want, members, twins):
        assert g == w, (precision, n)
        for x, y in zip(s.get_solver_costs(), q.get_solver_costs()):
            np.testing.assert_array_equal(x, y, err_msg=n)
        assert s.lower_bound() == q.lower_bound(), n
    np.testing.assert_array_equal(host_bounds(batch), [q.lower_bound() for q in twins])
    batch.close()


# ---------------------------------------------------------------- 6. refusals
def test_refusals_leave_every_member_and_the_output_untouched():
    import torch
    a, b = fused("assign8", "float"), fused("cover40x60", "float")
    batch = bdd_hip_batch([a, b])
    batch.iterations(2)
    before = host_bounds(batch)
    L = batch._L
    assert L.bddmma_lower_bound_batch(None, None, 0) == capi.ERR_INVALID_ARGUMENT
    assert L.bddmma_lower_bound_batch(batch._h, None, 0) == capi.ERR_INVALID_ARGUMENT
    assert L.bddmma_lower_bound_batch(batch._h, None, 1) == capi.ERR_INVALID_ARGUMENT
    assert b"null" in L.bddmma_batch_last_error(batch._h)
    d = np.random.default_rng(24).uniform(-0.5, 0.5, b.nr_variables())
    b.update_costs([], d)   # stale: the call would sweep it
    wrapper = bdd_hip_lbfgs(b)
    snap = snapshot([a, b])
    rc, out = bounds_abi(batch)
    assert rc == capi.ERR_STATE and np.all(out == SENTINEL)
    msg = L.bddmma_batch_last_error(batch._h)
    assert b"member 1" in msg and b"L-BFGS" in msg
    dev = torch.full((2,), SENTINEL, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    with pytest.raises(capi.BddMmaError, match=f"error {capi.ERR_STATE}:"):
        batch.lower_bounds(out=dev)
    torch.cuda.synchronize()
    assert torch.all(dev == SENTINEL)
    a.set_profiling(True)
    rc, out = bounds_abi(batch)
    assert rc == capi.ERR_STATE and np.all(out == SENTINEL)
    assert b"member 0" in L.bddmma_batch_last_error(batch._h)
    a.set_profiling(False)
    assert_unchanged([a, b], snap)
    assert a.lower_bound() == before[0]
    batch.close()
    wrapper.close()
