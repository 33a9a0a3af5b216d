"""The min-marginal differences of a batch and their gradient, one launch each (bddmma_min_marginal_diff_batch,
bddmma_grad_min_marginal_diff_batch: kernels/batchmm.hpp; ComputeAllMinMarginalsDiff on a batch) on the MI355X.

The reference of every comparison is a twin of each member driven alone through the per-member calls.  Every comparison is bit for bit:
minima are exact in any order, and the gradient's sums run in the order of the bodies the batch kernel shares with the per-member
kernels (kernels/gradmm.hpp), ties included, which leaves no room for a tolerance.  The member sets are those of
tests/test_gpu_batch_costs.py::names_of: one pack (assign3, mostly padding lanes; assign9 with more than 64 layers on one wave), set
covers of 2, 4, 7 and 10 packs (10 packs: 16 waves of which 6 are idle, float only) and mixed3x9, whose waves sweep packs of 3 and of 9
hops.  Every test asserts nr_packs() and fused_small() first (fused())."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from bdd_amd import capi  # noqa: E402
from bdd_amd.solver import bdd_hip_batch, bdd_hip_lbfgs, bdd_hip_parallel_mma  # noqa: E402
from test_gpu_batch_bounds import read, sentinel, set_both  # noqa: E402
from test_gpu_batch_costs import VIEWS, dev, fused, member_set, names_of, offsets, random_costs, refused, set_alone, part, state, views  # noqa: E402
from test_gpu_small_learned import AUTOGRAD_MEMBERS  # noqa: E402


def batch_diff(batch, members, device_arrays):
    if not device_arrays:
        return batch.min_marginal_diff()
    out = sentinel(offsets(members)[-1], members)
    assert batch.min_marginal_diff(out=out) is out
    return read(batch, out)[0]


def batch_grad(batch, members, g, device_arrays):
    if not device_arrays:
        return batch.grad_all_min_marginal_differences(g)
    import torch
    n = offsets(members)[-1]
    out = (sentinel(n, members), sentinel(n, members))
    gd = dev(g)
    torch.cuda.synchronize()
    batch.stream_wait(torch.cuda.current_stream().cuda_stream)
    batch.grad_all_min_marginal_differences(gd, out=out)
    return read(batch, *out)


def twin_grad(twins, g):
    off = offsets(twins)
    res = [q.grad_all_min_marginal_differences(g[off[i]:off[i + 1]]) for i, q in enumerate(twins)]
    return np.concatenate([r[0] for r in res]), np.concatenate([r[1] for r in res])


def assert_views(names, members, twins, what):
    for n, s, q in zip(names, members, twins):
        for x, y, nm in zip(views(s), views(q), VIEWS):
            np.testing.assert_array_equal(x, y, err_msg=f"{what}, {n}: {nm}")


# ---------------------------------------------------------------- 1. differences
@pytest.mark.parametrize("device_arrays", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("precision", ["float", "double"])
def test_batch_differences_equal_each_members_own(precision, device_arrays):
    names = names_of(precision)
    members, twins = member_set(names, precision), member_set(names, precision)
    batch = bdd_hip_batch(members)
    rng = np.random.default_rng(71)

    def check(what):
        got = batch_diff(batch, members, device_arrays)
        want = np.concatenate([q.min_marginal_diff() for q in twins])
        assert got.dtype == members[0].value_type and got.shape == want.shape
        np.testing.assert_array_equal(got, want, err_msg=f"{precision}, {what}")
        assert np.any(got != 0)

    set_both(batch, twins, random_costs(members, rng))
    check("behind a batch set")
    batch.iterations(3)
    for q in twins:
        q.iterations(3)
    check("behind 3 iterations")
    # stale sweep states on two members, valid ones on the others
    for i in (1, len(members) - 1):
        v = members[i].nr_variables()
        d0, d1 = rng.uniform(-0.5, 0.5, v), rng.uniform(-0.5, 0.5, v)
        members[i].update_costs(d0, d1)
        twins[i].update_costs(d0, d1)
    check("behind update_costs on two members")
    assert_views(names, members, twins, precision)
    batch.close()


# ---------------------------------------------------------------- 2. gradient
@pytest.mark.parametrize("device_arrays", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("precision", ["float", "double"])
def test_batch_difference_gradient_equals_each_members_own(precision, device_arrays):
    names = names_of(precision)
    members, twins = member_set(names, precision), member_set(names, precision)
    batch = bdd_hip_batch(members)
    dt = members[0].value_type
    n = int(offsets(members)[-1])
    off = offsets(members)
    rng = np.random.default_rng(72)
    integer = lambda k: rng.integers(-2, 3, k).astype(dt)
    nonzero = lambda k: rng.choice(np.asarray([-2.0, -1.0, 1.0, 2.0]), k).astype(dt)
    cases = [("random", random_costs(members, rng)[:2], rng.normal(0, 1, n).astype(dt)),
             ("integer", (integer(n), integer(n)), integer(n)),
             ("zero", (np.zeros(n, dt), np.zeros(n, dt)), nonzero(n)),
             ("zero, hi = 1 on every other layer", (np.zeros(n, dt), (np.arange(n) % 2).astype(dt)), nonzero(n))]
    for what, (lo, hi), g in cases:
        set_both(batch, twins, (lo, hi, np.zeros(n, dt)))
        want = twin_grad(twins, g)
        if what != "random":
            # exact ties all over: the twins' own output, decided by the tie rule of include/bdd_mma.h, is not identically zero on any member
            for i, nm in enumerate(names):
                assert np.any(want[0][off[i]:off[i + 1]] != 0) or np.any(want[1][off[i]:off[i + 1]] != 0), (what, nm)
        for rep in range(2):   # twice in a row
            got = batch_grad(batch, members, g, device_arrays)
            for k, nm in enumerate(("grad_lo", "grad_hi")):
                assert got[k].dtype == dt and got[k].shape == (n,)
                np.testing.assert_array_equal(got[k], want[k], err_msg=f"{precision}, {what}, call {rep}: {nm}")
        assert np.any(got[0] != 0) and np.any(got[1] != 0)
    batch.iterations(2)
    for q in twins:
        q.iterations(2)
    g = rng.normal(0, 1, n).astype(dt)
    got, want = batch_grad(batch, members, g, device_arrays), twin_grad(twins, g)
    for k, nm in enumerate(("grad_lo", "grad_hi")):
        np.testing.assert_array_equal(got[k], want[k], err_msg=f"{precision}, behind 2 iterations: {nm}")
    before = [state(s) for s in members]
    got = batch_grad(batch, members, g, device_arrays)   # arc costs, deferred differences and delta are unchanged by the call
    for nme, s, bf in zip(names, members, before):
        for x, y, nm in zip(state(s), bf, VIEWS):
            np.testing.assert_array_equal(x, y, err_msg=f"{precision}, {nme}: {nm} changed")
    assert_views(names, members, twins, precision)   # ... and every getter agrees with the twin's
    batch.close()


# ---------------------------------------------------------------- 3. ordering without host synchronisation
@pytest.mark.parametrize("precision", ["float", "double"])
def test_member_calls_and_batch_mmdiff_calls_order_themselves(precision):
    import torch
    names = names_of(precision)
    members, twins = member_set(names, precision), member_set(names, precision)
    batch = bdd_hip_batch(members)
    dt = members[0].value_type
    n = int(offsets(members)[-1])
    rng = np.random.default_rng(73)
    stream = torch.cuda.current_stream().cuda_stream

    def twins_do(f):
        for q in twins:
            f(q)
            q.synchronize()

    # ---- member iterations (which overwrite costs and both sweep states) right behind each batch call
    arrays = random_costs(members, rng)
    g = rng.normal(0, 1, n).astype(dt)
    d, gd = [dev(x) for x in arrays], dev(g)
    mm, g_lo, g_hi = sentinel(n, members), sentinel(n, members), sentinel(n, members)
    torch.cuda.synchronize()
    batch.stream_wait(stream)
    batch.set_solver_costs(*d)
    batch.min_marginal_diff(out=mm)
    for s in members:
        s.iterations(2)
    batch.grad_all_min_marginal_differences(gd, out=(g_lo, g_hi))
    for s in members:
        s.iterations(2)
    got = read(batch, mm, g_lo, g_hi)
    off = offsets(twins)
    for i, q in enumerate(twins):
        set_alone(q, *(part(x, off, i) for x in arrays))
        q.synchronize()
    want_mm = np.concatenate([q.min_marginal_diff() for q in twins])
    twins_do(lambda q: q.iterations(2))
    want_g = twin_grad(twins, g)
    twins_do(lambda q: q.iterations(2))
    np.testing.assert_array_equal(got[0], want_mm, err_msg=f"{precision}: differences in front of member iterations")
    np.testing.assert_array_equal(got[1], want_g[0], err_msg=f"{precision}: grad_lo between member iterations")
    np.testing.assert_array_equal(got[2], want_g[1], err_msg=f"{precision}: grad_hi between member iterations")
    assert_views(names, members, twins, f"{precision}, member iterations behind the batch calls")
    # ---- each batch call right behind 50 queued member iterations
    g = rng.normal(0, 1, n).astype(dt)
    gd = dev(g)
    torch.cuda.synchronize()
    batch.stream_wait(stream)
    for s in members:
        s.iterations(50)
    batch.min_marginal_diff(out=mm)
    for s in members:
        s.iterations(50)
    batch.grad_all_min_marginal_differences(gd, out=(g_lo, g_hi))
    got = read(batch, mm, g_lo, g_hi)
    twins_do(lambda q: q.iterations(50))
    want_mm = np.concatenate([q.min_marginal_diff() for q in twins])
    twins_do(lambda q: q.iterations(50))
    want_g = twin_grad(twins, g)
    np.testing.assert_array_equal(got[0], want_mm, err_msg=f"{precision}: differences behind 50 member iterations")
    np.testing.assert_array_equal(got[1], want_g[0], err_msg=f"{precision}: grad_lo behind 50 member iterations")
    np.testing.assert_array_equal(got[2], want_g[1], err_msg=f"{precision}: grad_hi behind 50 member iterations")
    assert np.any(got[0] != 0) and np.any(got[1] != 0) and np.any(got[2] != 0)
    assert_views(names, members, twins, f"{precision}, batch calls behind member iterations")
    batch.close()


# ---------------------------------------------------------------- 4. refusals
def test_refusals_are_decided_before_any_member_or_output_is_touched():
    import torch
    names = ("assign8", "cover40x60", "cover67x100", "assign3")
    members = member_set(names, "float")
    batch = bdd_hip_batch(members)
    L, h = batch._L, batch._h
    dt = members[0].value_type
    n = int(offsets(members)[-1])
    off = offsets(members)
    rng = np.random.default_rng(74)
    batch.set_solver_costs(*random_costs(members, rng))
    batch.iterations(2)
    before = [state(s) for s in members]

    def unchanged(what):
        for nme, s, bf in zip(names, members, before):
            for x, y, nm in zip(state(s), bf, VIEWS):
                np.testing.assert_array_equal(x, y, err_msg=f"{what}, {nme}: {nm}")

    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    g = rng.normal(0, 1, n).astype(dt)
    lo, hi, mm = np.full(n, -7.0, dt), np.full(n, -7.0, dt), np.full(n, -7.0, dt)
    # a null array
    for on_device in (0, 1):
        assert L.bddmma_min_marginal_diff_batch(h, None, on_device) == capi.ERR_INVALID_ARGUMENT
        assert b"null" in L.bddmma_batch_last_error(h)
        for args in ((None, ptr(lo), ptr(hi)), (ptr(g), None, ptr(hi)), (ptr(g), ptr(lo), None)):
            assert L.bddmma_grad_min_marginal_diff_batch(h, *args, on_device) == capi.ERR_INVALID_ARGUMENT
        assert b"null" in L.bddmma_batch_last_error(h)
    unchanged("null arrays")
    # a NaN inside the third member's part of grad_mm, and an infinity behind it in the fourth's
    bad = g.copy()
    bad[off[2] + 1] = np.nan
    bad[off[3]] = np.inf
    msg = refused(capi.ERR_INVALID_ARGUMENT, lambda: batch._check(L.bddmma_grad_min_marginal_diff_batch(h, ptr(bad), ptr(lo), ptr(hi), 0), h))
    assert "member 2" in msg and "grad_mm" in msg, msg
    d_lo, d_hi = sentinel(n, members), sentinel(n, members)
    d_bad = dev(bad)
    torch.cuda.synchronize()
    msg = refused(capi.ERR_INVALID_ARGUMENT, lambda: batch.grad_all_min_marginal_differences(d_bad, out=(d_lo, d_hi)))
    assert "member 2" in msg and "grad_mm" in msg, msg
    torch.cuda.synchronize()
    assert np.all(lo == -7.0) and np.all(hi == -7.0) and bool((d_lo == -7.0).all()) and bool((d_hi == -7.0).all())
    unchanged("a NaN in grad_mm")
    got = batch.grad_all_min_marginal_differences(g)   # and accepted again
    assert np.all(np.isfinite(got[0])) and np.any(got[1] != 0)
    # a member with an L-BFGS wrapper attached
    before = [state(s) for s in members]
    wrapper = bdd_hip_lbfgs(members[2])
    calls = (lambda: batch._check(L.bddmma_min_marginal_diff_batch(h, ptr(mm), 0), h),
             lambda: batch.min_marginal_diff(out=d_lo),
             lambda: batch._check(L.bddmma_grad_min_marginal_diff_batch(h, ptr(g), ptr(lo), ptr(hi), 0), h),
             lambda: batch.grad_all_min_marginal_differences(dev(g), out=(d_lo, d_hi)))
    for call in calls:
        msg = refused(capi.ERR_STATE, call)
        assert "member 2" in msg and "L-BFGS" in msg, msg
    torch.cuda.synchronize()
    assert np.all(mm == -7.0) and np.all(lo == -7.0) and np.all(hi == -7.0) and bool((d_lo == -7.0).all()) and bool((d_hi == -7.0).all())
    unchanged("an L-BFGS wrapper")
    wrapper.close()
    batch.close()


# ---------------------------------------------------------------- 5. autograd
COUNTED = [(cls, name) for cls in (bdd_hip_batch, bdd_hip_parallel_mma)
           for name in ("set_solver_costs", "get_solver_costs", "min_marginal_diff", "grad_all_min_marginal_differences")]
COUNTED += [(bdd_hip_parallel_mma, "stream_wait"), (bdd_hip_parallel_mma, "stream_signal")]


def counters(monkeypatch):
    calls = {}
    for cls, name in COUNTED:
        f, key = getattr(cls, name), f"{'batch' if cls is bdd_hip_batch else 'member'}.{name}"
        calls[key] = 0

        def wrapper(*a, _f=f, _key=key, **kw):
            calls[_key] += 1
            return _f(*a, **kw)
        monkeypatch.setattr(cls, name, wrapper)
    return calls


def mm_inputs(a, rng):
    dt = a[0].value_type
    n = int(offsets(a)[-1])
    return rng.uniform(-1.0, 3.0, n).astype(dt), rng.uniform(-1.0, 3.0, n).astype(dt), rng.normal(0, 1, n).astype(dt)


def run_mm(solvers, lo, hi, g, tdt):
    """ComputeAllMinMarginalsDiff forward and backward: the output and the two gradients as NumPy arrays"""
    import torch
    from bdd_amd.autograd import ComputeAllMinMarginalsDiff
    u = [torch.tensor(v, dtype=tdt, device="cuda", requires_grad=True) for v in (lo, hi)]
    mm = ComputeAllMinMarginalsDiff.apply(solvers, *u)
    mm.backward(torch.tensor(g, dtype=tdt, device="cuda"))
    torch.cuda.synchronize()
    return [mm.detach().cpu().numpy()] + [v.grad.cpu().numpy() for v in u]


@pytest.mark.parametrize("precision", ["float", "double"])
def test_the_function_of_a_batch_makes_batch_calls_only(precision, monkeypatch):
    """On a batch the forward makes one batch set and one batch min_marginal_diff, forward and backward two batch sets and one batch call
    each; neither makes a call on a member.  Outputs and gradients are the list form's bit for bit."""
    import torch
    from bdd_amd.autograd import ComputeAllMinMarginalsDiff
    tdt = torch.float64 if precision == "double" else torch.float32
    a, b = [fused(n, precision) for n in AUTOGRAD_MEMBERS], [fused(n, precision) for n in AUTOGRAD_MEMBERS]
    batch = bdd_hip_batch(a)
    rng = np.random.default_rng(75)
    lo, hi, g = mm_inputs(a, rng)
    calls = counters(monkeypatch)
    zero = {k: 0 for k in calls}
    t = [torch.tensor(v, dtype=tdt, device="cuda") for v in (lo, hi)]
    ComputeAllMinMarginalsDiff.apply(batch, *t)
    assert calls == {**zero, "batch.set_solver_costs": 1, "batch.min_marginal_diff": 1}, calls
    calls.update(zero)
    got = run_mm(batch, lo, hi, g, tdt)
    assert calls == {**zero, "batch.set_solver_costs": 2, "batch.min_marginal_diff": 1, "batch.grad_all_min_marginal_differences": 1}, calls
    calls.update(zero)
    want = run_mm(list(b), lo, hi, g, tdt)
    n = len(a)
    assert all(v == 0 for k, v in calls.items() if k.startswith("batch.")), calls
    assert calls["member.set_solver_costs"] == 2 * n and calls["member.min_marginal_diff"] == n and calls["member.grad_all_min_marginal_differences"] == n, calls
    for x, y in zip(got, want):
        np.testing.assert_array_equal(x, y)
        assert np.any(x != 0)
    batch.close()


@pytest.mark.parametrize("precision", ["float", "double"])
def test_the_function_of_a_batch_keeps_the_list_form_where_it_is_needed(precision, monkeypatch):
    """A member that has had an L-BFGS wrapper: the batch's first call refuses with BDDMMA_ERR_STATE, touching nothing, and the Function runs
    the list form.  The results are the list's."""
    import torch
    tdt = torch.float64 if precision == "double" else torch.float32
    a, b = [fused(n, precision) for n in AUTOGRAD_MEMBERS], [fused(n, precision) for n in AUTOGRAD_MEMBERS]
    batch = bdd_hip_batch(a)
    rng = np.random.default_rng(76)
    lo, hi, g = mm_inputs(a, rng)
    for s in (a[1], b[1]):
        wrapper = bdd_hip_lbfgs(s)
        wrapper.iteration()
        wrapper.close()
    calls = counters(monkeypatch)
    got = run_mm(batch, lo, hi, g, tdt)
    n = len(a)
    assert calls["member.min_marginal_diff"] == n and calls["member.grad_all_min_marginal_differences"] == n, calls
    assert calls["batch.min_marginal_diff"] == 0 and calls["batch.grad_all_min_marginal_differences"] == 0, calls
    want = run_mm(list(b), lo, hi, g, tdt)
    for x, y in zip(got, want):
        np.testing.assert_array_equal(x, y)
        assert np.any(x != 0)
    batch.close()
