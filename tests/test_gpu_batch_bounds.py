"""The tail of a training step's loss for a batch, one launch each (bddmma_lower_bound_per_bdd_batch,
bddmma_grad_lower_bound_per_bdd_batch, bddmma_distribute_delta_batch: kernels/batchbound.hpp; DistributeDeferredDelta and
ComputeLowerBoundperBDD on a batch) on the MI355X.

The reference of every comparison is a twin of each member driven alone through the per-member calls.  Every comparison is bit for bit:
the kernels copy, add in the per-member kernels' order and multiply once, which leaves no room for a tolerance (the one exception is the
whole chain behind DualIterations, which carries that Function's tiers: tests/test_gpu_small_learned.py::_assert_tiered).  The member
sets are those of tests/test_gpu_batch_costs.py::names_of: one pack (assign3, mostly padding lanes; assign9 with more than 64 layers on
one wave), set covers of 2, 4, 7 and 10 packs (10 packs: 16 waves of which 6 are idle, float only) and mixed3x9, whose waves sweep packs
of 3 and of 9 hops.  Every test asserts nr_packs() and fused_small() first (fused())."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from bdd_amd import capi  # noqa: E402
from bdd_amd.solver import bdd_hip_batch, bdd_hip_lbfgs, bdd_hip_parallel_mma  # noqa: E402
from test_gpu_batch_costs import VIEWS, dev, fused, member_set, names_of, offsets, part, random_costs, refused, set_alone, state, views  # noqa: E402
from test_gpu_small_learned import AUTOGRAD_MEMBERS, _assert_tiered, dirichlet_weights  # noqa: E402


def bdd_offsets(members):
    return np.cumsum([0] + [s.nr_bdds() for s in members])


def tdt_of(members):
    import torch
    return torch.float64 if members[0].value_type == np.float64 else torch.float32


def sentinel(n, members):
    import torch
    return torch.full((int(n),), -7.0, dtype=tdt_of(members), device="cuda")


def read(batch, *tensors):
    """device outputs of a batch call, read on torch's stream behind the batch's"""
    import torch
    batch.stream_signal(torch.cuda.current_stream().cuda_stream)
    return [t.cpu().numpy() for t in tensors]


def batch_bounds(batch, members, device_arrays):
    if not device_arrays:
        return batch.lower_bound_per_bdd()
    out = sentinel(bdd_offsets(members)[-1], members)
    assert batch.lower_bound_per_bdd(out=out) is out
    return read(batch, out)[0]


def batch_grad(batch, members, g, device_arrays):
    if not device_arrays:
        return batch.grad_lower_bound_per_bdd(g)
    import torch
    n = offsets(members)[-1]
    out = (sentinel(n, members), sentinel(n, members))
    gd = dev(g)
    torch.cuda.synchronize()
    batch.stream_wait(torch.cuda.current_stream().cuda_stream)
    batch.grad_lower_bound_per_bdd(gd, out=out)
    return read(batch, *out)


def twin_grad(twins, g):
    ob = bdd_offsets(twins)
    res = [q.grad_lower_bound_per_bdd(g[ob[i]:ob[i + 1]]) for i, q in enumerate(twins)]
    return np.concatenate([r[0] for r in res]), np.concatenate([r[1] for r in res])


def set_both(batch, twins, arrays):
    off = offsets(twins)
    batch.set_solver_costs(*arrays)
    for i, q in enumerate(twins):
        set_alone(q, *(part(x, off, i) for x in arrays))


# ---------------------------------------------------------------- 1. bounds
@pytest.mark.parametrize("device_arrays", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("precision", ["float", "double"])
def test_batch_bounds_equal_each_members_own(precision, device_arrays):
    names = names_of(precision)
    members, twins = member_set(names, precision), member_set(names, precision)
    batch = bdd_hip_batch(members)
    rng = np.random.default_rng(61)

    def check(what):
        got = batch_bounds(batch, members, device_arrays)
        want = np.concatenate([q.lower_bound_per_bdd() for q in twins])
        assert got.dtype == members[0].value_type and got.shape == want.shape
        np.testing.assert_array_equal(got, want, err_msg=f"{precision}, {what}")
        assert np.any(got != 0)

    set_both(batch, twins, random_costs(members, rng))
    check("behind a batch set")
    batch.iterations(3)
    for q in twins:
        q.iterations(3)
    check("behind 3 iterations")
    # stale costs-to-terminal on two members, valid ones on the others
    for i in (1, len(members) - 1):
        v = members[i].nr_variables()
        d0, d1 = rng.uniform(-0.5, 0.5, v), rng.uniform(-0.5, 0.5, v)
        members[i].update_costs(d0, d1)
        twins[i].update_costs(d0, d1)
    check("behind update_costs on two members")
    for n, s, q in zip(names, members, twins):   # nothing but the backward state has changed
        for x, y, nm in zip(views(s), views(q), VIEWS):
            np.testing.assert_array_equal(x, y, err_msg=f"{precision}, {n}: {nm}")
    batch.close()


# ---------------------------------------------------------------- 2. gradient
@pytest.mark.parametrize("device_arrays", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("precision", ["float", "double"])
def test_batch_bound_gradient_equals_each_members_own(precision, device_arrays):
    names = names_of(precision)
    members, twins = member_set(names, precision), member_set(names, precision)
    batch = bdd_hip_batch(members)
    dt = members[0].value_type
    n, nb = int(offsets(members)[-1]), int(bdd_offsets(members)[-1])
    off = offsets(members)
    rng = np.random.default_rng(62)
    integer = lambda k: rng.integers(-2, 3, k).astype(dt)
    nonzero = lambda k: rng.choice(np.asarray([-2.0, -1.0, 1.0, 2.0]), k).astype(dt)
    cases = [("random", random_costs(members, rng)[:2], rng.normal(0, 1, nb).astype(dt)),
             ("integer", (integer(n), integer(n)), integer(nb)),
             ("zero", (np.zeros(n, dt), np.zeros(n, dt)), nonzero(nb)),
             ("zero, hi = 1 on every other layer", (np.zeros(n, dt), (np.arange(n) % 2).astype(dt)), nonzero(nb))]
    for what, (lo, hi), g in cases:
        set_both(batch, twins, (lo, hi, np.zeros(n, dt)))
        want = twin_grad(twins, g)
        if what.startswith("zero"):
            # All-zero costs: every decision between two finite paths ties, and a tie takes the hi arc.  On the twins' own output every member
            # has layers with x = 1; an assignment member also has x = 0 (behind its one hi arc the hi path is infeasible), a covering
            # member has none — in its BDDs every layer keeps a node with two finite paths, so x = 1 on every layer.  With hi = 1 on
            # every other layer the ties remain on the even layers and every member has both values.
            layer_g = np.concatenate([g[bdd_offsets(twins)[i] + np.asarray(q.get_bdd_index())] for i, q in enumerate(twins)])
            x = want[1] / layer_g
            np.testing.assert_array_equal(want[0], (1 - x) * layer_g)
            for i, nm in enumerate(names):
                xi = set(np.unique(x[off[i]:off[i + 1]]))
                assert xi == {0.0, 1.0} or (what == "zero" and not nm.startswith("assign") and xi == {1.0}), (what, nm, xi)
            assert set(np.unique(x)) == {0.0, 1.0}
        for rep in range(2):   # twice in a row
            got = batch_grad(batch, members, g, device_arrays)
            for k, nm in enumerate(("grad_lo", "grad_hi")):
                assert got[k].dtype == dt and got[k].shape == (n,)
                np.testing.assert_array_equal(got[k], want[k], err_msg=f"{precision}, {what}, call {rep}: {nm}")
        assert np.any(got[0] != 0) and np.any(got[1] != 0)
    batch.iterations(2)
    for q in twins:
        q.iterations(2)
    g = rng.normal(0, 1, nb).astype(dt)
    got, want = batch_grad(batch, members, g, device_arrays), twin_grad(twins, g)
    for k, nm in enumerate(("grad_lo", "grad_hi")):
        np.testing.assert_array_equal(got[k], want[k], err_msg=f"{precision}, behind 2 iterations: {nm}")
    for nme, s, q in zip(names, members, twins):   # arc costs, deferred differences and delta are unchanged; every getter agrees
        for x, y, nm in zip(views(s), views(q), VIEWS):
            np.testing.assert_array_equal(x, y, err_msg=f"{precision}, {nme}: {nm}")
    batch.close()


# ---------------------------------------------------------------- 3. distribute_delta
@pytest.mark.parametrize("precision", ["float", "double"])
def test_batch_distribute_delta_leaves_each_members_own_state(precision):
    names = names_of(precision)
    members, twins = member_set(names, precision), member_set(names, precision)
    batch = bdd_hip_batch(members)
    dt = members[0].value_type
    off = offsets(members)
    rng = np.random.default_rng(63)
    for round_, what in enumerate(("members that never had a distribute_delta", "behind iterations, a second time")):
        if round_ == 1:   # a pending delta that the call has to clear
            batch.iterations(2)
            for q in twins:
                q.iterations(2)
            assert any(np.any(s.get_delta() != 0) for s in members)
        arrays = random_costs(members, rng)
        assert np.any(arrays[2] > 0) and np.any(arrays[2] < 0)
        set_both(batch, twins, arrays)
        batch.distribute_delta()
        for q in twins:
            q.distribute_delta()
        for i, (n, s, q) in enumerate(zip(names, members, twins)):
            vs, vq = views(s), views(q)
            for x, y, nm in zip(vs, vq, VIEWS):
                np.testing.assert_array_equal(x, y, err_msg=f"{precision}, {what}, {n}: {nm}")
            assert not np.any(vs[2]) and not np.any(vs[3]), (what, n)   # deferred differences and delta: all zero
            assert np.any(vs[0] != arrays[0][off[i]:off[i + 1]]) and np.any(vs[1] != arrays[1][off[i]:off[i + 1]]), (what, n)
        # a member's own grad_distribute_delta afterwards reads what the batch call applied
        for i, (n, s, q) in enumerate(zip(names, members, twins)):
            g_lo, g_hi = (rng.normal(0, 1, s.nr_layers()).astype(dt) for _ in range(2))
            got, want = s.grad_distribute_delta(g_lo, g_hi), q.grad_distribute_delta(g_lo, g_hi)
            np.testing.assert_array_equal(got, want, err_msg=f"{precision}, {what}, {n}: grad_distribute_delta")
            m = arrays[2][off[i]:off[i + 1]]
            np.testing.assert_array_equal(got, np.where(m > 0, g_hi, -g_lo))
    batch.close()


# ---------------------------------------------------------------- 4. ordering without host synchronisation
@pytest.mark.parametrize("precision", ["float", "double"])
def test_member_calls_and_batch_tail_calls_order_themselves(precision):
    import torch
    names = names_of(precision)
    members, twins = member_set(names, precision), member_set(names, precision)
    batch = bdd_hip_batch(members)
    dt = members[0].value_type
    n, nb = int(offsets(members)[-1]), int(bdd_offsets(members)[-1])
    rng = np.random.default_rng(64)
    stream = torch.cuda.current_stream().cuda_stream

    def twins_do(f):
        for q in twins:
            f(q)
            q.synchronize()

    def assert_state(what):
        for nme, s, q in zip(names, members, twins):
            for x, y, nm in zip(views(s), views(q), VIEWS):
                np.testing.assert_array_equal(x, y, err_msg=f"{precision}, {what}, {nme}: {nm}")

    # ---- member iterations (which overwrite costs and costs-to-terminal) right behind each batch call
    arrays = random_costs(members, rng)
    g = rng.normal(0, 1, nb).astype(dt)
    d, gd = [dev(x) for x in arrays], dev(g)
    lb, g_lo, g_hi = sentinel(nb, members), sentinel(n, members), sentinel(n, members)
    torch.cuda.synchronize()
    batch.stream_wait(stream)
    batch.set_solver_costs(*d)
    batch.lower_bound_per_bdd(out=lb)
    for s in members:
        s.iterations(2)
    batch.grad_lower_bound_per_bdd(gd, out=(g_lo, g_hi))
    for s in members:
        s.iterations(2)
    batch.distribute_delta()
    for s in members:
        s.iterations(2)
    got = read(batch, lb, g_lo, g_hi)
    off = offsets(twins)
    for i, q in enumerate(twins):
        set_alone(q, *(part(x, off, i) for x in arrays))
        q.synchronize()
    want_lb = np.concatenate([q.lower_bound_per_bdd() for q in twins])
    twins_do(lambda q: q.iterations(2))
    want_g = twin_grad(twins, g)
    twins_do(lambda q: q.iterations(2))
    twins_do(lambda q: q.distribute_delta())
    twins_do(lambda q: q.iterations(2))
    np.testing.assert_array_equal(got[0], want_lb, err_msg=f"{precision}: bounds in front of member iterations")
    np.testing.assert_array_equal(got[1], want_g[0], err_msg=f"{precision}: grad_lo between member iterations")
    np.testing.assert_array_equal(got[2], want_g[1], err_msg=f"{precision}: grad_hi between member iterations")
    assert_state("member iterations behind the batch calls")
    # ---- each batch call right behind 50 queued member iterations
    g = rng.normal(0, 1, nb).astype(dt)
    gd = dev(g)
    torch.cuda.synchronize()
    batch.stream_wait(stream)
    for s in members:
        s.iterations(50)
    batch.lower_bound_per_bdd(out=lb)
    for s in members:
        s.iterations(50)
    batch.grad_lower_bound_per_bdd(gd, out=(g_lo, g_hi))
    for s in members:
        s.iterations(50)
    batch.distribute_delta()
    got = read(batch, lb, g_lo, g_hi)
    twins_do(lambda q: q.iterations(50))
    want_lb = np.concatenate([q.lower_bound_per_bdd() for q in twins])
    twins_do(lambda q: q.iterations(50))
    want_g = twin_grad(twins, g)
    twins_do(lambda q: q.iterations(50))
    twins_do(lambda q: q.distribute_delta())
    np.testing.assert_array_equal(got[0], want_lb, err_msg=f"{precision}: bounds behind 50 member iterations")
    np.testing.assert_array_equal(got[1], want_g[0], err_msg=f"{precision}: grad_lo behind 50 member iterations")
    np.testing.assert_array_equal(got[2], want_g[1], err_msg=f"{precision}: grad_hi behind 50 member iterations")
    assert_state("batch calls behind member iterations")
    batch.close()


# ---------------------------------------------------------------- 5. refusals
def test_refusals_are_decided_before_any_member_or_output_is_touched():
    import torch
    names = ("assign8", "cover40x60", "cover67x100", "assign3")
    members = member_set(names, "float")
    batch = bdd_hip_batch(members)
    L, h = batch._L, batch._h
    dt = members[0].value_type
    n, nb = int(offsets(members)[-1]), int(bdd_offsets(members)[-1])
    ob = bdd_offsets(members)
    rng = np.random.default_rng(65)
    batch.set_solver_costs(*random_costs(members, rng))
    batch.iterations(2)
    before = [state(s) for s in members]

    def unchanged(what):
        for nme, s, bf in zip(names, members, before):
            for x, y, nm in zip(state(s), bf, VIEWS):
                np.testing.assert_array_equal(x, y, err_msg=f"{what}, {nme}: {nm}")

    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    g = rng.normal(0, 1, nb).astype(dt)
    lo, hi, lb = np.full(n, -7.0, dt), np.full(n, -7.0, dt), np.full(nb, -7.0, dt)
    # a null array
    for on_device in (0, 1):
        assert L.bddmma_lower_bound_per_bdd_batch(h, None, on_device) == capi.ERR_INVALID_ARGUMENT
        for args in ((None, ptr(lo), ptr(hi)), (ptr(g), None, ptr(hi)), (ptr(g), ptr(lo), None)):
            assert L.bddmma_grad_lower_bound_per_bdd_batch(h, *args, on_device) == capi.ERR_INVALID_ARGUMENT
        assert b"null" in L.bddmma_batch_last_error(h)
    unchanged("null arrays")
    # a NaN inside the third member's part of grad_lb, and an infinity behind it in the fourth's
    bad = g.copy()
    bad[ob[2] + 1] = np.nan
    bad[ob[3]] = np.inf
    msg = refused(capi.ERR_INVALID_ARGUMENT, lambda: batch._check(L.bddmma_grad_lower_bound_per_bdd_batch(h, ptr(bad), ptr(lo), ptr(hi), 0), h))
    assert "member 2" in msg and "grad_lb_per_bdd" in msg, msg
    d_lo, d_hi = sentinel(n, members), sentinel(n, members)
    d_bad = dev(bad)
    torch.cuda.synchronize()
    msg = refused(capi.ERR_INVALID_ARGUMENT, lambda: batch.grad_lower_bound_per_bdd(d_bad, out=(d_lo, d_hi)))
    assert "member 2" in msg and "grad_lb_per_bdd" in msg, msg
    torch.cuda.synchronize()
    assert np.all(lo == -7.0) and np.all(hi == -7.0) and bool((d_lo == -7.0).all()) and bool((d_hi == -7.0).all())
    unchanged("a NaN in grad_lb")
    got = batch.grad_lower_bound_per_bdd(g)   # and accepted again
    assert np.all(np.isfinite(got[0])) and np.any(got[1] != 0)
    # a member with an L-BFGS wrapper attached
    before = [state(s) for s in members]
    wrapper = bdd_hip_lbfgs(members[2])
    calls = (lambda: batch._check(L.bddmma_lower_bound_per_bdd_batch(h, ptr(lb), 0), h),
             lambda: batch.lower_bound_per_bdd(out=d_lo),
             lambda: batch._check(L.bddmma_grad_lower_bound_per_bdd_batch(h, ptr(g), ptr(lo), ptr(hi), 0), h),
             lambda: batch.grad_lower_bound_per_bdd(dev(g), out=(d_lo, d_hi)),
             batch.distribute_delta)
    for call in calls:
        msg = refused(capi.ERR_STATE, call)
        assert "member 2" in msg and "L-BFGS" in msg, msg
    torch.cuda.synchronize()
    assert np.all(lb == -7.0) and np.all(lo == -7.0) and np.all(hi == -7.0) and bool((d_lo == -7.0).all()) and bool((d_hi == -7.0).all())
    unchanged("an L-BFGS wrapper")
    wrapper.close()
    batch.close()


# ---------------------------------------------------------------- 6. autograd
COUNTED = [(bdd_hip_batch, "set_solver_costs"), (bdd_hip_batch, "get_solver_costs"), (bdd_hip_batch, "distribute_delta"),
           (bdd_hip_batch, "lower_bound_per_bdd"), (bdd_hip_batch, "grad_lower_bound_per_bdd"),
           (bdd_hip_parallel_mma, "set_solver_costs"), (bdd_hip_parallel_mma, "get_solver_costs"), (bdd_hip_parallel_mma, "distribute_delta"),
           (bdd_hip_parallel_mma, "lower_bound_per_bdd"), (bdd_hip_parallel_mma, "grad_lower_bound_per_bdd"),
           (bdd_hip_parallel_mma, "grad_smooth_lower_bound_per_bdd"), (bdd_hip_parallel_mma, "stream_wait"), (bdd_hip_parallel_mma, "stream_signal")]


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


def tail_inputs(a, rng):
    dt = a[0].value_type
    costs = [s.get_solver_costs() for s in a]
    lo, hi = (np.concatenate([c[k] for c in costs]) for k in range(2))
    mm = rng.uniform(-0.25, 0.25, lo.size).astype(dt)
    return lo, hi, mm


def run_tail(solvers, lo, hi, mm, g_out, g_lb, temp, tdt):
    """DistributeDeferredDelta and ComputeLowerBoundperBDD, forward and backward, each by itself: outputs and gradients as NumPy arrays, and
    the calls each made (cleared by the caller's dict)"""
    import torch
    from bdd_amd.autograd import ComputeLowerBoundperBDD, DistributeDeferredDelta
    t = [torch.tensor(v, dtype=tdt, device="cuda", requires_grad=True) for v in (lo, hi, mm)]
    out = DistributeDeferredDelta.apply(solvers, *t)
    torch.autograd.backward(out, [torch.tensor(v, dtype=tdt, device="cuda") for v in g_out])
    u = [torch.tensor(v, dtype=tdt, device="cuda", requires_grad=True) for v in (lo, hi)]
    lb = ComputeLowerBoundperBDD.apply(solvers, *u, temp)
    lb.backward(torch.tensor(g_lb, dtype=tdt, device="cuda"))
    torch.cuda.synchronize()
    return [o.detach().cpu().numpy() for o in out] + [v.grad.cpu().numpy() for v in t] + [lb.detach().cpu().numpy()] + [v.grad.cpu().numpy() for v in u]


@pytest.mark.parametrize("precision", ["float", "double"])
def test_the_tail_functions_of_a_batch_make_batch_calls_only(precision, monkeypatch):
    """On a batch DistributeDeferredDelta makes one batch set, one batch distribute_delta and one batch get; ComputeLowerBoundperBDD forward
    and backward two batch sets and one batch call each; neither makes a call on a member.  Outputs and gradients are the list form's
    bit for bit."""
    import torch
    tdt = torch.float64 if precision == "double" else torch.float32
    a, b = [fused(n, precision) for n in AUTOGRAD_MEMBERS], [fused(n, precision) for n in AUTOGRAD_MEMBERS]
    batch = bdd_hip_batch(a)
    rng = np.random.default_rng(66)
    lo, hi, mm = tail_inputs(a, rng)
    dt = a[0].value_type
    g_out = [rng.normal(0, 1, lo.size).astype(dt) for _ in range(2)]
    g_lb = rng.normal(0, 1, int(bdd_offsets(a)[-1])).astype(dt)
    calls = counters(monkeypatch)
    from bdd_amd.autograd import ComputeLowerBoundperBDD, DistributeDeferredDelta
    t = [torch.tensor(v, dtype=tdt, device="cuda") for v in (lo, hi, mm)]
    DistributeDeferredDelta.apply(batch, *t)
    n = len(a)
    zero = {k: 0 for k in calls}
    assert calls == {**zero, "batch.set_solver_costs": 1, "batch.distribute_delta": 1, "batch.get_solver_costs": 1}, calls
    calls.update(zero)
    u = [torch.tensor(v, dtype=tdt, device="cuda", requires_grad=True) for v in (lo, hi)]
    lb = ComputeLowerBoundperBDD.apply(batch, *u)
    lb.backward(torch.tensor(g_lb, dtype=tdt, device="cuda"))
    assert calls == {**zero, "batch.set_solver_costs": 2, "batch.lower_bound_per_bdd": 1, "batch.grad_lower_bound_per_bdd": 1}, calls
    calls.update(zero)
    got = run_tail(batch, lo, hi, mm, g_out, g_lb, 0.0, tdt)
    assert all(v == 0 for k, v in calls.items() if k.startswith("member.")), calls
    calls.update(zero)
    want = run_tail(list(b), lo, hi, mm, g_out, g_lb, 0.0, tdt)
    assert all(v == 0 for k, v in calls.items() if k.startswith("batch.")), calls
    assert calls["member.set_solver_costs"] == 3 * n and calls["member.distribute_delta"] == n and calls["member.grad_lower_bound_per_bdd"] == n, calls
    for x, y in zip(got, want):
        np.testing.assert_array_equal(x, y)
        assert np.any(x != 0)
    batch.close()


@pytest.mark.parametrize("why", ["smooth", "lbfgs"])
@pytest.mark.parametrize("precision", ["float", "double"])
def test_the_tail_functions_of_a_batch_keep_the_list_form_where_it_is_needed(precision, why, monkeypatch):
    """smooth_gradients_temp > 0: the backward of ComputeLowerBoundperBDD is the list form's.  A member that has had an L-BFGS wrapper: the
    batch's first call refuses with BDDMMA_ERR_STATE, touching nothing, and both Functions run the list form.  The results are the list's."""
    import torch
    tdt = torch.float64 if precision == "double" else torch.float32
    a, b = [fused(n, precision) for n in AUTOGRAD_MEMBERS], [fused(n, precision) for n in AUTOGRAD_MEMBERS]
    batch = bdd_hip_batch(a)
    rng = np.random.default_rng(67)
    lo, hi, mm = tail_inputs(a, rng)
    dt = a[0].value_type
    g_out = [rng.normal(0, 1, lo.size).astype(dt) for _ in range(2)]
    g_lb = rng.normal(0, 1, int(bdd_offsets(a)[-1])).astype(dt)
    temp = 0.5 if why == "smooth" else 0.0
    if why == "lbfgs":
        for s in (a[1], b[1]):
            wrapper = bdd_hip_lbfgs(s)
            wrapper.iteration()
            wrapper.close()
    calls = counters(monkeypatch)
    got = run_tail(batch, lo, hi, mm, g_out, g_lb, temp, tdt)
    n = len(a)
    if why == "smooth":
        assert calls["member.grad_smooth_lower_bound_per_bdd"] == n and calls["batch.grad_lower_bound_per_bdd"] == 0, calls
    else:
        assert calls["member.distribute_delta"] == n and calls["member.lower_bound_per_bdd"] == n and calls["member.grad_lower_bound_per_bdd"] == n, calls
        assert calls["batch.distribute_delta"] == 0 and calls["batch.lower_bound_per_bdd"] == 0 and calls["batch.grad_lower_bound_per_bdd"] == 0, calls
    want = run_tail(list(b), lo, hi, mm, g_out, g_lb, temp, tdt)
    for x, y in zip(got, want):
        np.testing.assert_array_equal(x, y)
    batch.close()


@pytest.mark.parametrize("precision", ["float", "double"])
def test_a_training_step_on_a_batch_equals_the_one_on_the_list(precision):
    """DualIterations -> DistributeDeferredDelta -> ComputeLowerBoundperBDD -> backward(): the DualIterations part carries the tiers of
    tests/test_gpu_small_learned.py::_assert_tiered, the tail adds none"""
    import torch
    from bdd_amd.autograd import ComputeLowerBoundperBDD, DistributeDeferredDelta, DualIterations
    tdt = torch.float64 if precision == "double" else torch.float32
    a, b = [fused(n, precision) for n in AUTOGRAD_MEMBERS], [fused(n, precision) for n in AUTOGRAD_MEMBERS]
    assert all(s.fused_small_learned() and s.fused_small_history() for s in a + b)
    batch = bdd_hip_batch(a)
    rng = np.random.default_rng(68)
    lo, hi, mm = tail_inputs(a, rng)
    dt = a[0].value_type
    w = np.concatenate([dirichlet_weights(s, rng) for s in a])
    om = np.asarray([0.5], dt)
    g_lb = rng.normal(0, 1, int(bdd_offsets(a)[-1])).astype(dt)
    results = []
    for solvers in (batch, list(b)):
        t = [torch.tensor(v, dtype=tdt, device="cuda", requires_grad=True) for v in (lo, hi, mm, w, om)]
        out = DualIterations.apply(solvers, *t[:4], 5, t[4], 3, 0.0, 1, 3, 0.9)
        lo2, hi2 = DistributeDeferredDelta.apply(solvers, *out[:3])
        lb = ComputeLowerBoundperBDD.apply(solvers, lo2, hi2)
        (lb * torch.tensor(g_lb, dtype=tdt, device="cuda")).sum().backward()
        torch.cuda.synchronize()
        results.append(([o.detach().cpu().numpy() for o in (lo2, hi2, lb)], [v.grad.cpu().numpy() for v in t]))
    batch.close()
    off = offsets(a)
    (out_b, grad_b), (out_l, grad_l) = results
    _assert_tiered(out_b, out_l, off, precision)
    _assert_tiered(grad_b, grad_l, off, precision)
    assert all(np.any(v != 0) for v in grad_b[:4])
