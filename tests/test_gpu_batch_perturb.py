"""Per-BDD solutions, cost updates and the gradient of a cost perturbation of a batch, one launch each (bddmma_bdds_solution_batch,
bddmma_update_costs_batch, bddmma_grad_cost_perturbation_batch: kernels/batchsol.hpp; ComputePerBDDSolutions and PerturbPrimalCosts on a
batch) on the MI355X.

The reference of every comparison is a twin of each member driven alone through the per-member calls.  Every comparison is bit for bit:
the batch kernels evaluate the per-member kernels' own expressions (the path pass of FWD_SOLUTION out of LDS with its tie rule;
kernels/elementwise.hpp: ew_cost_quotient, ew_cost_add, ew_grad_perturb), so there is no tolerance to choose.  The member sets are those
of tests/test_gpu_batch_costs.py::names_of — one pack (assign3, mostly padding lanes; assign9 with more than 64 layers on one wave), set
covers of 2, 4, 5, 7 and 10 packs (10 packs: 16 waves of which 6 are idle, float only) and mixed3x9, whose waves sweep packs of 3 and of
9 hops — and one more, built here: a set cover over 300 variables, more than the 256 threads of the per-variable kernel, so that its
stride loop takes a second trip.  Every test asserts nr_packs() and fused_small() first (fused(), big_member())."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from bdd_amd import capi  # noqa: E402
from bdd_amd.instances import random_set_cover  # noqa: E402
from bdd_amd.solver import bdd_hip_batch, bdd_hip_lbfgs, bdd_hip_parallel_mma  # noqa: E402
from test_gpu_batch_bounds import bdd_offsets, read, sentinel, set_both, tdt_of  # noqa: E402
from test_gpu_batch_costs import VIEWS, dev, fused, member_set, names_of, offsets, random_costs, refused, set_alone, part, state, views  # noqa: E402
from test_gpu_small_learned import AUTOGRAD_MEMBERS  # noqa: E402

BIG = "cover300x100"   # random_set_cover(300, 100, 4): 400 layers, 300 variables


def big_member(precision):
    col, costs = random_set_cover(300, 100, 4, seed=100)
    s = bdd_hip_parallel_mma(col, costs, precision=precision)
    assert s.nr_variables() > 256, s.nr_variables()   # more variables than the per-variable kernel has threads
    assert s.fused_small(), BIG
    return s


def all_names(precision):
    return list(names_of(precision)) + [BIG]


def all_members(precision):
    return member_set(names_of(precision), precision) + [big_member(precision)]


def var_offsets(members):
    return np.cumsum([0] + [s.nr_variables() for s in members])


def assert_views(names, members, twins, what):
    for n, s, q in zip(names, members, twins):
        for x, y, nm in zip(views(s), views(q), VIEWS):
            np.testing.assert_array_equal(x, y, err_msg=f"{what}, {n}: {nm}")


def sentinel8(n):
    import torch
    return torch.full((int(n),), -7, dtype=torch.int8, device="cuda")


def batch_sol(batch, members, device_arrays):
    if not device_arrays:
        return batch.bdds_solution_vec()
    out = sentinel8(offsets(members)[-1])
    assert batch.bdds_solution_vec(out=out) is out
    return read(batch, out)[0]


def twin_sol(twins):
    return np.concatenate([q.bdds_solution_vec() for q in twins])


def update_alone(q, d0, d1, device_arrays):
    """update_costs of one solver with full-length vectors, either of them None; host float64 or device REAL"""
    if device_arrays:
        q.update_costs(dev(None if d0 is None else d0.astype(q.value_type)), dev(None if d1 is None else d1.astype(q.value_type)))
        q.synchronize()
        return
    arr = [None if x is None else np.ascontiguousarray(x, dtype=np.float64) for x in (d0, d1)]
    ptr = [None if x is None else x.ctypes.data_as(C.c_void_p) for x in arr]
    capi.check(q._L.bddmma_update_costs(q._h, ptr[0], 0 if arr[0] is None else arr[0].size, ptr[1], 0 if arr[1] is None else arr[1].size, capi.F64, 0), q._h)


def batch_update(batch, members, d0, d1, device_arrays):
    if not device_arrays:
        batch.update_costs(d0, d1)
        return
    import torch
    dt = members[0].value_type
    t0, t1 = dev(None if d0 is None else d0.astype(dt)), dev(None if d1 is None else d1.astype(dt))
    torch.cuda.synchronize()
    batch.stream_wait(torch.cuda.current_stream().cuda_stream)
    batch.update_costs(t0, t1)
    batch.stream_signal(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()   # (t0 / t1 are released on return)


def batch_pert(batch, members, g_lo, g_hi, device_arrays):
    if not device_arrays:
        return batch.grad_cost_perturbation(g_lo, g_hi)
    import torch
    nv = var_offsets(members)[-1]
    out = (sentinel(nv, members), sentinel(nv, members))
    d_lo, d_hi = dev(g_lo), dev(g_hi)
    torch.cuda.synchronize()
    batch.stream_wait(torch.cuda.current_stream().cuda_stream)
    res = batch.grad_cost_perturbation(d_lo, d_hi, out=out)
    assert res[0] is out[0] and res[1] is out[1]
    return read(batch, *out)


def twin_pert(twins, g_lo, g_hi):
    off = offsets(twins)
    res = [q.grad_cost_perturbation(g_lo[off[i]:off[i + 1]], g_hi[off[i]:off[i + 1]]) for i, q in enumerate(twins)]
    return np.concatenate([r[0] for r in res]), np.concatenate([r[1] for r in res])


# ---------------------------------------------------------------- 1. solutions
@pytest.mark.parametrize("device_arrays", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("precision", ["float", "double"])
def test_batch_solutions_equal_each_members_own(precision, device_arrays):
    names = all_names(precision)
    members, twins = all_members(precision), all_members(precision)
    batch = bdd_hip_batch(members)
    dt = members[0].value_type
    off, ob = offsets(members), bdd_offsets(members)
    n = int(off[-1])
    rng = np.random.default_rng(91)
    zero = np.zeros(n, dt)

    def check(what, both=True):
        got, want = batch_sol(batch, members, device_arrays), twin_sol(twins)
        assert got.dtype == np.int8 and got.shape == (n,)
        np.testing.assert_array_equal(got, want, err_msg=f"{precision}, {what}")
        assert set(np.unique(got)) <= {0, 1}, what
        if both:
            for i, nme in enumerate(names):
                x = got[off[i]:off[i + 1]]
                assert np.any(x == 0) and np.any(x == 1), (what, nme)
        return got

    set_both(batch, twins, random_costs(members, rng))
    check("random costs")
    lo, hi = rng.integers(-2, 3, n).astype(dt), rng.integers(-2, 3, n).astype(dt)
    set_both(batch, twins, (lo, hi, zero))
    x = check("integer costs").astype(dt)
    # independent of the twins: a BDD's bound is the cost of its arg-min path (integer costs, no deferred differences: exact sums)
    per_layer = x * hi + (1 - x) * lo
    lb = batch.lower_bound_per_bdd()
    for i, s in enumerate(members):
        want = np.zeros(s.nr_bdds(), dt)
        np.add.at(want, np.asarray(s.get_bdd_index()), per_layer[off[i]:off[i + 1]])
        np.testing.assert_array_equal(want, lb[ob[i]:ob[i + 1]], err_msg=f"{precision}, {names[i]}: cost of the path against the bound")
    set_both(batch, twins, (zero, zero, zero))
    check("zero costs (every decision a tie)", both=False)
    set_both(batch, twins, random_costs(members, rng))
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


# ---------------------------------------------------------------- 2. update_costs
@pytest.mark.parametrize("device_arrays", [False, True], ids=["host float64", "device"])
@pytest.mark.parametrize("precision", ["float", "double"])
def test_batch_update_costs_equals_each_members_own(precision, device_arrays):
    names = all_names(precision)
    members, twins = all_members(precision), all_members(precision)
    batch = bdd_hip_batch(members)
    ov = var_offsets(members)
    rng = np.random.default_rng(92)
    # shares that do not divide evenly: random values on variables of three and more BDDs
    for nme, s in zip(names, members):
        if nme.startswith("cover"):
            assert np.max(s.get_num_bdds_per_var()) >= 3, nme
    set_both(batch, twins, random_costs(members, rng))
    for given in ((1, 1), (1, 0), (0, 1)):
        # members that have iterated (a pending delta, deferred differences) and whose bound has just been read (a cached one)
        batch.iterations(2)
        for q in twins:
            q.iterations(2)
        for s in members + twins:
            s.lower_bound()
        d = [rng.uniform(-1.0, 1.0, int(ov[-1])) if g else None for g in given]
        batch_update(batch, members, d[0], d[1], device_arrays)
        for i, q in enumerate(twins):
            update_alone(q, part(d[0], ov, i), part(d[1], ov, i), device_arrays)
        assert_views(names, members, twins, f"{precision}, update {given}")
    before = [views(s) for s in members]
    batch.update_costs(None, None)   # nothing given: nothing done
    for nme, s, bf in zip(names, members, before):
        for x, y, nm in zip(views(s), bf, VIEWS):
            np.testing.assert_array_equal(x, y, err_msg=f"{precision}, empty update, {nme}: {nm}")
    batch.close()


# ---------------------------------------------------------------- 3. grad_cost_perturbation
@pytest.mark.parametrize("device_arrays", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("precision", ["float", "double"])
def test_batch_perturbation_gradient_equals_each_members_own(precision, device_arrays):
    names = all_names(precision)
    members, twins = all_members(precision), all_members(precision)
    batch = bdd_hip_batch(members)
    dt = members[0].value_type
    off, ov = offsets(members), var_offsets(members)
    n, nv = int(off[-1]), int(ov[-1])
    rng = np.random.default_rng(93)
    set_both(batch, twins, random_costs(members, rng))
    batch.iterations(2)
    for q in twins:
        q.iterations(2)
    before = [state(s) for s in members]
    ints = (rng.integers(-3, 4, n).astype(dt), rng.integers(-3, 4, n).astype(dt))
    for what, (g_lo, g_hi) in (("random", (rng.normal(0, 1, n).astype(dt), rng.normal(0, 1, n).astype(dt))), ("integer", ints)):
        want = twin_pert(twins, g_lo, g_hi)
        for rep in range(2):   # twice in a row
            got = batch_pert(batch, members, g_lo, g_hi, device_arrays)
            for k, nm in enumerate(("grad_lo_pert", "grad_hi_pert")):
                assert got[k].dtype == dt and got[k].shape == (nv,)
                np.testing.assert_array_equal(got[k], want[k], err_msg=f"{precision}, {what}, call {rep}: {nm}")
        assert np.any(got[0] != 0) and np.any(got[1] != 0)
    # independent of the twins: integer gradients sum exactly; one correctly rounded division in the solver's type
    for i, (nme, s) in enumerate(zip(names, members)):
        var = np.asarray(s.get_primal_variable_index())
        nb = np.asarray(s.get_num_bdds_per_var())
        assert nb.shape == (s.nr_variables(),)
        if np.any(nb == 0):
            print(f"{nme}: {int(np.sum(nb == 0))} of {nb.size} variables are in no BDD")
        for k in range(2):
            total = np.zeros(s.nr_variables(), dt)
            np.add.at(total, var, ints[k][off[i]:off[i + 1]])
            want_v = total / np.maximum(nb, 1).astype(dt)
            assert want_v.dtype == dt
            np.testing.assert_array_equal(got[k][ov[i]:ov[i + 1]], want_v, err_msg=f"{precision}, {nme}: side {k} against NumPy")
            assert np.all(got[k][ov[i]:ov[i + 1]][nb == 0] == 0)
    for nme, s, bf in zip(names, members, before):   # no member's state changes
        for x, y, nm in zip(state(s), bf, VIEWS):
            np.testing.assert_array_equal(x, y, err_msg=f"{precision}, {nme}: {nm} changed")
    assert_views(names, members, twins, precision)
    batch.close()


# ---------------------------------------------------------------- 4. ordering without host synchronisation
@pytest.mark.parametrize("precision", ["float", "double"])
def test_member_calls_and_batch_perturb_calls_order_themselves(precision):
    import torch
    names = all_names(precision)
    members, twins = all_members(precision), all_members(precision)
    batch = bdd_hip_batch(members)
    dt = members[0].value_type
    off, ov = offsets(members), var_offsets(members)
    n, nv = int(off[-1]), int(ov[-1])
    rng = np.random.default_rng(94)
    stream = torch.cuda.current_stream().cuda_stream
    labels = ("solution", "grad_lo_pert", "grad_hi_pert")

    def twins_do(f):
        for q in twins:
            f(q)
            q.synchronize()

    def twins_step(x, k):
        """what the batch side does below, on the twins: each of the three calls with k member iterations behind (k > 0) or in front of it"""
        d0, d1, g_lo, g_hi = x
        res = []
        calls = (lambda: [twin_sol(twins)],
                 lambda: [update_alone(q, part(d0, ov, i), part(d1, ov, i), True) for i, q in enumerate(twins)][:0],
                 lambda: list(twin_pert(twins, g_lo, g_hi)))
        for call in calls:
            if k < 0:
                twins_do(lambda q: q.iterations(-k))
            res += call()
            if k > 0:
                twins_do(lambda q: q.iterations(k))
        return res

    def batch_step(xd, outs, k):
        calls = (lambda: batch.bdds_solution_vec(out=outs[0]), lambda: batch.update_costs(xd[0], xd[1]),
                 lambda: batch.grad_cost_perturbation(xd[2], xd[3], out=outs[1:3]))
        for call in calls:
            if k < 0:
                for s in members:
                    s.iterations(-k)
            call()
            if k > 0:
                for s in members:
                    s.iterations(k)

    def inputs():
        return rng.uniform(-1, 1, nv).astype(dt), rng.uniform(-1, 1, nv).astype(dt), rng.normal(0, 1, n).astype(dt), rng.normal(0, 1, n).astype(dt)

    # ---- member iterations (which overwrite costs and both sweep states) right behind each batch call
    arrays = random_costs(members, rng)
    x = inputs()
    d, xd = [dev(a) for a in arrays], [dev(a) for a in x]
    outs = (sentinel8(n), sentinel(nv, members), sentinel(nv, members))
    torch.cuda.synchronize()
    batch.stream_wait(stream)
    batch.set_solver_costs(*d)
    batch_step(xd, outs, 2)
    got = read(batch, *outs)
    for i, q in enumerate(twins):
        set_alone(q, *(part(a, off, i) for a in arrays))
        q.synchronize()
    want = twins_step(x, 2)
    for g, w, nm in zip(got, want, labels):
        np.testing.assert_array_equal(g, w, err_msg=f"{precision}: {nm} in front of member iterations")
    assert_views(names, members, twins, f"{precision}, member iterations behind the batch calls")
    # ---- each batch call right behind 50 queued member iterations
    x = inputs()
    xd = [dev(a) for a in x]
    torch.cuda.synchronize()
    batch.stream_wait(stream)
    batch_step(xd, outs, -50)
    got = read(batch, *outs)
    want = twins_step(x, -50)
    for g, w, nm in zip(got, want, labels):
        np.testing.assert_array_equal(g, w, err_msg=f"{precision}: {nm} behind 50 member iterations")
        assert np.any(g != g[0]), nm
    assert_views(names, members, twins, f"{precision}, batch calls behind member iterations")
    torch.cuda.synchronize()
    batch.close()


# ---------------------------------------------------------------- 5. refusals
def test_refusals_are_decided_before_any_member_or_output_is_touched():
    import torch
    names = ("assign8", "cover40x60", "cover67x100", "assign3")
    members = member_set(names, "float")
    batch = bdd_hip_batch(members)
    L, h = batch._L, batch._h
    dt = members[0].value_type
    off, ov = offsets(members), var_offsets(members)
    n, nv = int(off[-1]), int(ov[-1])
    rng = np.random.default_rng(95)
    batch.set_solver_costs(*random_costs(members, rng))
    batch.iterations(2)
    before = [state(s) for s in members]

    def unchanged(what):
        for nme, s, bf in zip(names, members, before):
            for x, y, nm in zip(state(s), bf, VIEWS):
                np.testing.assert_array_equal(x, y, err_msg=f"{what}, {nme}: {nm}")

    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    g_lo, g_hi = rng.normal(0, 1, n).astype(dt), rng.normal(0, 1, n).astype(dt)
    d0, d1 = rng.uniform(-1, 1, nv), rng.uniform(-1, 1, nv)
    p_lo, p_hi = np.full(nv, -7.0, dt), np.full(nv, -7.0, dt)
    sol = np.full(n, -7, np.int8)
    # a null array on each argument (update_costs has no required array: both NULL is BDDMMA_OK and nothing is done)
    for on_device in (0, 1):
        assert L.bddmma_bdds_solution_batch(h, None, on_device) == capi.ERR_INVALID_ARGUMENT
        assert b"null" in L.bddmma_batch_last_error(h)
        for k in range(4):
            args = [ptr(g_lo), ptr(g_hi), ptr(p_lo), ptr(p_hi)]
            args[k] = None
            assert L.bddmma_grad_cost_perturbation_batch(h, *args, on_device) == capi.ERR_INVALID_ARGUMENT
            assert b"null" in L.bddmma_batch_last_error(h)
        for prec in (capi.F32, capi.F64):
            assert L.bddmma_update_costs_batch(h, None, None, prec, on_device) == capi.OK
    assert np.all(p_lo == -7.0) and np.all(p_hi == -7.0) and np.all(sol == -7)
    unchanged("null arrays")
    # a NaN in the third member's part of grad_hi and an infinity in the fourth's part of grad_lo
    bad_lo, bad_hi = g_lo.copy(), g_hi.copy()
    bad_hi[off[2] + 1] = np.nan
    bad_lo[off[3]] = np.inf
    msg = refused(capi.ERR_INVALID_ARGUMENT, lambda: batch._check(L.bddmma_grad_cost_perturbation_batch(h, ptr(bad_lo), ptr(bad_hi), ptr(p_lo), ptr(p_hi), 0), h))
    assert "member 2" in msg and "grad_hi" in msg, msg
    dp_lo, dp_hi = sentinel(nv, members), sentinel(nv, members)
    db_lo, db_hi = dev(bad_lo), dev(bad_hi)
    torch.cuda.synchronize()
    msg = refused(capi.ERR_INVALID_ARGUMENT, lambda: batch.grad_cost_perturbation(db_lo, db_hi, out=(dp_lo, dp_hi)))
    assert "member 2" in msg and "grad_hi" in msg, msg
    torch.cuda.synchronize()
    assert np.all(p_lo == -7.0) and np.all(p_hi == -7.0) and bool((dp_lo == -7.0).all()) and bool((dp_hi == -7.0).all())
    unchanged("a NaN in grad_hi")
    # ... and each call is accepted again
    got = batch.grad_cost_perturbation(g_lo, g_hi)
    assert np.all(np.isfinite(got[0])) and np.any(got[1] != 0)
    assert set(np.unique(batch.bdds_solution_vec())) == {0, 1}
    batch.update_costs(d0, d1)
    assert any(np.any(x != y) for s, bf in zip(members, before) for x, y in zip(state(s)[:2], bf[:2]))
    # a member with an L-BFGS wrapper attached
    before = [state(s) for s in members]
    wrapper = bdd_hip_lbfgs(members[2])
    d_sol = sentinel8(n)
    t0, t1 = dev(d0.astype(dt)), dev(d1.astype(dt))
    torch.cuda.synchronize()
    calls = (lambda: batch._check(L.bddmma_bdds_solution_batch(h, ptr(sol), 0), h),
             lambda: batch.bdds_solution_vec(out=d_sol),
             lambda: batch.update_costs(d0, d1),
             lambda: batch.update_costs(t0, t1),
             lambda: batch.update_costs(None, None),
             lambda: batch._check(L.bddmma_grad_cost_perturbation_batch(h, ptr(g_lo), ptr(g_hi), ptr(p_lo), ptr(p_hi), 0), h),
             lambda: batch.grad_cost_perturbation(dev(g_lo), dev(g_hi), out=(dp_lo, dp_hi)))
    for call in calls:
        msg = refused(capi.ERR_STATE, call)
        assert "member 2" in msg and "L-BFGS" in msg, msg
    torch.cuda.synchronize()
    assert np.all(sol == -7) and np.all(p_lo == -7.0) and np.all(p_hi == -7.0)
    assert bool((d_sol == -7).all()) and bool((dp_lo == -7.0).all()) and bool((dp_hi == -7.0).all())
    unchanged("an L-BFGS wrapper")
    wrapper.close()
    batch.close()
    # the members that never had a wrapper, as a batch of their own: every call is accepted
    rest = [members[i] for i in (0, 1, 3)]
    batch = bdd_hip_batch(rest)
    lay, var = int(offsets(rest)[-1]), int(var_offsets(rest)[-1])
    assert set(np.unique(batch.bdds_solution_vec())) == {0, 1}
    batch.update_costs(d0[:var], None)
    got = batch.grad_cost_perturbation(g_lo[:lay], g_hi[:lay])
    assert got[0].shape == (var,) and np.any(got[0] != 0)
    batch.close()


# ---------------------------------------------------------------- 6. autograd
COUNTED = [(cls, name) for cls in (bdd_hip_batch, bdd_hip_parallel_mma)
           for name in ("set_solver_costs", "get_solver_costs", "bdds_solution_vec", "update_costs", "grad_cost_perturbation")]
COUNTED += [(bdd_hip_parallel_mma, "stream_wait"), (bdd_hip_parallel_mma, "stream_signal")]


def counters(monkeypatch):
    """calls that returned, per method (a call the library refuses raises and is not counted: a refused first call of a batch is the
    signal for the list form, not a batch call that ran)"""
    calls = {}
    for cls, name in COUNTED:
        f, key = getattr(cls, name), f"{'batch' if cls is bdd_hip_batch else 'member'}.{name}"
        calls[key] = 0

        def wrapper(*a, _f=f, _key=key, **kw):
            r = _f(*a, **kw)
            calls[_key] += 1
            return r
        monkeypatch.setattr(cls, name, wrapper)
    return calls


def autograd_inputs(a, rng):
    dt = a[0].value_type
    n, nv = int(offsets(a)[-1]), int(var_offsets(a)[-1])
    return dict(lo=rng.uniform(-1.0, 3.0, n).astype(dt), hi=rng.uniform(-1.0, 3.0, n).astype(dt), p_lo=rng.uniform(-1.0, 1.0, nv).astype(dt),
                p_hi=rng.uniform(-1.0, 1.0, nv).astype(dt), w_lo=rng.normal(0, 1, n).astype(dt), w_hi=rng.normal(0, 1, n).astype(dt),
                w_sol=rng.normal(0, 1, n).astype(dt))


def run_perturb(solvers, x, tdt, calls=None, expect=None):
    """PerturbPrimalCosts forward and backward: both outputs and all four gradients as NumPy arrays"""
    import torch
    from bdd_amd.autograd import PerturbPrimalCosts
    t = {k: torch.tensor(v, dtype=tdt, device="cuda", requires_grad=k in ("lo", "hi", "p_lo", "p_hi")) for k, v in x.items()}
    lo, hi = PerturbPrimalCosts.apply(solvers, t["p_lo"], t["p_hi"], t["lo"], t["hi"])
    if expect is not None:
        assert calls == {**expect[0], "batch.set_solver_costs": 1, "batch.update_costs": 1, "batch.get_solver_costs": 1}, calls
        calls.update(expect[0])
    ((lo * t["w_lo"]).sum() + (hi * t["w_hi"]).sum()).backward()
    if expect is not None:
        assert calls == {**expect[0], "batch.grad_cost_perturbation": 1}, calls
        calls.update(expect[0])
    torch.cuda.synchronize()
    return [v.detach().cpu().numpy() for v in (lo, hi, t["p_lo"].grad, t["p_hi"].grad, t["lo"].grad, t["hi"].grad)]


def run_solutions(solvers, x, tdt, calls=None, expect=None):
    """ComputePerBDDSolutions, and ComputePerBDDSolutionsIdentityBackward with its two gradients"""
    import torch
    from bdd_amd.autograd import ComputePerBDDSolutions, ComputePerBDDSolutionsIdentityBackward
    t = {k: torch.tensor(x[k], dtype=tdt, device="cuda", requires_grad=k in ("lo", "hi")) for k in ("lo", "hi", "w_sol")}
    plain = ComputePerBDDSolutions(solvers, t["lo"].detach(), t["hi"].detach())
    if expect is not None:
        assert calls == {**expect[0], "batch.set_solver_costs": 1, "batch.bdds_solution_vec": 1}, calls
        calls.update(expect[0])
    sol = ComputePerBDDSolutionsIdentityBackward.apply(solvers, t["lo"], t["hi"], 0.5)
    if expect is not None:
        assert calls == {**expect[0], "batch.set_solver_costs": 1, "batch.bdds_solution_vec": 1}, calls
        calls.update(expect[0])
    (sol * t["w_sol"]).sum().backward()
    if expect is not None:
        assert calls == expect[0], calls   # the straight-through backward touches no solver
    torch.cuda.synchronize()
    return [v.detach().cpu().numpy() for v in (plain, sol, t["lo"].grad, t["hi"].grad)]


@pytest.mark.parametrize("precision", ["float", "double"])
def test_the_perturbation_functions_of_a_batch_make_batch_calls_only(precision, monkeypatch):
    """On a batch ComputePerBDDSolutions makes one batch set and one batch.bdds_solution_vec, PerturbPrimalCosts one batch set, update and
    get forward and one batch.grad_cost_perturbation backward, and none makes a call on a member (its stream_wait / stream_signal
    included).  Outputs and gradients are the list form's on twin solvers bit for bit."""
    import torch
    tdt = torch.float64 if precision == "double" else torch.float32
    a, b = [fused(n, precision) for n in AUTOGRAD_MEMBERS], [fused(n, precision) for n in AUTOGRAD_MEMBERS]
    batch = bdd_hip_batch(a)
    x = autograd_inputs(a, np.random.default_rng(96))
    calls = counters(monkeypatch)
    zero = {k: 0 for k in calls}
    got = run_perturb(batch, x, tdt, calls, (zero,)) + run_solutions(batch, x, tdt, calls, (zero,))
    calls.update(zero)
    want = run_perturb(list(b), x, tdt) + run_solutions(list(b), x, tdt)
    n = len(a)
    assert all(v == 0 for k, v in calls.items() if k.startswith("batch.")), calls
    assert calls["member.update_costs"] == n and calls["member.grad_cost_perturbation"] == n and calls["member.bdds_solution_vec"] == 2 * n, calls
    assert len(got) == len(want) == 10
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == a[0].value_type
        np.testing.assert_array_equal(g, w, err_msg=f"{precision}: output {k}")
        assert np.any(g != g[0]), k
    assert set(np.unique(got[6])) == {0.0, 1.0}
    batch.close()


@pytest.mark.parametrize("precision", ["float", "double"])
def test_the_perturbation_functions_of_a_batch_keep_the_list_form_where_it_is_needed(precision, monkeypatch):
    """A member that has had an L-BFGS wrapper: the batch's first call refuses with BDDMMA_ERR_STATE, touching nothing, and the functions run
    the list form.  The results are the list's."""
    import torch
    tdt = torch.float64 if precision == "double" else torch.float32
    a, b = [fused(n, precision) for n in AUTOGRAD_MEMBERS], [fused(n, precision) for n in AUTOGRAD_MEMBERS]
    batch = bdd_hip_batch(a)
    x = autograd_inputs(a, np.random.default_rng(97))
    for s in (a[1], b[1]):
        wrapper = bdd_hip_lbfgs(s)
        wrapper.iteration()
        wrapper.close()
    calls = counters(monkeypatch)
    got = run_perturb(batch, x, tdt) + run_solutions(batch, x, tdt)
    n = len(a)
    assert all(v == 0 for k, v in calls.items() if k.startswith("batch.")), calls
    assert calls["member.update_costs"] == n and calls["member.grad_cost_perturbation"] == n and calls["member.bdds_solution_vec"] == 2 * n, calls
    want = run_perturb(list(b), x, tdt) + run_solutions(list(b), x, tdt)
    for k, (g, w) in enumerate(zip(got, want)):
        np.testing.assert_array_equal(g, w, err_msg=f"{precision}: output {k}")
        assert np.any(g != g[0]), k
    batch.close()
