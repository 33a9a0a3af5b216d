"""The log-sum-exp family of a batch, one launch per wave count each (bddmma_sum_marginals_batch, bddmma_smooth_solution_batch,
bddmma_grad_smooth_lower_bound_per_bdd_batch: kernels/batchsm.hpp; GetSumMarginals and GetMarginalProbability on a batch) on the MI355X.

The reference of every comparison is a twin of each member driven alone through the per-member calls, which
tests/test_gpu_sum_marginals.py pins to the NumPy restatement.  Every comparison is bit for bit: the batch kernel runs the bodies of the
per-member sweeps (kernels/summarg.hpp) on a wave's pack and the per-layer expressions of the per-member elementwise kernels
(kernels/elementwise.hpp: ew_*), so there is no room for a tolerance.  The member sets are those of
tests/test_gpu_batch_costs.py::names_of: one pack (assign3, mostly padding lanes; assign9 with more than 64 layers on one wave), set
covers of 2, 4, 5, 7 and 10 packs (10 packs: 16 waves of which 6 are idle, float only) and mixed3x9, whose waves sweep packs of 3 and of
9 hops.  Every test asserts nr_packs() and fused_small() first (fused())."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from bdd_amd import capi  # noqa: E402
from bdd_amd.solver import bdd_hip_batch, bdd_hip_lbfgs, bdd_hip_parallel_mma  # noqa: E402
from test_gpu_batch_bounds import bdd_offsets, read, sentinel, set_both  # noqa: E402
from test_gpu_batch_costs import VIEWS, dev, fused, member_set, names_of, offsets, random_costs, refused, set_alone, part, state, views  # noqa: E402
from test_gpu_small_learned import AUTOGRAD_MEMBERS  # noqa: E402

KINDS = ("log sum-marginals", "sum-marginals", "smooth solution")


def batch_out(batch, members, kind, device_arrays):
    """the outputs of one batch call of the family as a list of NumPy arrays"""
    n = offsets(members)[-1]
    if kind == "smooth solution":
        if not device_arrays:
            return [batch.smooth_solution_per_bdd()]
        out = sentinel(n, members)
        assert batch.smooth_solution_per_bdd(out=out) is out
        return read(batch, out)
    log = kind == "log sum-marginals"
    if not device_arrays:
        return list(batch.sum_marginals_cuda(log))
    out = (sentinel(n, members), sentinel(n, members))
    batch.sum_marginals_cuda(log, out=out)
    return read(batch, *out)


def twin_out(twins, kind):
    if kind == "smooth solution":
        return [np.concatenate([q.smooth_solution_per_bdd() for q in twins])]
    res = [q.sum_marginals_cuda(False, kind == "log sum-marginals") for q in twins]
    return [np.concatenate([r[1] for r in res]), np.concatenate([r[2] for r in res])]


def batch_grad(batch, members, g, device_arrays):
    if not device_arrays:
        return batch.grad_smooth_lower_bound_per_bdd(g)
    import torch
    n = offsets(members)[-1]
    out = (sentinel(n, members), sentinel(n, members))
    gd = dev(g)
    torch.cuda.synchronize()
    batch.stream_wait(torch.cuda.current_stream().cuda_stream)
    batch.grad_smooth_lower_bound_per_bdd(gd, out=out)
    return read(batch, *out)


def twin_grad(twins, g):
    ob = bdd_offsets(twins)
    res = [q.grad_smooth_lower_bound_per_bdd(g[ob[i]:ob[i + 1]]) for i, q in enumerate(twins)]
    return np.concatenate([r[0] for r in res]), np.concatenate([r[1] for r in res])


def assert_views(names, members, twins, what):
    for n, s, q in zip(names, members, twins):
        for x, y, nm in zip(views(s), views(q), VIEWS):
            np.testing.assert_array_equal(x, y, err_msg=f"{what}, {n}: {nm}")


def assert_family(batch, members, twins, device_arrays, what):
    """the three outputs of the family equal the twins'; returns the batch's, by kind"""
    got_all = {}
    for kind in KINDS:
        got, want = batch_out(batch, members, kind, device_arrays), twin_out(twins, kind)
        assert len(got) == len(want)
        for x, y in zip(got, want):
            assert x.dtype == members[0].value_type and x.shape == y.shape
            assert not np.any(np.isnan(y)), (what, kind)
            np.testing.assert_array_equal(x, y, err_msg=f"{what}: {kind}")
            assert np.any(x != x[0]), (what, kind, "constant output")
        got_all[kind] = got
    x = got_all["smooth solution"][0]
    assert np.all((x >= 0) & (x <= 1)), what
    return got_all


# ---------------------------------------------------------------- 1. sum-marginals and the smooth solution
@pytest.mark.parametrize("device_arrays", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("precision", ["float", "double"])
def test_batch_sum_marginals_and_smooth_solutions_equal_each_members_own(precision, device_arrays):
    names = names_of(precision)
    members, twins = member_set(names, precision), member_set(names, precision)
    batch = bdd_hip_batch(members)
    dt = members[0].value_type
    n = int(offsets(members)[-1])
    rng = np.random.default_rng(81)
    rand = random_costs(members, rng)
    zero = np.zeros(n, dt)
    cases = [("random costs", rand),
             ("integer costs", (rng.integers(-2, 3, n).astype(dt), rng.integers(-2, 3, n).astype(dt), zero)),
             ("zero costs", (zero, zero, zero)),
             ("random costs times 100", ((rand[0] * 100).astype(dt), (rand[1] * 100).astype(dt), zero))]
    for what, arrays in cases:
        set_both(batch, twins, arrays)
        got = assert_family(batch, members, twins, device_arrays, f"{precision}, {what}")
        if what == "zero costs":   # logs of path counts: -inf (no path takes that side) or >= 0
            for v in got["log sum-marginals"]:
                assert np.all(np.isneginf(v) | (v >= 0))
    set_both(batch, twins, rand)
    batch.iterations(3)
    for q in twins:
        q.iterations(3)
    assert_family(batch, members, twins, device_arrays, f"{precision}, behind 3 iterations")
    # stale sweep states on two members, valid ones on the others
    for i in (1, len(members) - 1):
        v = members[i].nr_variables()
        d0, d1 = rng.uniform(-0.5, 0.5, v), rng.uniform(-0.5, 0.5, v)
        members[i].update_costs(d0, d1)
        twins[i].update_costs(d0, d1)
    assert_family(batch, members, twins, device_arrays, f"{precision}, behind update_costs on two members")
    assert_views(names, members, twins, precision)
    batch.close()


# ---------------------------------------------------------------- 2. blocked arcs
@pytest.mark.parametrize("precision", ["float", "double"])
def test_blocked_arcs_give_minus_infinity_and_one_half(precision):
    names = names_of(precision)
    members, twins = member_set(names, precision), member_set(names, precision)
    batch = bdd_hip_batch(members)
    dt = members[0].value_type
    rng = np.random.default_rng(82)
    lo, hi, mm = random_costs(members, rng)
    mm[:] = 0
    off = offsets(members)
    blocked = []
    for i, s in enumerate(members):   # lo = hi = +inf on the first layer of the member's first BDD: no root-to-top path is left in that BDD
        l = off[i] + int(np.flatnonzero(np.asarray(s.get_bdd_index()) == 0)[0])
        lo[l] = hi[l] = np.inf
        blocked.append(l)
    set_both(batch, twins, (lo, hi, mm))
    want = {kind: twin_out(twins, kind) for kind in KINDS}
    for i, l in enumerate(blocked):   # the twins' own output shows them, on every member
        sl = slice(off[i], off[i + 1])
        assert np.isneginf(want["log sum-marginals"][0][l]) and np.isneginf(want["log sum-marginals"][1][l]), names[i]
        assert np.any(want["smooth solution"][0][sl] == 0.5) and want["smooth solution"][0][l] == 0.5, names[i]
        assert want["sum-marginals"][0][l] == 0 and want["sum-marginals"][1][l] == 0, names[i]
    for device_arrays in (False, True):
        for kind in KINDS:
            got = batch_out(batch, members, kind, device_arrays)
            for x, y in zip(got, want[kind]):
                assert not np.any(np.isnan(y)), kind
                np.testing.assert_array_equal(x, y, err_msg=f"{precision}, blocked arcs: {kind}")
    batch.close()


# ---------------------------------------------------------------- 3. gradient
@pytest.mark.parametrize("device_arrays", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("precision", ["float", "double"])
def test_batch_smooth_bound_gradient_equals_each_members_own(precision, device_arrays):
    names = names_of(precision)
    members, twins = member_set(names, precision), member_set(names, precision)
    batch = bdd_hip_batch(members)
    dt = members[0].value_type
    n, nb = int(offsets(members)[-1]), int(bdd_offsets(members)[-1])
    rng = np.random.default_rng(83)
    set_both(batch, twins, random_costs(members, rng))
    every_other = rng.normal(0, 1, nb).astype(dt)
    every_other[1::2] = 0
    for what, g in (("random", rng.normal(0, 1, nb).astype(dt)), ("zero on every other BDD", every_other), ("integer", rng.integers(-2, 3, nb).astype(dt))):
        want = twin_grad(twins, g)
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
    before = [state(s) for s in members]
    got = batch_grad(batch, members, g, device_arrays)   # arc costs, deferred differences and delta are unchanged by the call
    for nme, s, bf in zip(names, members, before):
        for x, y, nm in zip(state(s), bf, VIEWS):
            np.testing.assert_array_equal(x, y, err_msg=f"{precision}, {nme}: {nm} changed")
    assert_views(names, members, twins, precision)   # ... and every getter agrees with the twin's
    batch.close()


# ---------------------------------------------------------------- 4. ordering without host synchronisation
@pytest.mark.parametrize("precision", ["float", "double"])
def test_member_calls_and_batch_smooth_calls_order_themselves(precision):
    import torch
    names = names_of(precision)
    members, twins = member_set(names, precision), member_set(names, precision)
    batch = bdd_hip_batch(members)
    dt = members[0].value_type
    n, nb = int(offsets(members)[-1]), int(bdd_offsets(members)[-1])
    rng = np.random.default_rng(84)
    stream = torch.cuda.current_stream().cuda_stream
    labels = ("log sm_lo", "log sm_hi", "sm_lo", "sm_hi", "smooth solution", "grad_lo", "grad_hi")

    def twins_do(f):
        for q in twins:
            f(q)
            q.synchronize()

    def twins_step(g, k):
        """what the batch side does below, on the twins: every call of the family with k member iterations behind (k > 0) or in front of it"""
        res = []
        for call in (lambda: twin_out(twins, KINDS[0]), lambda: twin_out(twins, KINDS[1]), lambda: twin_out(twins, KINDS[2]), lambda: twin_grad(twins, g)):
            if k < 0:
                twins_do(lambda q: q.iterations(-k))
            res += list(call())
            if k > 0:
                twins_do(lambda q: q.iterations(k))
        return res

    def batch_step(gd, outs, k):
        calls = (lambda: batch.sum_marginals_cuda(True, out=outs[0:2]), lambda: batch.sum_marginals_cuda(False, out=outs[2:4]),
                 lambda: batch.smooth_solution_per_bdd(out=outs[4]), lambda: batch.grad_smooth_lower_bound_per_bdd(gd, out=outs[5:7]))
        for call in calls:
            if k < 0:
                for s in members:
                    s.iterations(-k)
            call()
            if k > 0:
                for s in members:
                    s.iterations(k)

    # ---- member iterations (which overwrite costs and both sweep states) right behind each batch call
    arrays = random_costs(members, rng)
    g = rng.normal(0, 1, nb).astype(dt)
    d, gd = [dev(x) for x in arrays], dev(g)
    outs = tuple(sentinel(n, members) for _ in labels)
    torch.cuda.synchronize()
    batch.stream_wait(stream)
    batch.set_solver_costs(*d)
    batch_step(gd, outs, 2)
    got = read(batch, *outs)
    off = offsets(twins)
    for i, q in enumerate(twins):
        set_alone(q, *(part(x, off, i) for x in arrays))
        q.synchronize()
    want = twins_step(g, 2)
    for x, y, nm in zip(got, want, labels):
        np.testing.assert_array_equal(x, y, err_msg=f"{precision}: {nm} in front of member iterations")
    assert_views(names, members, twins, f"{precision}, member iterations behind the batch calls")
    # ---- each batch call right behind 50 queued member iterations
    g = rng.normal(0, 1, nb).astype(dt)
    gd = dev(g)
    torch.cuda.synchronize()
    batch.stream_wait(stream)
    batch_step(gd, outs, -50)
    got = read(batch, *outs)
    want = twins_step(g, -50)
    for x, y, nm in zip(got, want, labels):
        np.testing.assert_array_equal(x, y, err_msg=f"{precision}: {nm} behind 50 member iterations")
        assert np.any(x != x[0]), nm
    assert_views(names, members, twins, f"{precision}, batch calls behind member iterations")
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
    rng = np.random.default_rng(85)
    batch.set_solver_costs(*random_costs(members, rng))
    batch.iterations(2)
    before = [state(s) for s in members]

    def unchanged(what):
        for nme, s, bf in zip(names, members, before):
            for x, y, nm in zip(state(s), bf, VIEWS):
                np.testing.assert_array_equal(x, y, err_msg=f"{what}, {nme}: {nm}")

    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    g = rng.normal(0, 1, nb).astype(dt)
    lo, hi, x = np.full(n, -7.0, dt), np.full(n, -7.0, dt), np.full(n, -7.0, dt)
    # a null array on each argument
    for on_device in (0, 1):
        for log_probs in (0, 1):
            for args in ((None, ptr(hi)), (ptr(lo), None)):
                assert L.bddmma_sum_marginals_batch(h, log_probs, *args, on_device) == capi.ERR_INVALID_ARGUMENT
                assert b"null" in L.bddmma_batch_last_error(h)
        assert L.bddmma_smooth_solution_batch(h, None, on_device) == capi.ERR_INVALID_ARGUMENT
        assert b"null" in L.bddmma_batch_last_error(h)
        for args in ((None, ptr(lo), ptr(hi)), (ptr(g), None, ptr(hi)), (ptr(g), ptr(lo), None)):
            assert L.bddmma_grad_smooth_lower_bound_per_bdd_batch(h, *args, on_device) == capi.ERR_INVALID_ARGUMENT
            assert b"null" in L.bddmma_batch_last_error(h)
    assert np.all(lo == -7.0) and np.all(hi == -7.0)
    unchanged("null arrays")
    # a NaN inside the third member's part of grad_lb_per_bdd, and an infinity behind it in the fourth's
    bad = g.copy()
    bad[ob[2] + 1] = np.nan
    bad[ob[3]] = np.inf
    msg = refused(capi.ERR_INVALID_ARGUMENT, lambda: batch._check(L.bddmma_grad_smooth_lower_bound_per_bdd_batch(h, ptr(bad), ptr(lo), ptr(hi), 0), h))
    assert "member 2" in msg and "grad_lb_per_bdd" in msg, msg
    d_lo, d_hi = sentinel(n, members), sentinel(n, members)
    d_bad = dev(bad)
    torch.cuda.synchronize()
    msg = refused(capi.ERR_INVALID_ARGUMENT, lambda: batch.grad_smooth_lower_bound_per_bdd(d_bad, out=(d_lo, d_hi)))
    assert "member 2" in msg and "grad_lb_per_bdd" in msg, msg
    torch.cuda.synchronize()
    assert np.all(lo == -7.0) and np.all(hi == -7.0) and bool((d_lo == -7.0).all()) and bool((d_hi == -7.0).all())
    unchanged("a NaN in grad_lb_per_bdd")
    got = batch.grad_smooth_lower_bound_per_bdd(g)   # and accepted again
    assert np.all(np.isfinite(got[0])) and np.any(got[1] != 0)
    # a member with an L-BFGS wrapper attached
    before = [state(s) for s in members]
    wrapper = bdd_hip_lbfgs(members[2])
    calls = (lambda: batch._check(L.bddmma_sum_marginals_batch(h, 1, ptr(lo), ptr(hi), 0), h),
             lambda: batch.sum_marginals_cuda(False, out=(d_lo, d_hi)),
             lambda: batch._check(L.bddmma_smooth_solution_batch(h, ptr(x), 0), h),
             lambda: batch.smooth_solution_per_bdd(out=d_lo),
             lambda: batch._check(L.bddmma_grad_smooth_lower_bound_per_bdd_batch(h, ptr(g), ptr(lo), ptr(hi), 0), h),
             lambda: batch.grad_smooth_lower_bound_per_bdd(dev(g), out=(d_lo, d_hi)))
    for call in calls:
        msg = refused(capi.ERR_STATE, call)
        assert "member 2" in msg and "L-BFGS" in msg, msg
    torch.cuda.synchronize()
    assert np.all(x == -7.0) and np.all(lo == -7.0) and np.all(hi == -7.0) and bool((d_lo == -7.0).all()) and bool((d_hi == -7.0).all())
    unchanged("an L-BFGS wrapper")
    wrapper.close()
    batch.close()


# ---------------------------------------------------------------- 6. autograd
COUNTED = [(cls, name) for cls in (bdd_hip_batch, bdd_hip_parallel_mma)
           for name in ("set_solver_costs", "get_solver_costs", "sum_marginals_cuda", "smooth_solution_per_bdd")]
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


def run_features(solvers, lo, hi, tdt):
    """GetSumMarginals with logits and without and GetMarginalProbability: the five outputs as NumPy arrays"""
    import torch
    from bdd_amd.autograd import GetMarginalProbability, GetSumMarginals
    t = [torch.tensor(v, dtype=tdt, device="cuda") for v in (lo, hi)]
    out = list(GetSumMarginals(solvers, *t, True)) + list(GetSumMarginals(solvers, *t, False)) + [GetMarginalProbability(solvers, *t)]
    torch.cuda.synchronize()
    return [v.cpu().numpy() for v in out]


def feature_inputs(a, rng):
    dt = a[0].value_type
    n = int(offsets(a)[-1])
    return rng.uniform(-1.0, 3.0, n).astype(dt), rng.uniform(-1.0, 3.0, n).astype(dt)


@pytest.mark.parametrize("precision", ["float", "double"])
def test_the_feature_functions_of_a_batch_make_batch_calls_only(precision, monkeypatch):
    """On a batch GetSumMarginals (both get_logits) and GetMarginalProbability make one batch set and one batch call each and no call on a
    member.  The results are the list form's bit for bit."""
    import torch
    from bdd_amd.autograd import GetMarginalProbability, GetSumMarginals
    tdt = torch.float64 if precision == "double" else torch.float32
    a, b = [fused(n, precision) for n in AUTOGRAD_MEMBERS], [fused(n, precision) for n in AUTOGRAD_MEMBERS]
    batch = bdd_hip_batch(a)
    rng = np.random.default_rng(86)
    lo, hi = feature_inputs(a, rng)
    calls = counters(monkeypatch)
    zero = {k: 0 for k in calls}
    t = [torch.tensor(v, dtype=tdt, device="cuda") for v in (lo, hi)]
    for get_logits in (True, False):
        GetSumMarginals(batch, *t, get_logits)
        assert calls == {**zero, "batch.set_solver_costs": 1, "batch.sum_marginals_cuda": 1}, (get_logits, calls)
        calls.update(zero)
    GetMarginalProbability(batch, *t)
    assert calls == {**zero, "batch.set_solver_costs": 1, "batch.smooth_solution_per_bdd": 1}, calls
    calls.update(zero)
    got = run_features(batch, lo, hi, tdt)
    assert calls == {**zero, "batch.set_solver_costs": 3, "batch.sum_marginals_cuda": 2, "batch.smooth_solution_per_bdd": 1}, calls
    calls.update(zero)
    want = run_features(list(b), lo, hi, tdt)
    n = len(a)
    assert all(v == 0 for k, v in calls.items() if k.startswith("batch.")), calls
    assert calls["member.set_solver_costs"] == 3 * n and calls["member.sum_marginals_cuda"] == 2 * n and calls["member.smooth_solution_per_bdd"] == n, calls
    for x, y in zip(got, want):
        np.testing.assert_array_equal(x, y)
        assert np.any(x != x[0])
    batch.close()


@pytest.mark.parametrize("precision", ["float", "double"])
def test_the_feature_functions_of_a_batch_keep_the_list_form_where_it_is_needed(precision, monkeypatch):
    """A member that has had an L-BFGS wrapper: the batch's first call refuses with BDDMMA_ERR_STATE, touching nothing, and the functions run
    the list form.  The results are the list's."""
    import torch
    tdt = torch.float64 if precision == "double" else torch.float32
    a, b = [fused(n, precision) for n in AUTOGRAD_MEMBERS], [fused(n, precision) for n in AUTOGRAD_MEMBERS]
    batch = bdd_hip_batch(a)
    rng = np.random.default_rng(87)
    lo, hi = feature_inputs(a, rng)
    for s in (a[1], b[1]):
        wrapper = bdd_hip_lbfgs(s)
        wrapper.iteration()
        wrapper.close()
    calls = counters(monkeypatch)
    got = run_features(batch, lo, hi, tdt)
    n = len(a)
    assert calls["member.sum_marginals_cuda"] == 2 * n and calls["member.smooth_solution_per_bdd"] == n, calls
    assert calls["batch.sum_marginals_cuda"] == 0 and calls["batch.smooth_solution_per_bdd"] == 0, calls
    want = run_features(list(b), lo, hi, tdt)
    for x, y in zip(got, want):
        np.testing.assert_array_equal(x, y)
        assert np.any(x != x[0])
    batch.close()
