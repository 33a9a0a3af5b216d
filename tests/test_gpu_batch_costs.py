"""A batch's solver costs in one launch each way (bddmma_set_solver_costs_batch / bddmma_get_solver_costs_batch: kernels/batchcosts.hpp
k_small_set_batch, k_small_get_batch; bddmma_stream_wait_batch / bddmma_stream_signal_batch; DualIterations on a batch) on the MI355X.

The reference of every comparison is a twin of each member driven alone through set_solver_costs / get_solver_costs (whose backward
sweep is the BWD_PLAIN launch of backward_run).  Every comparison is bit for bit: the kernels copy, add once and take one minimum per arc,
and sum a pack's roots in double in a fixed order, which leaves no room for a tolerance.  The shapes are those of
tests/grad_small_fixtures.py in the precisions each fuses in: one pack (assign3, assign8; assign9 with 81 variables on one wave), set
covers of 2, 4, 7 and 10 packs (10 packs: 16 waves, float only) and mixed3x9, whose waves sweep packs of 3 and of 9 hops.
Every test asserts nr_packs() and fused_small() first."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from bdd_amd import capi  # noqa: E402
from bdd_amd.solver import bdd_hip_batch, bdd_hip_lbfgs, bdd_hip_parallel_mma  # noqa: E402
from grad_small_fixtures import MIXED, PACKS, SHAPES, instance, pack_hops  # noqa: E402
from test_gpu_small_learned import AUTOGRAD_MEMBERS, _assert_tiered, dirichlet_weights  # noqa: E402

VIEWS = ("lo", "hi", "deferred mm", "delta", "lower bound", "lower bound per BDD", "min-marginal differences")


def names_of(precision):
    names = [name for name, _, fused_in in SHAPES if precision in fused_in]
    assert MIXED in names and "assign9" in names and ("cover200x300" in names) == (precision == "float")
    assert {PACKS[n] for n in names} >= {1, 2, 4, 5, 7} | ({10} if precision == "float" else set())
    return names


def fused(name, precision, seed=1):
    s = bdd_hip_parallel_mma(*instance(name, seed), precision=precision)
    assert s.nr_packs() == PACKS[name], (name, s.nr_packs())
    assert s.fused_small(), name
    return s


def member_set(names, precision):
    return [fused(n, precision) for n in names]


def offsets(members):
    return np.cumsum([0] + [s.nr_layers() for s in members])


def random_costs(members, rng):
    n, dt = int(offsets(members)[-1]), members[0].value_type
    return rng.uniform(-1.0, 3.0, n).astype(dt), rng.uniform(-1.0, 3.0, n).astype(dt), rng.uniform(-0.25, 0.25, n).astype(dt)


def set_alone(s, lo, hi, mm):
    """set_solver_costs of one solver through the C-ABI with host arrays, any of them None"""
    arr = [None if x is None else np.ascontiguousarray(x, dtype=s.value_type) for x in (lo, hi, mm)]
    ptr = [None if x is None else x.ctypes.data_as(C.c_void_p) for x in arr]
    capi.check(s._L.bddmma_set_solver_costs(s._h, *ptr, 0), s._h)


def get_alone(s, want):
    """get_solver_costs of one solver through the C-ABI, only the outputs `want` marks"""
    arr = [np.zeros(s.nr_layers(), s.value_type) if w else None for w in want]
    ptr = [None if x is None else x.ctypes.data_as(C.c_void_p) for x in arr]
    capi.check(s._L.bddmma_get_solver_costs(s._h, *ptr, 0), s._h)
    return arr


def views(s):
    """what a set is seen through; the min-marginal differences need a fresh forward state, which the call makes"""
    return list(s.get_solver_costs()) + [s.get_delta(), np.float64(s.lower_bound()), s.lower_bound_per_bdd(), s.min_marginal_diff()]


def state(s):
    return list(s.get_solver_costs()) + [s.get_delta(), np.float64(s.lower_bound())]


def assert_views(members, twins, names, what):
    for n, s, q in zip(names, members, twins):
        for x, y, nm in zip(views(s), views(q), VIEWS):
            np.testing.assert_array_equal(x, y, err_msg=f"{what}, {n}: {nm}")


def dev(x):
    import torch
    return None if x is None else torch.tensor(x, device="cuda")


def part(x, off, i):
    return None if x is None else x[off[i]:off[i + 1]]


def refused(rc, make):
    with pytest.raises(capi.BddMmaError, match=f"error {rc}:") as e:
        make()
    return str(e.value)


# ---------------------------------------------------------------- 1. set
@pytest.mark.parametrize("device_arrays", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("precision", ["float", "double"])
def test_batch_set_equals_each_member_set_alone(precision, device_arrays):
    """all three arrays, then (None, None, mm), (lo, hi, None) and (lo, None, None), each from fresh random values on members that have
    iterated (non-trivial T, F and a pending delta)"""
    import torch
    names = names_of(precision)
    hops = pack_hops(instance(MIXED)[0])
    assert hops.count(3) >= 2 and hops.count(9) >= 2, hops   # waves of one workgroup with sweeps of different lengths
    members, twins = member_set(names, precision), member_set(names, precision)
    batch = bdd_hip_batch(members)
    off = offsets(members)
    rng = np.random.default_rng(51)
    for s in members + twins:
        s.iterations(3)
    for k, given in enumerate([(1, 1, 1), (0, 0, 1), (1, 1, 0), (1, 0, 0)]):
        arrays = [x if g else None for x, g in zip(random_costs(members, rng), given)]
        batch.set_solver_costs(*([dev(x) for x in arrays] if device_arrays else arrays))
        for i, q in enumerate(twins):
            set_alone(q, *(part(x, off, i) for x in arrays))
        assert_views(members, twins, names, f"{precision}, set {given}")
        if k == 1:   # and a pending delta and F of another age than T in front of the next set
            for s in members + twins:
                s.iterations(1)
    batch.set_solver_costs(None, None, None)   # nothing given: nothing done
    assert_views(members, twins, names, f"{precision}, empty set")
    torch.cuda.synchronize()
    batch.close()


# ---------------------------------------------------------------- 2. set, then iterate
@pytest.mark.parametrize("precision", ["float", "double"])
def test_iterations_behind_a_batch_set_equal_those_behind_member_sets(precision):
    names = names_of(precision)
    a, b = member_set(names, precision), member_set(names, precision)
    batch_a, batch_b = bdd_hip_batch(a), bdd_hip_batch(b)
    off = offsets(a)
    rng = np.random.default_rng(52)
    w = np.concatenate([dirichlet_weights(s, rng) for s in a])
    ov = rng.uniform(0.1, 0.9, w.size).astype(a[0].value_type)
    runs = [("iterations", lambda bt: bt.iterations(3)), ("learned, scalar omega", lambda bt: bt.learned_iterations(w, 3, omega=0.4)),
            ("learned, omega_vec", lambda bt: bt.learned_iterations(w, 3, omega_vec=ov))]
    for what, run in runs:
        lo, hi, mm = random_costs(a, rng)
        batch_a.set_solver_costs(lo, hi, mm)
        for i, q in enumerate(b):
            q.set_solver_costs(lo[off[i]:off[i + 1]], hi[off[i]:off[i + 1]], mm[off[i]:off[i + 1]])
        run(batch_a), run(batch_b)
        for x, y, nm in zip(batch_a.get_solver_costs(), batch_b.get_solver_costs(), VIEWS):
            np.testing.assert_array_equal(x, y, err_msg=f"{precision}, {what}: {nm}")
        np.testing.assert_array_equal(batch_a.lower_bounds(), batch_b.lower_bounds(), err_msg=f"{precision}, {what}")
        for n, s, q in zip(names, a, b):
            for x, y, nm in zip(state(s), state(q), VIEWS):
                np.testing.assert_array_equal(x, y, err_msg=f"{precision}, {what}, {n}: {nm}")
    batch_a.close(), batch_b.close()


# ---------------------------------------------------------------- 3. get
@pytest.mark.parametrize("precision", ["float", "double"])
def test_batch_get_equals_each_members_own(precision):
    import torch
    names = names_of(precision)
    members = member_set(names, precision)
    batch = bdd_hip_batch(members)
    off = offsets(members)
    n, dt = int(off[-1]), members[0].value_type
    rng = np.random.default_rng(53)
    w = np.concatenate([dirichlet_weights(s, rng) for s in members])
    for what, run in (("iterations", lambda: batch.iterations(5)), ("learned", lambda: batch.learned_iterations(w, 3, omega=0.6))):
        run()
        got = batch.get_solver_costs()   # no host synchronisation behind the iterations: the call orders itself
        own = [s.get_solver_costs() for s in members]
        for k, nm in enumerate(VIEWS[:3]):
            assert got[k].dtype == dt and got[k].shape == (n,)
            np.testing.assert_array_equal(got[k], np.concatenate([o[k] for o in own]), err_msg=f"{precision}, {what}: {nm}")
            assert np.any(got[k] != 0)
        for wanted in ((1, 1, 1), (0, 1, 0), (1, 0, 1), (0, 0, 1)):
            out = [torch.full((n,), -7.0, dtype=torch.float64 if dt == np.float64 else torch.float32, device="cuda") if x else None for x in wanted]
            assert batch.get_solver_costs(out=out) is not None
            batch.stream_signal(torch.cuda.current_stream().cuda_stream)   # the read below runs on torch's stream
            alone = [get_alone(s, wanted) for s in members]
            for k, nm in enumerate(VIEWS[:3]):
                if wanted[k]:
                    np.testing.assert_array_equal(out[k].cpu().numpy(), np.concatenate([o[k] for o in alone]), err_msg=f"{precision}, {what}, device {wanted}: {nm}")
                    np.testing.assert_array_equal(out[k].cpu().numpy(), got[k])
                else:
                    assert all(o[k] is None for o in alone)
        # host outputs with one or two of them left out, through the C-ABI (the Python method always asks for all three)
        for wanted in ((1, 0, 0), (0, 1, 1)):
            arr = [np.full(n, -7.0, dt) if x else None for x in wanted]
            ptr = [None if x is None else x.ctypes.data_as(C.c_void_p) for x in arr]
            batch._check(batch._L.bddmma_get_solver_costs_batch(batch._h, *ptr, 0), batch._h)
            for k in range(3):
                if wanted[k]:
                    np.testing.assert_array_equal(arr[k], got[k], err_msg=f"{precision}, {what}, host {wanted}")
    batch.close()


# ---------------------------------------------------------------- 4. ordering without host synchronisation
@pytest.mark.parametrize("precision", ["float", "double"])
def test_member_calls_and_batch_sets_order_themselves(precision):
    import torch
    names = names_of(precision)
    members, twins = member_set(names, precision), member_set(names, precision)
    batch = bdd_hip_batch(members)
    off = offsets(members)
    rng = np.random.default_rng(54)
    # a member call right behind a device-array batch set
    arrays = random_costs(members, rng)
    d = [dev(x) for x in arrays]
    torch.cuda.synchronize()
    batch.set_solver_costs(*d)
    bounds = [s.lower_bound() for s in members]
    for s in members:
        s.iterations(2)
    for i, q in enumerate(twins):
        set_alone(q, *(part(x, off, i) for x in arrays))
        q.synchronize()
        assert bounds[i] == q.lower_bound(), names[i]
        q.synchronize()
        q.iterations(2)
        q.synchronize()
    assert_views(members, twins, names, f"{precision}, member calls behind a batch set")
    # a batch set right behind queued member iterations (their launches write the costs the set replaces)
    arrays = random_costs(members, rng)
    d = [dev(x) for x in arrays]
    torch.cuda.synchronize()
    for s in members:
        s.iterations(50)
    batch.set_solver_costs(*d)
    for i, q in enumerate(twins):
        q.iterations(50)
        q.synchronize()
        set_alone(q, *(part(x, off, i) for x in arrays))
        q.synchronize()
    assert_views(members, twins, names, f"{precision}, a batch set behind member iterations")
    batch.close()


# ---------------------------------------------------------------- 5. refusals
@pytest.mark.parametrize("reason", ["profiling", "lbfgs"])
def test_refusals_name_the_member_and_leave_every_member_alone(reason):
    names = ("assign8", "cover40x60", "cover67x100", "assign3")
    members = member_set(names, "float")
    batch = bdd_hip_batch(members)
    rng = np.random.default_rng(55)
    batch.iterations(2)
    lb = None
    if reason == "profiling":
        members[2].set_profiling(True)
    else:
        lb = bdd_hip_lbfgs(members[2])
    before = [state(s) for s in members]
    arrays = random_costs(members, rng)
    out = [np.full_like(x, -7.0) for x in arrays]
    ptr = [x.ctypes.data_as(C.c_void_p) for x in out]
    for call in (lambda: batch.set_solver_costs(*arrays), lambda: batch.set_solver_costs(*[dev(x) for x in arrays]), batch.get_solver_costs,
                 lambda: batch._check(batch._L.bddmma_get_solver_costs_batch(batch._h, *ptr, 0), batch._h)):
        msg = refused(capi.ERR_STATE, call)
        assert "member 2" in msg and ("profiling" in msg if reason == "profiling" else "L-BFGS" in msg), msg
    assert all(np.all(x == -7.0) for x in out)
    for n, s, bf in zip(names, members, before):
        for x, y, nm in zip(state(s), bf, VIEWS):
            np.testing.assert_array_equal(x, y, err_msg=f"{reason}, {n}: {nm}")
    if lb is not None:
        lb.close()
    else:
        members[2].set_profiling(False)
        batch.set_solver_costs(*arrays)   # and accepted again
        np.testing.assert_array_equal(batch.get_solver_costs()[0], arrays[0])
    batch.close()


# ---------------------------------------------------------------- 6. streams
def _sleep_cycles(ms):
    """cycles for torch.cuda._sleep that keep a stream busy for about `ms` (tests/test_gpu_autograd.py)"""
    import torch
    a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    probe = 1 << 20
    torch.cuda._sleep(probe)
    torch.cuda.synchronize()
    a.record(); torch.cuda._sleep(probe); z.record()
    torch.cuda.synchronize()
    per_ms = probe / max(a.elapsed_time(z), 1e-3)
    return int(min(ms * per_ms, 2 ** 31 - 1))


@pytest.mark.parametrize("precision", ["double", "float"])
def test_batch_stream_ordering_needs_no_host_synchronisation(precision):
    """The recipe of tests/test_gpu_autograd.py::test_stream_ordering_needs_no_host_synchronisation for the batch's own pair: on a torch
    stream of its own a spin of about 30 ms, then the kernels that write the (zero-filled) inputs, then stream_wait, set, learned
    iterations, get and stream_signal with no host synchronisation in between, the inputs overwritten and the outputs read on that
    stream right behind the signal.  What that test says about hardware queues holds here too: with HIP's default of four the runtime
    may serialise the streams and hide a missing wait; the test asks for the ordering everywhere."""
    import torch
    names = names_of(precision)
    members = member_set(names, precision)
    batch = bdd_hip_batch(members)
    rng = np.random.default_rng(56)
    src = [dev(x) for x in random_costs(members, rng)] + [dev(np.concatenate([dirichlet_weights(s, rng) for s in members]))]
    torch.cuda.synchronize()
    want = [torch.empty_like(src[0]) for _ in range(3)]
    batch.set_solver_costs(*src[:3])
    batch.learned_iterations(src[3], 3, omega=0.5)
    batch.get_solver_costs(out=want)
    batch.stream_signal(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    want = [x.cpu() for x in want]
    assert all(x.abs().sum() > 0 for x in want)
    cycles = _sleep_cycles(30.0)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        t = [torch.zeros_like(x) for x in src]
        got = [torch.zeros_like(x) for x in src[:3]]
        torch.cuda.synchronize()
        torch.cuda._sleep(cycles)
        for dst, s_ in zip(t, src):
            dst.copy_(s_, non_blocking=True)
        busy = not side.query()
        batch.stream_wait(side.cuda_stream)
        batch.set_solver_costs(*t[:3])
        batch.learned_iterations(t[3], 3, omega=0.5)
        batch.get_solver_costs(out=got)
        batch.stream_signal(side.cuda_stream)
        for x in t:
            x.fill_(float("nan"))     # right behind the signal: must not reach what the batch queued
        got = [x.cpu() for x in got]   # read on the same stream
    torch.cuda.synchronize()
    print(f"{precision}: spin of {cycles} cycles; the stream was still busy when the batch was called: {busy}")
    for x, y in zip(got, want):
        assert torch.equal(x, y)
    batch.close()


# ---------------------------------------------------------------- 7. autograd
COUNTED = [(bdd_hip_batch, "set_solver_costs"), (bdd_hip_batch, "get_solver_costs"), (bdd_hip_parallel_mma, "set_solver_costs"),
           (bdd_hip_parallel_mma, "get_solver_costs"), (bdd_hip_parallel_mma, "stream_wait"), (bdd_hip_parallel_mma, "stream_signal")]


@pytest.mark.parametrize("per_layer_omega", [False, True], ids=["omega", "omega_vec"])
@pytest.mark.parametrize("precision", ["float", "double"])
def test_dual_iterations_of_a_batch_transfer_the_costs_in_batch_calls(precision, per_layer_omega, monkeypatch):
    """5 iterations of which 3 are tracked: the batch form makes two bdd_hip_batch.set_solver_costs calls (forward, backward), one
    get_solver_costs and no per-solver set, get, stream_wait or stream_signal; the list form's counts are what they were; outputs and
    gradients agree, tiered as tests/test_gpu_small_learned.py::_assert_tiered"""
    import torch
    from bdd_amd.autograd import DualIterations
    calls = {}

    def count(cls, name):
        f, key = getattr(cls, name), f"{cls.__name__}.{name}"
        calls[key] = 0

        def wrapper(*a, **kw):
            calls[key] += 1
            return f(*a, **kw)
        monkeypatch.setattr(cls, name, wrapper)

    tdt = torch.float64 if precision == "double" else torch.float32
    a = [fused(n, precision) for n in AUTOGRAD_MEMBERS]
    b = [fused(n, precision) for n in AUTOGRAD_MEMBERS]
    assert all(s.fused_small_learned() for s in a + b)
    batch = bdd_hip_batch(a)
    dt = a[0].value_type
    rng = np.random.default_rng(57)
    costs = [s.get_solver_costs() for s in a]
    lo, hi = (np.concatenate([c[k] for c in costs]) for k in range(2))
    mm = rng.uniform(-0.25, 0.25, lo.size).astype(dt)
    w = np.concatenate([dirichlet_weights(s, rng) for s in a])
    om = rng.uniform(0.1, 0.9, lo.size).astype(dt) if per_layer_omega else np.asarray([0.5], dt)
    g = [rng.normal(0, 1, lo.size).astype(dt) for _ in range(3)]
    for cls, name in COUNTED:
        count(cls, name)
    results, seen = [], []
    for solvers in (batch, list(b)):
        for k in calls:
            calls[k] = 0
        t = [torch.tensor(v, dtype=tdt, device="cuda", requires_grad=True) for v in (lo, hi, mm, w, om)]
        out = DualIterations.apply(solvers, *t[:4], 5, t[4], 3, 0.0, 1, 0, 0.9)
        torch.autograd.backward(out[:3], [torch.tensor(v, dtype=tdt, device="cuda") for v in g])
        torch.cuda.synchronize()
        results.append(([o.detach().cpu().numpy() for o in out if o is not None], [v.grad.cpu().numpy() for v in t]))
        seen.append(dict(calls))
    batch.close()
    n = len(b)
    assert seen[0] == {"bdd_hip_batch.set_solver_costs": 2, "bdd_hip_batch.get_solver_costs": 1, "bdd_hip_parallel_mma.set_solver_costs": 0,
                       "bdd_hip_parallel_mma.get_solver_costs": 0, "bdd_hip_parallel_mma.stream_wait": 0, "bdd_hip_parallel_mma.stream_signal": 0}, seen
    assert seen[1] == {"bdd_hip_batch.set_solver_costs": 0, "bdd_hip_batch.get_solver_costs": 0, "bdd_hip_parallel_mma.set_solver_costs": 2 * n,
                       "bdd_hip_parallel_mma.get_solver_costs": n, "bdd_hip_parallel_mma.stream_wait": 2 * n, "bdd_hip_parallel_mma.stream_signal": 2 * n}, seen
    off = np.cumsum([0] + [s.nr_layers() for s in a])
    (out_b, grad_b), (out_l, grad_l) = results
    _assert_tiered(out_b, out_l, off, precision)
    _assert_tiered(grad_b, grad_l, off, precision)
    assert all(np.any(v != 0) for v in grad_b)
