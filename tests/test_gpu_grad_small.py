"""The batch backward of the learned iterations (bddmma_grad_learned_iterations_batch: kernels/gradsmall.hpp k_grad_small_batch,
BatchT::grad_learned_iterations; bdd_hip_batch.grad_iterations; DualIterations.backward on a batch) on the MI355X.

1. the exact fixtures of tests/grad_small_fixtures.py against the NumPy restatement, bit for bit (tests/test_grad_small_fixtures.py
   asserts on the CPU that the restatement is exact on them, with a fifth to two thirds of the deciding minima exact ties);
2. a batch against each member's twin on the four-launch path (variant_flags bit 19) driven alone through grad_iterations: bit-equal in
   float and on the assign* members in double; on the cover* members (and the mixed cover) in double within 4 x the deviation of the
   restatement in double from the restatement in long double on the same inputs, per output, with the per-BDD / per-variable floors of
   tests/test_gpu_grad_iterations.py — there the fused forward adds a variable's more than two terms in another order than the
   four-launch exchange's atomics;
3. the state contract and calls on a member right behind the batch's; 4. the refusals; 5. autograd.
Every test asserts nr_packs(), fused_small_learned() and the twin's `not fused_small()` first."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from bdd_amd import capi  # noqa: E402
from bdd_amd.solver import bdd_hip_batch, bdd_hip_lbfgs, bdd_hip_parallel_mma  # noqa: E402
from grad_small_fixtures import EXACT_LONG, EXACT_SEEDS, MIXED, PACKS, SHAPES, exact_reference, instance, model_of, pack_hops  # noqa: E402
from test_gpu_small_learned import AUTOGRAD_MEMBERS, SEQ, _assert_tiered, dirichlet_weights  # noqa: E402
from test_gpu_small_learned import instance as learned_instance  # noqa: E402

GRADS = ("grad_lo", "grad_hi", "grad_mm", "grad_dist_weights", "grad_omega")


def names_of(precision):
    return [name for name, _, fused_in in SHAPES if precision in fused_in]


def fused(name, precision, seed=1):
    s = bdd_hip_parallel_mma(*instance(name, seed), precision=precision)
    assert s.nr_packs() == PACKS[name], (name, s.nr_packs())
    assert s.fused_small() and s.fused_small_learned(), (name, s.fused_small(), s.fused_small_learned())
    return s


def sequential(name, precision, seed=1):
    q = bdd_hip_parallel_mma(*instance(name, seed), precision=precision, variant_flags=SEQ)
    assert not q.fused_small() and not q.fused_small_learned()
    return q


def state(s):
    return list(s.get_solver_costs()) + [s.get_delta(), np.float64(s.lower_bound())]


def assert_state(s, before, what=""):
    for x, y, nm in zip(state(s), before, ("lo", "hi", "deferred mm", "delta", "lower bound")):
        np.testing.assert_array_equal(x, y, err_msg=f"{what} {nm}")


def to_public(x, perm, dt):
    out = np.empty(len(x), dt)
    out[perm] = x
    return out


def split(arrays, members, scalar_omega):
    """the five outputs of a batch call per member"""
    off = np.cumsum([0] + [s.nr_layers() for s in members])
    out = []
    for i in range(len(members)):
        sl = slice(off[i], off[i + 1])
        out.append([a[sl] for a in arrays[:4]] + [arrays[4][i:i + 1] if scalar_omega else arrays[4][sl]])
    return out


# ---------------------------------------------------------------- 1. exact fixtures against the restatement
def _exact_case(names, seeds, precision, omega_vec, untracked, tracked):
    members = [fused(n, precision) for n in names]
    dt = members[0].value_type
    batch = bdd_hip_batch(members)
    refs, perms, pubs = [], [], []
    for n, seed, s in zip(names, seeds, members):
        ref = exact_reference(n, seed, omega_vec, untracked, tracked)
        perm = s.bdd_major_order()
        np.testing.assert_array_equal(model_of(n).layer_var, s.get_primal_variable_index()[perm])
        pub = {k: to_public(v, perm, dt) for k, v in ref["x"].items() if isinstance(v, np.ndarray)}
        s.set_solver_costs(pub["lo"], pub["hi"], np.zeros(s.nr_layers(), dt))
        refs.append(ref), perms.append(perm), pubs.append(pub)
    cat = lambda k: np.concatenate([p[k] for p in pubs])
    omega = dict(omega_vec=cat("omega_vec")) if omega_vec else dict(omega=1.0)
    before = [state(s) for s in members]
    for call in range(2):
        got = batch.grad_iterations(cat("alpha"), cat("g_lo"), cat("g_hi"), cat("g_mm"), track_grad_after_itr=untracked, track_grad_for_num_itr=tracked,
                                    num_caches=1 + call, **omega)
        for n, s, ref, perm, mine, b in zip(names, members, refs, perms, split(got, members, not omega_vec), before):
            what = f"{n} {precision} {'omega_vec' if omega_vec else 'omega'} {untracked}+{tracked}, call {call}"
            for g, want, nm in zip(mine, ref["grads"], GRADS):
                assert g.dtype == dt
                if nm == "grad_omega" and not omega_vec:   # the scalar: the per-layer values summed in double (exact)
                    want = np.array([want.astype(np.float64).sum()])
                else:
                    g = g[perm]
                np.testing.assert_array_equal(g, np.asarray(want).astype(dt), err_msg=f"{what}: {nm}")
            assert_state(s, b, what)
    batch.close()


@pytest.mark.parametrize("omega_vec", [False, True], ids=["omega", "omega_vec"])
@pytest.mark.parametrize("precision", ["float", "double"])
def test_exact_fixtures_equal_the_restatement_bit_for_bit(precision, omega_vec):
    names = names_of(precision)
    assert MIXED in names and "assign9" in names and ("cover200x300" in names) == (precision == "float")
    hops = pack_hops(instance(MIXED)[0])
    assert hops.count(3) >= 2 and hops.count(9) >= 2, hops   # waves of one workgroup with sweeps of different lengths
    _exact_case(names, [EXACT_SEEDS[n][omega_vec] for n in names], precision, omega_vec, 1, 2)


@pytest.mark.parametrize("precision", ["float", "double"])
def test_exact_fixtures_of_five_tracked_iterations(precision):
    names = sorted(EXACT_LONG)
    _exact_case(names, [EXACT_LONG[n] for n in names], precision, False, 2, 5)


# ---------------------------------------------------------------- 2. a batch against its members driven alone
AFTER, TRACK = 2, 5
_RANDOM = {}


def _random_case(precision, omega_vec):
    """members, their four-launch twins' results of grad_iterations(2 untracked + 5 tracked), the inputs — computed once per case and left
    unchanged; every member holds its start state again (the state contract)"""
    key = (precision, omega_vec)
    if key in _RANDOM:
        return _RANDOM[key]
    names = names_of(precision)
    members = [fused(n, precision) for n in names]
    twins = [sequential(n, precision) for n in names]
    dt = members[0].value_type
    rng = np.random.default_rng(31 + omega_vec)
    x = dict(w=[], lo=[], hi=[], mm=[], g_lo=[], g_hi=[], g_mm=[], ov=[])
    for s, q in zip(members, twins):
        L = s.nr_layers()
        lo, hi, _ = s.get_solver_costs()
        mm = rng.uniform(-0.25, 0.25, L).astype(dt)
        for t in (s, q):
            t.set_solver_costs(lo, hi, mm)
        x["lo"].append(lo), x["hi"].append(hi), x["mm"].append(mm)
        x["w"].append(dirichlet_weights(s, rng))
        x["ov"].append(rng.uniform(0.1, 0.9, L).astype(dt))
        for k in ("g_lo", "g_hi", "g_mm"):
            x[k].append(rng.normal(0, 1, L).astype(dt))
    want = []
    for i, q in enumerate(twins):
        om = dict(omega_vec=x["ov"][i]) if omega_vec else dict(omega=0.5)
        want.append(q.grad_iterations(x["w"][i], x["g_lo"][i], x["g_hi"][i], x["g_mm"][i], track_grad_after_itr=AFTER, track_grad_for_num_itr=TRACK, num_caches=1, **om))
    _RANDOM[key] = (names, members, x, want)
    return _RANDOM[key]


def _batch_call(batch, x, idx, omega_vec, num_caches):
    cat = lambda k: np.concatenate([x[k][i] for i in idx])
    om = dict(omega_vec=cat("ov")) if omega_vec else dict(omega=0.5)
    return batch.grad_iterations(cat("w"), cat("g_lo"), cat("g_hi"), cat("g_mm"), track_grad_after_itr=AFTER, track_grad_for_num_itr=TRACK,
                                 num_caches=num_caches, **om)


def _double_allowance(name, s, x, i, omega_vec):
    """per output: max(4 * |restatement in double - restatement in long double|, the floors of tests/test_gpu_grad_iterations.py)"""
    m = model_of(name)
    perm = s.bdd_major_order()
    major = {k: np.asarray(x[k][i], np.float64)[perm] for k in ("lo", "hi", "mm", "w", "g_lo", "g_hi", "g_mm", "ov")}
    omega = major["ov"] if omega_vec else 0.5
    runs = []
    for R in (np.float64, np.longdouble):
        start = m.iterate(major["lo"], major["hi"], major["mm"], major["w"], omega, AFTER, R)
        runs.append(m.grad_iterations(*start, major["w"], omega, TRACK, major["g_lo"], major["g_hi"], major["g_mm"], R))
    eps = np.finfo(np.float64).eps
    inc = np.abs(major["g_lo"]) + np.abs(major["g_hi"]) + np.abs(major["g_mm"])
    bdd = m.layer_bdd()
    per_bdd = 16 * eps * np.bincount(bdd, weights=inc, minlength=m.n_bdds)[bdd]
    per_var = 16 * eps * np.bincount(m.layer_var, weights=inc, minlength=m.n_vars)[m.layer_var]
    floors = [per_bdd, per_bdd, per_var, per_bdd, per_bdd if omega_vec else np.array([16 * eps * inc.sum()])]
    tols, devs = [], []
    for k, nm in enumerate(GRADS):
        low, ref = runs[0][k], runs[1][k]
        if nm == "grad_omega" and not omega_vec:
            low, ref = np.array([low.astype(np.float64).sum()]), np.array([ref.sum()])
        dev = float(np.max(np.abs(low.astype(np.longdouble) - ref)))
        devs.append(dev)
        tols.append(np.maximum(4 * dev, floors[k]))
    return tols, devs, perm


@pytest.mark.parametrize("omega_vec", [False, True], ids=["omega", "omega_vec"])
@pytest.mark.parametrize("precision", ["float", "double"])
def test_batch_equals_each_member_on_the_four_launch_path(precision, omega_vec):
    names, members, x, want = _random_case(precision, omega_vec)
    before = [state(s) for s in members]
    batch = bdd_hip_batch(members)
    idx = list(range(len(members)))
    results = {c: _batch_call(batch, x, idx, omega_vec, c) for c in (1, 2, 5)}
    again = _batch_call(batch, x, idx, omega_vec, 1)
    for c in (2, 5):   # num_caches does not change the result
        for a, b, nm in zip(results[1], results[c], GRADS):
            np.testing.assert_array_equal(a, b, err_msg=f"num_caches 1 against {c}: {nm}")
    for a, b, nm in zip(results[1], again, GRADS):
        np.testing.assert_array_equal(a, b, err_msg=f"second call: {nm}")
    for i, (name, s, mine) in enumerate(zip(names, members, split(results[1], members, not omega_vec))):
        what = f"{name} {precision} {'omega_vec' if omega_vec else 'omega'}"
        if precision == "float" or name.startswith("assign"):
            for g, w, nm in zip(mine, want[i], GRADS):
                np.testing.assert_array_equal(g, w, err_msg=f"{what}: {nm}")
        else:
            assert s.get_num_bdds_per_var().max() > 2
            tols, devs, perm = _double_allowance(name, s, x, i, omega_vec)
            for g, w, tol, dev, nm in zip(mine, want[i], tols, devs, GRADS):
                per_layer = g.size == s.nr_layers()
                err = np.abs(np.asarray(g, np.longdouble) - np.asarray(w, np.longdouble)).astype(np.float64)
                err = err[perm] if per_layer else err
                print(f"{what} {nm}: restatement double vs long double {dev:.3e}; batch vs four-launch twin {err.max():.3e}; allowed (min over entries) "
                      f"{tol.min():.3e}; largest |value| {float(np.abs(w).max()):.3e}")
                assert np.all(err <= tol), (what, nm, float(err.max()), float(tol.min()))
        assert_state(s, before[i], what)
    batch.close()
    # a batch of one member equals the batch of many on that member
    for i in (0, len(members) - 1):
        one = bdd_hip_batch([members[i]])
        got = _batch_call(one, x, [i], omega_vec, 1)
        for g, w, nm in zip(got, split(results[1], members, not omega_vec)[i], GRADS):
            np.testing.assert_array_equal(g, w, err_msg=f"batch of one, {names[i]}: {nm}")
        one.close()


# ---------------------------------------------------------------- 3. state contract and interleaving
@pytest.mark.parametrize("device_arrays", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("precision", ["float", "double"])
def test_state_contract_and_a_member_call_right_behind(precision, device_arrays):
    import torch
    names = names_of(precision)
    members = [fused(n, precision, 2) for n in names]
    twins = [fused(n, precision, 2) for n in names]
    rng = np.random.default_rng(33)
    w = [dirichlet_weights(s, rng) for s in members]
    for i, (s, t) in enumerate(zip(members, twins)):   # a state with deferred differences and a delta; every second member's costs updated since
        for u in (s, t):
            u.iterations(2)
        if i % 2:
            d = rng.uniform(-0.5, 0.5, size=s.nr_variables())
            s.update_costs([], d)
            t.update_costs([], d)
    before = [state(s) for s in members]
    batch = bdd_hip_batch(members)
    dt = members[0].value_type
    n = sum(s.nr_layers() for s in members)
    g = [rng.normal(0, 1, n).astype(dt) for _ in range(3)]
    if device_arrays:
        put = lambda a: torch.tensor(a, device="cuda")
        t_g = [put(a) for a in g]
        out = (torch.empty(n, dtype=t_g[0].dtype, device="cuda"), torch.empty(len(members), dtype=t_g[0].dtype, device="cuda"))
        res = batch.grad_iterations(put(np.concatenate(w)), *t_g, omega=0.4, track_grad_after_itr=1, track_grad_for_num_itr=3, out=out)
        assert res[0] is t_g[0] and res[3] is out[0]
        for s, wi in zip(members, w):   # right behind it, without the host having waited
            assert s.learned_iterations(wi, 2, 0.5, improvement_slope=0.0) == 2
        torch.cuda.synchronize()
        res = [r.cpu().numpy() for r in res]
    else:
        res = batch.grad_iterations(np.concatenate(w), *g, omega=0.4, track_grad_after_itr=1, track_grad_for_num_itr=3)
        for a, b in zip(res[:3], g):
            assert a is not b   # new arrays
        for s, b, name in zip(members, before, names):
            assert_state(s, b, name)
        for s, wi in zip(members, w):
            assert s.learned_iterations(wi, 2, 0.5, improvement_slope=0.0) == 2
    assert all(np.all(np.isfinite(r)) for r in res) and np.any(res[0] != g[0]) and np.any(res[3] != 0)
    for s, t, wi, name in zip(members, twins, w, names):
        assert t.learned_iterations(wi, 2, 0.5, improvement_slope=0.0) == 2
        assert_state(s, state(t), f"{name}: learned_iterations behind the batch call")
    batch.close()


# ---------------------------------------------------------------- 4. refusals
def refused(rc, make):
    with pytest.raises(capi.BddMmaError, match=f"error {rc}:") as e:
        make()
    return str(e.value)


def test_refusals_leave_every_member_untouched():
    names = ("assign8", "cover40x60", "cover67x100", "assign3")
    members = [fused(n, "float") for n in names]
    batch = bdd_hip_batch(members)
    rng = np.random.default_rng(34)
    w = [dirichlet_weights(s, rng) for s in members]
    g = [[rng.normal(0, 1, s.nr_layers()).astype(np.float32) for s in members] for _ in range(3)]
    cat = np.concatenate
    batch.learned_iterations(cat(w), 2)
    before = [state(s) for s in members]
    call = lambda w_=w, g_=g, **kw: batch.grad_iterations(cat(w_), cat(g_[0]), cat(g_[1]), cat(g_[2]), track_grad_after_itr=1, track_grad_for_num_itr=2, **kw)

    def unchanged():
        for s, b, name in zip(members, before, names):
            assert_state(s, b, name)

    bad_g = [[a.copy() for a in arr] for arr in g]
    bad_g[1][2][7] = np.nan
    msg = refused(capi.ERR_INVALID_ARGUMENT, lambda: call(g_=bad_g))
    assert "member 2" in msg and "grad_hi" in msg
    unchanged()
    bad_w = [a.copy() for a in w]
    bad_w[1][3] = -0.5
    msg = refused(capi.ERR_INVALID_ARGUMENT, lambda: call(w_=bad_w))
    assert "member 1" in msg and "dist_weights" in msg
    unchanged()
    refused(capi.ERR_INVALID_ARGUMENT, lambda: call(omega=-1.0))
    unchanged()
    # a null grad_mm: below the Python layer, which would not pass one
    n = sum(s.nr_layers() for s in members)
    arr = [cat(w)] + [cat(a).copy() for a in g] + [np.zeros(n, np.float32), np.zeros(len(members), np.float32)]
    p = [a.ctypes.data for a in arr]
    rc = batch._L.bddmma_grad_learned_iterations_batch(batch._h, p[0], None, 0.5, p[1], p[2], None, p[4], p[5], 1, 2, 1, 0)
    assert rc == capi.ERR_INVALID_ARGUMENT and b"null" in batch._L.bddmma_batch_last_error(batch._h)
    unchanged()
    # no tracked iteration: zero outputs, the in-out arrays as they were
    res = batch.grad_iterations(cat(w), cat(g[0]), cat(g[1]), cat(g[2]), track_grad_after_itr=3, track_grad_for_num_itr=0)
    for r, a in zip(res[:3], g):
        np.testing.assert_array_equal(r, cat(a))
    assert res[3].size == n and not res[3].any() and res[4].size == len(members) and not res[4].any()
    unchanged()
    wrapper = bdd_hip_lbfgs(members[3])
    msg = refused(capi.ERR_STATE, call)
    assert "member 3" in msg and "L-BFGS" in msg
    unchanged()
    wrapper.close()
    batch.close()


def test_a_member_that_is_not_learned_fusable_is_refused():
    """cover160x240 in double: fused_small, not fused_small_learned (tests/test_gpu_small_learned.py)"""
    a = fused("assign8", "double")
    b = bdd_hip_parallel_mma(*learned_instance("cover160x240", 0), precision="double")
    assert b.nr_packs() == 8 and b.fused_small() and not b.fused_small_learned()
    batch = bdd_hip_batch([a, b])
    batch.iterations(2)
    before = [state(s) for s in (a, b)]
    rng = np.random.default_rng(35)
    n = a.nr_layers() + b.nr_layers()
    w = np.concatenate([dirichlet_weights(s, rng) for s in (a, b)])
    g = [rng.normal(0, 1, n) for _ in range(3)]
    msg = refused(capi.ERR_UNSUPPORTED, lambda: batch.grad_iterations(w, *g))
    assert "member 1" in msg and "fused_small_learned" in msg
    for s, bf in zip((a, b), before):
        assert_state(s, bf)
    batch.close()


# ---------------------------------------------------------------- 5. autograd
@pytest.mark.parametrize("per_layer_omega", [False, True], ids=["omega", "omega_vec"])
@pytest.mark.parametrize("precision", ["float", "double"])
def test_dual_iterations_backward_of_a_batch_is_one_batch_call(precision, per_layer_omega, monkeypatch):
    """5 iterations of which 3 are tracked: the batch form against the list form, tiered as tests/test_gpu_small_learned.py::_assert_tiered;
    the batch form makes exactly one bdd_hip_batch.grad_iterations call and no per-solver one"""
    import torch
    from bdd_amd.autograd import DualIterations
    calls = {"batch": 0, "solver": 0}
    batch_call, solver_call = bdd_hip_batch.grad_iterations, bdd_hip_parallel_mma.grad_iterations

    def count(key, f):
        def wrapper(*a, **kw):
            calls[key] += 1
            return f(*a, **kw)
        return wrapper

    monkeypatch.setattr(bdd_hip_batch, "grad_iterations", count("batch", batch_call))
    monkeypatch.setattr(bdd_hip_parallel_mma, "grad_iterations", count("solver", solver_call))
    tdt = torch.float64 if precision == "double" else torch.float32
    a = [fused(n, precision) for n in AUTOGRAD_MEMBERS]
    b = [fused(n, precision) for n in AUTOGRAD_MEMBERS]
    batch = bdd_hip_batch(a)
    dt = a[0].value_type
    rng = np.random.default_rng(36)
    costs = [s.get_solver_costs() for s in a]
    lo, hi = (np.concatenate([c[k] for c in costs]) for k in range(2))
    mm = rng.uniform(-0.25, 0.25, lo.size).astype(dt)
    w = np.concatenate([dirichlet_weights(s, rng) for s in a])
    om = rng.uniform(0.1, 0.9, lo.size).astype(dt) if per_layer_omega else np.asarray([0.5], dt)
    g = [rng.normal(0, 1, lo.size).astype(dt) for _ in range(3)]
    results, seen = [], []
    for solvers in (batch, list(b)):
        t = [torch.tensor(v, dtype=tdt, device="cuda", requires_grad=True) for v in (lo, hi, mm, w, om)]
        out = DualIterations.apply(solvers, *t[:4], 5, t[4], 3, 0.0, 1, 0, 0.9)
        torch.autograd.backward(out[:3], [torch.tensor(v, dtype=tdt, device="cuda") for v in g])
        torch.cuda.synchronize()
        results.append(([o.detach().cpu().numpy() for o in out if o is not None], [v.grad.cpu().numpy() for v in t]))
        seen.append(dict(calls))
    batch.close()
    assert seen[0] == {"batch": 1, "solver": 0}, seen
    assert seen[1] == {"batch": 1, "solver": len(b)}, seen
    off = np.cumsum([0] + [s.nr_layers() for s in a])
    (out_b, grad_b), (out_l, grad_l) = results
    _assert_tiered(out_b, out_l, off, precision)
    _assert_tiered(grad_b, grad_l, off, precision)
    assert all(np.any(v != 0) for v in grad_b)
