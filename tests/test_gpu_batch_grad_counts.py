"""The batch backward of the learned iterations with per-member counts (bddmma_grad_learned_iterations_counts_batch: kernels/gradsmall.hpp
k_grad_small_untracked_batch and k_grad_small_counts_batch, BatchT::grad_learned_iterations_counts; bdd_hip_batch.grad_iterations_counts;
DualIterations.backward on a batch whose members stopped at different counts) on the MI355X.

1. the exact fixtures of tests/grad_counts_fixtures.py — every member with its own row — against the NumPy restatement, bit for bit, with
   a member that tracks nothing beside them (tests/test_batch_grad_counts_abi.py asserts the rows on the CPU);
2. random inputs against each member's twin on the four-launch path (variant_flags bit 19) driven alone with that member's counts, in the
   tiers of tests/test_gpu_grad_small.py::test_batch_equals_each_member_on_the_four_launch_path (its helpers, floors and factor);
3. equal counts: the call of tests/test_gpu_grad_small.py on a twin batch, array for array;
4. the state contract and member calls right behind the batch's with device arrays; 5. the refusals; 6. the workspace; 7. autograd.
Every test asserts nr_packs() and fused_small_learned() first (test_gpu_grad_small.fused)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import test_gpu_grad_small as tg  # noqa: E402
from bdd_amd import capi  # noqa: E402
from bdd_amd.solver import bdd_hip_batch, bdd_hip_lbfgs, bdd_hip_parallel_mma  # noqa: E402
from grad_counts_fixtures import IDLE, row  # noqa: E402
from grad_small_fixtures import MIXED, exact_reference, instance, model_of, pack_hops  # noqa: E402
from test_gpu_grad_small import GRADS, assert_state, fused, names_of, refused, sequential, split, state, to_public  # noqa: E402
from test_gpu_small_learned import AUTOGRAD_MEMBERS, _assert_tiered, dirichlet_weights  # noqa: E402
from test_gpu_small_learned import instance as learned_instance  # noqa: E402

# per member, cycled: at least three values of each, a member that tracks nothing, one without untracked iterations in front of tracked ones
AFTERS = [0, 5, 2, 1, 7, 3, 0, 4]
TRACKS = [3, 1, 5, 0, 2, 4, 1, 2]


def counts_of(k):
    a, t = [AFTERS[i % len(AFTERS)] for i in range(k)], [TRACKS[i % len(TRACKS)] for i in range(k)]
    assert len(set(a)) >= 3 and len(set(t)) >= 3 and 0 in t and any(x == 0 and y > 0 for x, y in zip(a, t))
    return a, t


# ---------------------------------------------------------------- 1. exact fixtures against the restatement
@pytest.mark.parametrize("omega_vec", [False, True], ids=["omega", "omega_vec"])
@pytest.mark.parametrize("precision", ["float", "double"])
def test_exact_fixtures_with_their_own_counts_equal_the_restatement_bit_for_bit(precision, omega_vec):
    names = names_of(precision)
    assert MIXED in names and "assign9" in names and ("cover200x300" in names) == (precision == "float")
    hops = pack_hops(instance(MIXED)[0])
    assert hops.count(3) >= 2 and hops.count(9) >= 2, hops   # waves of one workgroup with sweeps of different lengths
    rows = [row(n, omega_vec) for n in names]
    names, rows = names + [IDLE[0]], rows + [(IDLE[1], IDLE[2], row(IDLE[0], omega_vec)[2])]   # the member that tracks nothing, last
    idle = len(names) - 1
    members = [fused(n, precision) for n in names]
    dt = members[0].value_type
    batch = bdd_hip_batch(members)
    refs, perms, pubs = [], [], []
    for n, (untracked, tracked, seed), s in zip(names, rows, members):
        # (the idle member: the inputs of its shape's row, which depend on the seed alone; its reference is not looked at)
        ref = exact_reference(n, seed, omega_vec, *(row(n, omega_vec)[:2] if tracked == 0 else (untracked, tracked)))
        perm = s.bdd_major_order()
        np.testing.assert_array_equal(model_of(n).layer_var, s.get_primal_variable_index()[perm])
        pub = {k: to_public(v, perm, dt) for k, v in ref["x"].items() if isinstance(v, np.ndarray)}
        s.set_solver_costs(pub["lo"], pub["hi"], np.zeros(s.nr_layers(), dt))
        refs.append(ref), perms.append(perm), pubs.append(pub)
    cat = lambda k: np.concatenate([p[k] for p in pubs])
    omega = dict(omega_vec=cat("omega_vec")) if omega_vec else dict(omega=1.0)
    before = [state(s) for s in members]
    for call in range(2):
        got = batch.grad_iterations_counts(cat("alpha"), cat("g_lo"), cat("g_hi"), cat("g_mm"), [r[0] for r in rows], [r[1] for r in rows],
                                           num_caches=1 + call, **omega)
        for i, (n, s, ref, perm, mine, b) in enumerate(zip(names, members, refs, perms, split(got, members, not omega_vec), before)):
            what = f"{n} {precision} {'omega_vec' if omega_vec else 'omega'} {rows[i][0]}+{rows[i][1]}, call {call}"
            if i == idle:   # in-out parts unchanged, outputs zero
                for g, k in zip(mine[:3], ("g_lo", "g_hi", "g_mm")):
                    np.testing.assert_array_equal(g, pubs[i][k], err_msg=f"{what}: {k}")
                assert not mine[3].any() and not mine[4].any() and mine[4].size == (s.nr_layers() if omega_vec else 1), what
            else:
                for g, want, nm in zip(mine, ref["grads"], GRADS):
                    assert g.dtype == dt
                    if nm == "grad_omega" and not omega_vec:   # the scalar: the per-layer values summed in double (exact)
                        want = np.array([want.astype(np.float64).sum()])
                    else:
                        g = g[perm]
                    np.testing.assert_array_equal(g, np.asarray(want).astype(dt), err_msg=f"{what}: {nm}")
            assert_state(s, b, what)   # (the idle member: lower_bound() is the value read before the call)
    batch.close()


# ---------------------------------------------------------------- 2. a batch against its members driven alone
@pytest.mark.parametrize("omega_vec", [False, True], ids=["omega", "omega_vec"])
@pytest.mark.parametrize("precision", ["float", "double"])
def test_batch_with_counts_equals_each_member_on_the_four_launch_path(precision, omega_vec, monkeypatch):
    names = names_of(precision)
    members = [fused(n, precision) for n in names]
    twins = [sequential(n, precision) for n in names]
    afters, tracks = counts_of(len(names))
    dt = members[0].value_type
    rng = np.random.default_rng(41 + omega_vec)
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
        want.append(q.grad_iterations(x["w"][i], x["g_lo"][i], x["g_hi"][i], x["g_mm"][i], track_grad_after_itr=afters[i], track_grad_for_num_itr=tracks[i],
                                      num_caches=1, **om))
    before = [state(s) for s in members]
    batch = bdd_hip_batch(members)
    cat = lambda k: np.concatenate(x[k])
    om = dict(omega_vec=cat("ov")) if omega_vec else dict(omega=0.5)
    got = batch.grad_iterations_counts(cat("w"), cat("g_lo"), cat("g_hi"), cat("g_mm"), afters, tracks, num_caches=1, **om)
    again = batch.grad_iterations_counts(cat("w"), cat("g_lo"), cat("g_hi"), cat("g_mm"), afters, tracks, num_caches=3, **om)
    for a, b, nm in zip(got, again, GRADS):
        np.testing.assert_array_equal(a, b, err_msg=f"second call, num_caches 3: {nm}")
    for i, (name, s, mine) in enumerate(zip(names, members, split(got, members, not omega_vec))):
        what = f"{name} {precision} {'omega_vec' if omega_vec else 'omega'} {afters[i]}+{tracks[i]}"
        if precision == "float" or name.startswith("assign") or tracks[i] == 0:
            for g, w, nm in zip(mine, want[i], GRADS):
                np.testing.assert_array_equal(g, w, err_msg=f"{what}: {nm}")
        else:
            assert s.get_num_bdds_per_var().max() > 2
            monkeypatch.setattr(tg, "AFTER", afters[i])   # _double_allowance's counts: this member's
            monkeypatch.setattr(tg, "TRACK", tracks[i])
            tols, devs, perm = tg._double_allowance(name, s, x, i, omega_vec)
            for g, w, tol, dev, nm in zip(mine, want[i], tols, devs, GRADS):
                per_layer = g.size == s.nr_layers()
                err = np.abs(np.asarray(g, np.longdouble) - np.asarray(w, np.longdouble)).astype(np.float64)
                err = err[perm] if per_layer else err
                print(f"{what} {nm}: restatement double vs long double {dev:.3e}; batch vs four-launch twin {err.max():.3e}; allowed (min over entries) "
                      f"{tol.min():.3e}; largest |value| {float(np.abs(w).max()):.3e}")
                assert np.all(err <= tol), (what, nm, float(err.max()), float(tol.min()))
        assert_state(s, before[i], what)
    batch.close()


# ---------------------------------------------------------------- 3. equal counts
@pytest.mark.parametrize("precision", ["float", "double"])
def test_equal_counts_are_the_call_with_one_count(precision):
    names = names_of(precision)
    sets = [[fused(n, precision, 2) for n in names] for _ in range(2)]
    rng = np.random.default_rng(43)
    w = [dirichlet_weights(s, rng) for s in sets[0]]
    dt = sets[0][0].value_type
    n = sum(s.nr_layers() for s in sets[0])
    g = [rng.normal(0, 1, n).astype(dt) for _ in range(3)]
    ov = rng.uniform(0.1, 0.9, n).astype(dt)
    for ms in sets:
        for s in ms:
            s.iterations(2)
    batches = [bdd_hip_batch(ms) for ms in sets]
    K = len(names)
    for a, t, om in ((2, 3, dict(omega=0.4)), (0, 2, dict(omega_vec=ov)), (3, 0, dict(omega=0.4))):
        mine = batches[0].grad_iterations_counts(np.concatenate(w), *g, [a] * K, [t] * K, **om)
        want = batches[1].grad_iterations(np.concatenate(w), *g, track_grad_after_itr=a, track_grad_for_num_itr=t, **om)
        for x, y, nm in zip(mine, want, GRADS):
            np.testing.assert_array_equal(x, y, err_msg=f"{a}+{t}: {nm}")
    for s, t, wi, name in zip(sets[0], sets[1], w, names):
        assert s.learned_iterations(wi, 2, 0.5, improvement_slope=0.0) == 2 and t.learned_iterations(wi, 2, 0.5, improvement_slope=0.0) == 2
        assert_state(s, state(t), f"{name}: learned_iterations behind the calls")
    for b in batches:
        b.close()


# ---------------------------------------------------------------- 4. state contract and ordering with device arrays
@pytest.mark.parametrize("precision", ["float", "double"])
def test_member_calls_right_behind_the_call_with_device_arrays(precision):
    import torch
    names = names_of(precision)
    members = [fused(n, precision, 2) for n in names]
    twins = [fused(n, precision, 2) for n in names]
    afters, tracks = counts_of(len(names))
    rng = np.random.default_rng(44)
    w = [dirichlet_weights(s, rng) for s in members]
    for i, (s, t) in enumerate(zip(members, twins)):   # deferred differences and a delta; every second member's costs updated since (stale sweeps)
        for u in (s, t):
            u.iterations(2)
        if i % 2:
            d = rng.uniform(-0.5, 0.5, size=s.nr_variables())
            s.update_costs([], d)
            t.update_costs([], d)
    dt = members[0].value_type
    g = [[rng.normal(0, 1, s.nr_layers()).astype(dt) for s in members] for _ in range(3)]
    put = lambda a: torch.tensor(np.concatenate(a), device="cuda")
    t_g = [put(a) for a in g]
    n = t_g[0].numel()
    out = (torch.empty(n, dtype=t_g[0].dtype, device="cuda"), torch.empty(len(members), dtype=t_g[0].dtype, device="cuda"))
    batch = bdd_hip_batch(members)
    res = batch.grad_iterations_counts(put(w), *t_g, afters, tracks, omega=0.4, out=out)
    assert res[0] is t_g[0] and res[3] is out[0]
    bounds = []
    for i, s in enumerate(members):   # right behind it, without the host having waited
        if i % 3 == 0:
            bounds.append(s.lower_bound())
        s.iterations(2)
    torch.cuda.synchronize()
    res = [r.cpu().numpy() for r in res]
    want, twin_bounds = [], []
    for i, t in enumerate(twins):     # the per-member path: the member's own call, then the same calls
        want.append(t.grad_iterations(w[i], g[0][i], g[1][i], g[2][i], omega=0.4, track_grad_after_itr=afters[i], track_grad_for_num_itr=tracks[i]))
        if i % 3 == 0:
            twin_bounds.append(t.lower_bound())
        t.iterations(2)
    assert bounds == twin_bounds
    for i, (s, t, mine, name) in enumerate(zip(members, twins, split(res, members, True), names)):
        for x, y, nm in zip(mine, want[i], GRADS):   # the same fused forward, the same reverse arithmetic
            if precision == "float" or name.startswith("assign") or tracks[i] == 0:
                np.testing.assert_array_equal(x, y, err_msg=f"{name}: {nm}")
        assert_state(s, state(t), f"{name}: iterations behind the batch call")
    batch.close()


# ---------------------------------------------------------------- 5. refusals
def test_refusals_leave_every_member_and_every_output_untouched():
    names = ("assign8", "cover40x60", "cover67x100", "assign3")
    members = [fused(n, "float") for n in names]
    batch = bdd_hip_batch(members)
    rng = np.random.default_rng(45)
    w = [dirichlet_weights(s, rng) for s in members]
    ov = [rng.uniform(0.1, 0.9, s.nr_layers()).astype(np.float32) for s in members]
    g = [[rng.normal(0, 1, s.nr_layers()).astype(np.float32) for s in members] for _ in range(3)]
    cat = np.concatenate
    batch.learned_iterations(cat(w), 2)
    before = [state(s) for s in members]
    n = sum(s.nr_layers() for s in members)
    FILL = np.float32(7.0)

    def raw(w_=w, g_=g, ov_=None, after=(1, 0, 2, 1), tracked=(2, 1, 0, 3)):
        """through capi, with outputs the test owns: (rc, message, the five arrays afterwards, the three in-out ones as given)"""
        arr = [cat(w_)] + [cat(a).copy() for a in g_] + [np.full(n, FILL), np.full(n if ov_ is not None else len(members), FILL)]
        o = cat(ov_) if ov_ is not None else None
        mk = lambda c: None if c is None else (C.c_uint64 * len(c))(*c)
        rc = batch._L.bddmma_grad_learned_iterations_counts_batch(batch._h, arr[0].ctypes.data, None if o is None else o.ctypes.data, 0.5,
                                                                  *(a.ctypes.data for a in arr[1:]), mk(after), mk(tracked), 1, 0)
        return rc, batch._L.bddmma_batch_last_error(batch._h).decode(), arr[1:], [cat(a) for a in g_]

    def untouched(res, rc):
        code, msg, arrays, given = res
        assert code == rc, (code, msg)
        for a, b in zip(arrays[:3], given):
            np.testing.assert_array_equal(a, b)
        assert np.all(arrays[3] == FILL) and np.all(arrays[4] == FILL)
        for s, b, name in zip(members, before, names):
            assert_state(s, b, name)
        return msg

    assert "count" in untouched(raw(after=None), capi.ERR_INVALID_ARGUMENT)
    assert "count" in untouched(raw(tracked=None), capi.ERR_INVALID_ARGUMENT)
    msg = untouched(raw(tracked=(2, 1, 2 ** 32, 2 ** 32)), capi.ERR_INVALID_ARGUMENT)
    assert "member 2" in msg and "tracked" in msg
    bad_w = [a.copy() for a in w]
    bad_w[2][3] = np.nan
    msg = untouched(raw(w_=bad_w), capi.ERR_INVALID_ARGUMENT)   # member 2 tracks nothing: its arguments are checked all the same
    assert "member 2" in msg and "dist_weights" in msg
    bad_ov = [a.copy() for a in ov]
    bad_ov[1][0] = -0.25
    msg = untouched(raw(ov_=bad_ov), capi.ERR_INVALID_ARGUMENT)
    assert "member 1" in msg and "omega_vec" in msg
    bad_g = [[a.copy() for a in arr] for arr in g]
    bad_g[1][3][5] = np.inf
    msg = untouched(raw(g_=bad_g), capi.ERR_INVALID_ARGUMENT)
    assert "member 3" in msg and "grad_hi" in msg
    # through the Python class as well
    msg = refused(capi.ERR_INVALID_ARGUMENT, lambda: batch.grad_iterations_counts(cat(w), cat(g[0]), cat(g[1]), cat(g[2]), [1, 0, 2, 1], [2, 2 ** 32, 0, 3]))
    assert "member 1" in msg
    wrapper = bdd_hip_lbfgs(members[3])
    msg = untouched(raw(), capi.ERR_STATE)
    assert "member 3" in msg and "L-BFGS" in msg
    wrapper.close()
    batch.close()


def test_a_member_that_is_not_learned_fusable_is_refused_with_counts():
    """cover160x240 in double: fused_small, not fused_small_learned (tests/test_gpu_small_learned.py)"""
    a = fused("assign8", "double")
    b = bdd_hip_parallel_mma(*learned_instance("cover160x240", 0), precision="double")
    assert b.nr_packs() == 8 and b.fused_small() and not b.fused_small_learned()
    batch = bdd_hip_batch([a, b])
    batch.iterations(2)
    before = [state(s) for s in (a, b)]
    rng = np.random.default_rng(46)
    n = a.nr_layers() + b.nr_layers()
    w = np.concatenate([dirichlet_weights(s, rng) for s in (a, b)])
    g = [rng.normal(0, 1, n) for _ in range(3)]
    msg = refused(capi.ERR_UNSUPPORTED, lambda: batch.grad_iterations_counts(w, *g, [1, 0], [2, 0]))
    assert "member 1" in msg and "fused_small_learned" in msg
    for s, bf in zip((a, b), before):
        assert_state(s, bf)
    batch.close()


# ---------------------------------------------------------------- 6. the workspace
def test_workspace_grows_with_the_largest_tracked_count_only():
    names = ("assign8", "cover40x60", "assign3", "cover67x100")
    members = [fused(n, "float") for n in names]
    twins = [fused(n, "float") for n in names]
    batch = bdd_hip_batch(members)
    rng = np.random.default_rng(47)
    w = [dirichlet_weights(s, rng) for s in members]
    g = [[rng.normal(0, 1, s.nr_layers()).astype(np.float32) for s in members] for _ in range(3)]
    cat = np.concatenate
    calls = [([2, 0, 1, 3], [1, 1, 0, 1]), ([1, 2, 0, 0], [2, 6, 1, 3]), (0, 3), ([0, 1, 2, 3], [6, 0, 4, 5])]
    used = []
    for after, tracked in calls:
        if isinstance(after, int):
            got = batch.grad_iterations(cat(w), cat(g[0]), cat(g[1]), cat(g[2]), track_grad_after_itr=after, track_grad_for_num_itr=tracked)
            after, tracked = [after] * len(members), [tracked] * len(members)
        else:
            got = batch.grad_iterations_counts(cat(w), cat(g[0]), cat(g[1]), cat(g[2]), after, tracked)
        used.append(sum(s.device_bytes() for s in members))
        for i, (t, mine, name) in enumerate(zip(twins, split(got, members, True), names)):
            want = t.grad_iterations(w[i], g[0][i], g[1][i], g[2][i], track_grad_after_itr=after[i], track_grad_for_num_itr=tracked[i])
            for x, y, nm in zip(mine, want, GRADS):
                np.testing.assert_array_equal(x, y, err_msg=f"{name} {after[i]}+{tracked[i]}: {nm}")
    assert used[2] == used[1] and used[3] == used[1], used
    batch.close()


# ---------------------------------------------------------------- 7. autograd
@pytest.mark.parametrize("per_layer_omega", [False, True], ids=["omega", "omega_vec"])
@pytest.mark.parametrize("precision", ["float", "double"])
def test_dual_iterations_backward_with_different_counts_is_one_batch_call(precision, per_layer_omega, monkeypatch):
    """100 iterations at most with improvement_slope 1e-2 — the slope and limit of tests/test_gpu_batch_stop.py, at which that file's per-member
    twins of assign3 and assign8 (seed 1, the instances used here) stop after 3 and 14 iterations — of which 3 are tracked: the batch's
    backward is one grad_iterations_counts and nothing else; gradients against the list form's, tiered as
    tests/test_gpu_small_learned.py::_assert_tiered"""
    import torch
    from bdd_amd.autograd import DualIterations
    calls = {"counts": 0, "batch": 0, "solver": 0}

    def count(cls, name, key):
        inner = getattr(cls, name)

        def counted(*a, **kw):
            r = inner(*a, **kw)
            calls[key] += 1
            return r
        monkeypatch.setattr(cls, name, counted)

    count(bdd_hip_batch, "grad_iterations_counts", "counts")
    count(bdd_hip_batch, "grad_iterations", "batch")
    count(bdd_hip_parallel_mma, "grad_iterations", "solver")
    tdt = torch.float64 if precision == "double" else torch.float32
    a = [fused(n, precision) for n in AUTOGRAD_MEMBERS]
    b = [fused(n, precision) for n in AUTOGRAD_MEMBERS]
    assert all(s.fused_small_stop() for s in a + b)
    batch = bdd_hip_batch(a)
    dt = a[0].value_type
    rng = np.random.default_rng(48)
    costs = [s.get_solver_costs() for s in a]
    lo, hi = (np.concatenate([c[k] for c in costs]) for k in range(2))
    mm = rng.uniform(-0.25, 0.25, lo.size).astype(dt)
    w = np.concatenate([dirichlet_weights(s, rng) for s in a])
    om = rng.uniform(0.1, 0.9, lo.size).astype(dt) if per_layer_omega else np.asarray([0.5], dt)
    g = [rng.normal(0, 1, lo.size).astype(dt) for _ in range(3)]
    results, seen, done = [], [], []
    for solvers in (batch, list(b)):
        t = [torch.tensor(v, dtype=tdt, device="cuda", requires_grad=True) for v in (lo, hi, mm, w, om)]
        out = DualIterations.apply(solvers, *t[:4], 100, t[4], 3, 1e-2, 1, 0, 0.9)
        done.append([int(d) for d in out[0].grad_fn.iterations_done])
        torch.autograd.backward(out[:3], [torch.tensor(v, dtype=tdt, device="cuda") for v in g])
        torch.cuda.synchronize()
        results.append(([o.detach().cpu().numpy() for o in out if o is not None], [v.grad.cpu().numpy() for v in t]))
        seen.append(dict(calls))
    batch.close()
    print(f"[batch grad counts] DualIterations {precision} {'omega_vec' if per_layer_omega else 'omega'}: counts batch {done[0]} list {done[1]}")
    assert len(set(done[1])) >= 2, done
    assert seen[0] == {"counts": 1, "batch": 0, "solver": 0}, seen
    assert seen[1] == {"counts": 1, "batch": 0, "solver": len(b)}, seen
    for i, n in enumerate(AUTOGRAD_MEMBERS):
        if precision == "float" or n.startswith("assign"):
            assert done[0][i] == done[1][i], (n, done)
    (out_b, grad_b), (out_l, grad_l) = results
    assert all(np.any(v != 0) for v in grad_b)
    if done[0] == done[1]:
        off = np.cumsum([0] + [s.nr_layers() for s in a])
        _assert_tiered(out_b, out_l, off, precision)
        _assert_tiered(grad_b, grad_l, off, precision)
