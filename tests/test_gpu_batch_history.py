"""A batch's learned iterations with their history inside the members' workgroups (include/bdd_mma.h: bddmma_learned_iterations_history_batch,
bddmma_fused_small_history; kernels/small.hpp: the HISTORY form of small_iterate; kernels/smallhist.hpp: k_learned_small_hist_batch) on the
MI355X.

The reference of the batch comparisons is a second handle per member driven alone through learned_iterations with the same arguments (its
tracked iterations run the four launches, FWD_SOLUTION and the elementwise history kernels); one test compares with the NumPy restatement
instead, which shares no code with the library.  Tolerances: bit-equal in float and on assign* in double; ISO_TOL (1e-12, tier 1) on
cover* in double, where the two exchanges add a variable's terms in different orders — with cost seeds whose arg-min decisions have a
margin three orders above that (tests/batch_history_fixtures.py; tests/test_batch_history_fixtures.py asserts it without a GPU).

Every case asserts fused_small_history() and the pack count first."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from batch_history_fixtures import BETA, HISTORIES, NUM_ITR, OMEGA, LearnedMmaOv, major_inputs, member_keys  # noqa: E402
from bdd_amd import capi  # noqa: E402
from bdd_amd.solver import bdd_hip_batch, bdd_hip_parallel_mma  # noqa: E402
from test_gpu_small_learned import (AUTOGRAD_MEMBERS, ISO_TOL, REF_TOL, SHAPES, _assert_tiered, assert_same, dirichlet_weights, instance, refused,  # noqa: E402
                                    state)

FILL = 7.0


def member(name, packs, seed, precision):
    """a solver and its twin, and the member's inputs in the public layer order"""
    col, costs = instance(name, seed)
    s, t = (bdd_hip_parallel_mma(col, costs, precision=precision) for _ in range(2))
    assert s.nr_packs() == packs, (name, s.nr_packs())
    assert s.fused_small() and s.fused_small_learned() and s.fused_small_history() and t.fused_small_history(), name
    perm = s.bdd_major_order()
    wm, ovm = major_inputs(s.get_primal_variable_index()[perm], name, seed, s.value_type)
    w, ov = np.empty_like(wm), np.empty_like(ovm)
    w[perm], ov[perm] = wm, ovm
    return dict(name=name, seed=seed, s=s, t=t, w=w, ov=ov, perm=perm, col=col, costs=costs)


def members(precision, keys=None):
    return [member(name, packs, seed, precision) for name, packs, seed in (keys if keys is not None else member_keys(precision, SHAPES))]


def filled(ms):
    vt = ms[0]["s"].value_type
    return [np.full(sum(m["s"].nr_layers() for m in ms), FILL, vt), np.full(sum(m["s"].nr_bdds() for m in ms), FILL, vt),
            np.full(sum(m["s"].nr_bdds() for m in ms), FILL, vt)]


def batch_call(batch, ms, outs, history, with_ov, device, num_itr=NUM_ITR):
    """the batch call on host arrays or device tensors; returns the three outputs as NumPy arrays"""
    w = np.concatenate([m["w"] for m in ms])
    ov = np.concatenate([m["ov"] for m in ms]) if with_ov else None
    names = ("sol_avg", "lb_first_diff_avg", "lb_second_diff_avg")
    if not device:
        batch.learned_iterations_history(w, num_itr, omega=OMEGA, omega_vec=ov, compute_history_for_itr=history, history_avg_beta=BETA, **dict(zip(names, outs)))
        return outs
    import torch
    dev = [torch.tensor(x, device="cuda") for x in outs]
    batch.learned_iterations_history(torch.tensor(w, device="cuda"), num_itr, omega=OMEGA, omega_vec=None if ov is None else torch.tensor(ov, device="cuda"),
                                     compute_history_for_itr=history, history_avg_beta=BETA, **dict(zip(names, dev)))
    batch.stream_signal(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return [x.cpu().numpy() for x in dev]


def twin_call(m, history, with_ov, num_itr=NUM_ITR):
    t = m["t"]
    o = [np.full(t.nr_layers(), FILL, t.value_type), np.full(t.nr_bdds(), FILL, t.value_type), np.full(t.nr_bdds(), FILL, t.value_type)]
    args = dict(omega_vec=m["ov"]) if with_ov else dict(omega=OMEGA)
    assert t.learned_iterations(m["w"], num_itr, improvement_slope=0.0, sol_avg=o[0], lb_first_diff_avg=o[1], lb_second_diff_avg=o[2],
                                compute_history_for_itr=history, history_avg_beta=BETA, **args) == num_itr
    return o


def split(ms, outs):
    """the batch's outputs per member"""
    L = np.cumsum([0] + [m["s"].nr_layers() for m in ms])
    B = np.cumsum([0] + [m["s"].nr_bdds() for m in ms])
    return [[outs[0][L[i]:L[i + 1]], outs[1][B[i]:B[i + 1]], outs[2][B[i]:B[i + 1]]] for i in range(len(ms))]


def assert_history(got, want, rel, what):
    for x, y, nm in zip(got, want, ("sol_avg", "lb_first_diff_avg", "lb_second_diff_avg")):
        if rel == 0:
            np.testing.assert_array_equal(x, y, err_msg=f"{what} {nm}")
        else:
            y64 = np.asarray(y, np.float64)
            np.testing.assert_allclose(np.asarray(x, np.float64), y64, rtol=rel, atol=rel * max(1.0, float(np.abs(y64).max())), err_msg=f"{what} {nm}")


def assert_reach(o, history, what):
    """an entry the history does not reach keeps its content: one tracked iteration writes sol_avg only, two also the first differences"""
    assert not np.any(o[0] == FILL), what
    assert np.all(o[1] == FILL) == (history < 2), what
    assert np.all(o[2] == FILL) == (history < 3), what


def tol(m, precision):
    return 0 if precision == "float" or m["name"].startswith("assign") else ISO_TOL[precision]


# ---------------------------------------------------------------- 1. the batch against its members driven alone
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("precision", ["float", "double"])
def test_batch_history_equals_each_member_driven_alone(precision, device):
    ms = members(precision)
    assert len(ms) == (12 if precision == "float" else 10)
    batch = bdd_hip_batch([m["s"] for m in ms])
    start = [m["s"].get_solver_costs() for m in ms]
    for with_ov in (False, True):
        for history in HISTORIES:
            for m, c in zip(ms, start):   # every case runs the ten iterations whose decision margins the CPU test asserts
                m["s"].set_solver_costs(*c)
                m["t"].set_solver_costs(*c)
            outs = batch_call(batch, ms, filled(ms), history, with_ov, device)
            for m, o in zip(ms, split(ms, outs)):
                what = f"{m['name']} seed {m['seed']} {precision}: history {history}, omega_vec {with_ov}"
                ref = twin_call(m, history, with_ov)
                assert_same(m["s"], m["t"], tol(m, precision), what)
                assert_history(o, ref, tol(m, precision), what)
                assert_reach(o, history, what)
    batch.close()


# ---------------------------------------------------------------- 2. against the restatement
@pytest.mark.parametrize("with_ov,history", [(False, 10), (True, 3)], ids=["omega-all", "omega_vec-3"])
@pytest.mark.parametrize("name,packs", [("assign8", 1), ("cover40x60", 2), ("cover67x100", 4)])
def test_batch_history_of_one_member_vs_restatement(name, packs, with_ov, history):
    m = member(name, packs, 1, "double")
    s, perm = m["s"], m["perm"]
    r = LearnedMmaOv(m["col"].instr, m["col"].delims, "double")
    r.update_costs_hi(np.asarray(m["costs"], np.float64))
    np.testing.assert_array_equal(r.layer_var, s.get_primal_variable_index()[perm])
    batch = bdd_hip_batch([s])
    rel = REF_TOL["double"]
    outs = batch_call(batch, [m], filled([m]), history, with_ov, False)
    batch.close()
    want = [np.full(s.nr_layers(), FILL), np.full(s.nr_bdds(), FILL), np.full(s.nr_bdds(), FILL)]
    assert r.iterations(m["w"][perm], NUM_ITR, m["ov"][perm] if with_ov else OMEGA, improvement_slope=0.0, sol_avg=want[0], lb_first_diff_avg=want[1],
                        lb_second_diff_avg=want[2], compute_history_for_itr=history, history_avg_beta=BETA) == NUM_ITR
    lb_scale = max(1.0, float(np.abs(r.lower_bound_per_bdd()).max()))
    np.testing.assert_allclose(outs[0][perm], want[0], rtol=rel, atol=rel, err_msg="sol_avg")
    # differences of per-BDD bounds: their error is the bounds' (tests/test_gpu_learned_mma.py)
    np.testing.assert_allclose(outs[1], want[1], rtol=rel, atol=4 * rel * lb_scale, err_msg="lb_first_diff_avg")
    np.testing.assert_allclose(outs[2], want[2], rtol=rel, atol=8 * rel * lb_scale, err_msg="lb_second_diff_avg")
    lo, hi, mm = s.get_solver_costs()
    for x, y, nm in ((lo[perm], r.lo, "lo"), (hi[perm], r.hi, "hi"), (mm[perm], r.mm, "deferred mm")):
        np.testing.assert_allclose(x, y, rtol=rel, atol=rel * max(1.0, float(np.abs(y).max())), err_msg=nm)


# ---------------------------------------------------------------- 3. state across launches
@pytest.mark.parametrize("precision", ["float", "double"])
def test_history_with_the_first_iteration_in_a_launch_of_its_own(precision):
    """A fresh batch runs the first iteration as a launch of its own (the members' initial bound change is unset), so the history crosses a
    launch; a batch whose members have run a learned call before does not split.  The same state and inputs give the same history — and a
    second call starts its history afresh."""
    keys = [("assign8", 1, 1), ("cover67x100", 4, 1)]
    fresh, warm = members(precision, keys), members(precision, keys)
    for m in warm:      # one learned call, then the fresh members' state again
        lo, hi, mm = m["s"].get_solver_costs()
        m["s"].learned_iterations(m["w"], 1, OMEGA, improvement_slope=0.0)
        m["s"].set_solver_costs(lo, hi, mm)
    b_fresh, b_warm = bdd_hip_batch([m["s"] for m in fresh]), bdd_hip_batch([m["s"] for m in warm])
    for call in range(2):
        o_fresh = batch_call(b_fresh, fresh, filled(fresh), 3, False, False, num_itr=3)
        o_warm = batch_call(b_warm, warm, filled(warm), 3, False, False, num_itr=3)
        for a, b, of, ow in zip(fresh, warm, split(fresh, o_fresh), split(warm, o_warm)):
            what = f"{a['name']} {precision} call {call}"
            assert_same(a["s"], b["s"], tol(a, precision), what)
            assert_history(of, ow, tol(a, precision), what)
            assert_reach(of, 3, what)
            # two calls in a row: each starts at tracked = 0 — the twin, called twice as well, sees the same
            assert_history(of, twin_call(a, 3, False, num_itr=3), tol(a, precision), what + " (twin)")
    b_fresh.close()
    b_warm.close()


# ---------------------------------------------------------------- 4. a mix of wave counts, and a batch of one
def test_a_mix_of_wave_counts_in_interleaved_order():
    keys = [("cover200x300", 10, 1), ("assign8", 1, 1), ("cover147x220", 7, 1), ("cover40x60", 2, 1), ("cover67x100", 4, 1), ("assign3", 1, 2),
            ("cover200x300", 10, 2), ("cover40x60", 2, 2)]
    ms = members("float", keys)
    batch = bdd_hip_batch([m["s"] for m in ms])
    outs = batch_call(batch, ms, filled(ms), 4, True, False, num_itr=6)
    for m, o in zip(ms, split(ms, outs)):
        what = f"{m['name']} seed {m['seed']}"
        assert_history(o, twin_call(m, 4, True, num_itr=6), 0, what)
        assert_same(m["s"], m["t"], 0, what)
    batch.close()


@pytest.mark.parametrize("precision", ["float", "double"])
def test_history_batch_of_one_member(precision):
    m = member("cover147x220", 7, 2, precision)
    batch = bdd_hip_batch([m["s"]])
    outs = batch_call(batch, [m], filled([m]), 10, False, True)
    assert_history(outs, twin_call(m, 10, False), tol(m, precision), "one member")
    assert_same(m["s"], m["t"], tol(m, precision))
    batch.close()


# ---------------------------------------------------------------- 5. refusals
def test_history_refusals_leave_members_and_outputs_unchanged():
    ms = members("float", [("assign8", 1, 1), ("cover40x60", 2, 1), ("cover67x100", 4, 1)])
    batch = bdd_hip_batch([m["s"] for m in ms])
    outs = batch_call(batch, ms, filled(ms), 2, False, False, num_itr=2)
    before = [state(m["s"]) for m in ms]
    kept = [x.copy() for x in outs]
    w = np.concatenate([m["w"] for m in ms])

    def unchanged():
        for m, b in zip(ms, before):
            for x, y in zip(state(m["s"]), b):
                np.testing.assert_array_equal(x, y)
        for x, y in zip(outs, kept):
            np.testing.assert_array_equal(x, y)

    # a null history array
    msg = refused(capi.ERR_INVALID_ARGUMENT, lambda: batch.learned_iterations_history(w, 3, compute_history_for_itr=2, history_avg_beta=BETA, sol_avg=outs[0],
                                                                               lb_first_diff_avg=None, lb_second_diff_avg=outs[2]))
    assert "lb_first_diff_avg" in msg
    unchanged()
    # a negative weight with a history requested
    bad = w.copy()
    bad[ms[0]["s"].nr_layers() + 3] = -0.5
    msg = refused(capi.ERR_INVALID_ARGUMENT, lambda: batch.learned_iterations_history(bad, 3, compute_history_for_itr=2, history_avg_beta=BETA, sol_avg=outs[0],
                                                                               lb_first_diff_avg=outs[1], lb_second_diff_avg=outs[2]))
    assert "member 1" in msg and "dist_weights" in msg
    unchanged()
    batch.close()


def test_a_member_without_the_history_form_is_refused():
    """cover160x240 in double is fused_small and not fused_small_learned (tests/test_gpu_small_learned.py), hence not fused_small_history;
    no shape of the suite has the learned form without the history form, which needs no LDS of its own"""
    a = member("assign8", 1, 1, "double")
    b = bdd_hip_parallel_mma(*instance("cover160x240", 0), precision="double")
    assert b.nr_packs() == 8 and b.fused_small() and not b.fused_small_history() and a["s"].fused_small_history()
    batch = bdd_hip_batch([a["s"], b])
    before = [state(s) for s in (a["s"], b)]
    w = np.concatenate([a["w"], dirichlet_weights(b, np.random.default_rng(41))])
    outs = [np.full(a["s"].nr_layers() + b.nr_layers(), FILL), np.full(a["s"].nr_bdds() + b.nr_bdds(), FILL), np.full(a["s"].nr_bdds() + b.nr_bdds(), FILL)]
    msg = refused(capi.ERR_UNSUPPORTED, lambda: batch.learned_iterations_history(w, 3, compute_history_for_itr=3, history_avg_beta=BETA, sol_avg=outs[0],
                                                                          lb_first_diff_avg=outs[1], lb_second_diff_avg=outs[2]))
    assert "member 1" in msg and "fused_small_history" in msg
    for s, bf in zip((a["s"], b), before):
        for x, y in zip(state(s), bf):
            np.testing.assert_array_equal(x, y)
    assert all(np.all(x == FILL) for x in outs)
    batch.close()


# ---------------------------------------------------------------- 6. DualIterations
@pytest.mark.parametrize("history", [3, 5])
@pytest.mark.parametrize("precision", ["float", "double"])
def test_dual_iterations_with_a_history_take_the_batched_branch(precision, history, monkeypatch):
    """_autograd_case of tests/test_gpu_small_learned.py (5 iterations) with the members' learned_iterations counted: the batch form makes
    three batch calls and none on a member"""
    import torch
    from bdd_amd.autograd import DualIterations
    tdt = torch.float64 if precision == "double" else torch.float32
    a = [bdd_hip_parallel_mma(*instance(n, 1), precision=precision) for n in AUTOGRAD_MEMBERS]
    b = [bdd_hip_parallel_mma(*instance(n, 1), precision=precision) for n in AUTOGRAD_MEMBERS]
    assert all(s.fused_small_learned() and s.fused_small_history() for s in a + b)
    calls = {"batch": 0, "list": 0}
    for group, solvers in (("batch", a), ("list", b)):
        for s in solvers:
            def counted(*args, _inner=s.learned_iterations, _group=group, **kw):
                calls[_group] += 1
                return _inner(*args, **kw)
            monkeypatch.setattr(s, "learned_iterations", counted)
    batch = bdd_hip_batch(a)
    rng = np.random.default_rng(25)
    costs = [s.get_solver_costs() for s in a]
    lo, hi = (np.concatenate([c[k] for c in costs]) for k in range(2))
    mm = rng.uniform(-0.25, 0.25, lo.size).astype(a[0].value_type)
    w = np.concatenate([dirichlet_weights(s, rng) for s in a])
    om = np.asarray([0.5], a[0].value_type)
    g = [rng.normal(0, 1, lo.size).astype(a[0].value_type) for _ in range(3)]
    results = []
    for solvers in (batch, list(b)):
        t = [torch.tensor(x, dtype=tdt, device="cuda", requires_grad=True) for x in (lo, hi, mm, w, om)]
        out = DualIterations.apply(solvers, *t[:4], 5, t[4], 3, 0.0, 1, history, 0.9)
        torch.autograd.backward(out[:3], [torch.tensor(x, dtype=tdt, device="cuda") for x in g])
        torch.cuda.synchronize()
        results.append(([o.detach().cpu().numpy() for o in out], [x.grad.cpu().numpy() for x in t]))
    batch.close()
    assert calls == {"batch": 0, "list": len(b)}, calls
    (out_b, grad_b), (out_l, grad_l) = results
    assert len(out_b) == len(out_l) == 6
    off = np.cumsum([0] + [s.nr_layers() for s in a])
    _assert_tiered(out_b, out_l, off, precision)
    _assert_tiered(grad_b, grad_l, off, precision)
