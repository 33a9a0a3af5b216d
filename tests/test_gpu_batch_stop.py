"""A batch's learned iterations that stop on the bound's slope inside the members' workgroups (include/bdd_mma.h:
bddmma_learned_iterations_stop_batch, bddmma_fused_small_stop; kernels/small.hpp: the STOP form of small_iterate; kernels/smallstop.hpp:
k_learned_small_stop_batch, k_learned_small_hist_stop_batch) on the MI355X.

The yardstick is twins: a second handle per member, given the per-member learned_iterations with the same arguments — its stopping rule
reads the bound on the host after every iteration of four launches.  Compared per member: the count of iterations run, the arc costs and
deferred differences, delta, the three history outputs, lower_bound(), and a further per-member learned call on both handles, whose test
scales with the set-once initial change the first call left.  Bit for bit in float, and in double on the assignment problems (every
variable sits in two BDDs).  The set covers in double are compared at ISO_TOL, and only where the counts agree: there the four-launch
exchange of the twin is itself not reproducible between two handles (tests/test_gpu_small_learned.py,
test_dual_iterations_of_a_batch_fall_back_to_the_list_form), so a borderline test may fall differently.

Members: the generators of the other batch tests (assign3, assign8, cover40x60, cover67x100: 1, 1, 2, 4 packs) and the 12 x 12 assignment
problems of tests/test_gpu_batch_small.py's RUN_MEMBERS (uniform costs and integer costs with near-ties); Dirichlet weights on the
even members and isotropic ones on the odd; a scalar omega and omega_vec.

SLOPE and NUM_ITR were picked from the twins' counts alone (printed by every case; -s shows them).  With 150 iterations allowed, a scalar
omega and no history, the per-member call runs in both precisions
    slope 1e-1: 3, 8, 14, 16, 8, 87, 10, 7, 136, 6          slope 1e-2: 3, 14, 51, 54, 21, 150, 64, 34, 150, 7
    slope 3e-2: 3, 13, 23, 35, 16, 150, 44, 16, 150, 7      slope 1e-3: 3, 15, 150, 150, 150, 150, 93, 51, 150, 7
iterations on the ten members in the order below.  At 1e-2 with 100 iterations the members stop in the first and in the second launch of
the call (32 iterations each) and two run all of them; with omega_vec one stops in the third (94).  See SPREAD below."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from bdd_amd import capi, to_bdd_collection  # noqa: E402
from bdd_amd.instances import assignment_ilp  # noqa: E402
from bdd_amd.solver import bdd_hip_batch, bdd_hip_parallel_mma  # noqa: E402
from learned_mma_restatement import LearnedMma  # noqa: E402
from test_gpu_batch_small import RUN_MEMBERS  # noqa: E402
from test_gpu_small_learned import ISO_TOL, dirichlet_weights, instance, refused, state  # noqa: E402

CHUNK = 32          # iterations per launch of the stopping form (solver_bt.hpp: STOP_CHUNK)
NUM_ITR = 100
SLOPE = 1e-2
BETA = 0.7
OMEGA = 0.5
FILL = 7.0
GENERATED = (("assign3", 1), ("assign8", 1), ("cover40x60", 2), ("cover67x100", 4))
NAMES = ("sol_avg", "lb_first_diff_avg", "lb_second_diff_avg")


def run_instance(kind, seed):
    """tests/test_gpu_batch_small.py: run_members' instances"""
    rng = np.random.default_rng(seed)
    if kind == "uniform":
        costs = rng.uniform(-3.0, 1.0, size=(12, 12))
    else:
        costs = rng.integers(-3, 2, size=(12, 12)).astype(float) + rng.uniform(0, 1e-3, size=(12, 12))
    ilp = assignment_ilp(12, costs)
    return to_bdd_collection(ilp), np.asarray(ilp.objective, np.float64)


def members(precision, keys=None):
    """[dict] per member: the handle s of the batch, its twin t, its weights and omega_vec, and whether it is compared bit for bit"""
    out = []
    rng = np.random.default_rng(57)
    table = [(name, packs, instance(name, 1)) for name, packs in GENERATED] + [(f"assign12-{kind}{seed}", 1, run_instance(kind, seed)) for kind, seed in RUN_MEMBERS]
    for i, (name, packs, (col, costs)) in enumerate(table):
        if keys is not None and name not in keys:
            continue
        s, t = (bdd_hip_parallel_mma(col, costs, precision=precision) for _ in range(2))
        assert s.nr_packs() == packs, (name, s.nr_packs())
        assert s.fused_small_learned() and s.fused_small_history() and s.fused_small_stop() and t.fused_small_stop(), name
        w = dirichlet_weights(s, rng) if i % 2 == 0 else s.get_isotropic_dist_weights()
        ov = rng.uniform(0.1, 0.9, s.nr_layers()).astype(s.value_type)
        out.append(dict(name=name, s=s, t=t, w=w, ov=ov, col=col, costs=costs, exact=precision == "float" or name.startswith("assign")))
    return out


def filled(ms):
    vt = ms[0]["s"].value_type
    nl, nb = sum(m["s"].nr_layers() for m in ms), sum(m["s"].nr_bdds() for m in ms)
    return [np.full(nl, FILL, vt), np.full(nb, FILL, vt), np.full(nb, FILL, vt)]


def batch_call(batch, ms, num_itr, slope, history, with_ov=False, device=False):
    """the batch call on host arrays or device tensors; returns (counts, the three outputs as NumPy arrays or None)"""
    w = np.concatenate([m["w"] for m in ms])
    ov = np.concatenate([m["ov"] for m in ms]) if with_ov else None
    outs = filled(ms) if history else None
    if not device:
        kw = dict(zip(NAMES, outs)) if history else {}
        return batch.learned_iterations_stopping(w, num_itr, omega=OMEGA, improvement_slope=slope, omega_vec=ov, compute_history_for_itr=history,
                                                 history_avg_beta=BETA, **kw), outs
    import torch
    dev = [torch.tensor(x, device="cuda") for x in outs] if history else []
    counts = batch.learned_iterations_stopping(torch.tensor(w, device="cuda"), num_itr, omega=OMEGA, improvement_slope=slope,
                                               omega_vec=None if ov is None else torch.tensor(ov, device="cuda"), compute_history_for_itr=history,
                                               history_avg_beta=BETA, **dict(zip(NAMES, dev)))
    batch.stream_signal(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return counts, ([x.cpu().numpy() for x in dev] if history else None)


def member_call(s, m, num_itr, slope, history, with_ov=False):
    """the per-member call on handle s of member m; returns (count, outputs or None)"""
    o = [np.full(s.nr_layers(), FILL, s.value_type), np.full(s.nr_bdds(), FILL, s.value_type), np.full(s.nr_bdds(), FILL, s.value_type)] if history else None
    kw = dict(zip(NAMES, o)) if history else {}
    args = dict(omega_vec=m["ov"]) if with_ov else dict(omega=OMEGA)
    return s.learned_iterations(m["w"], num_itr, improvement_slope=slope, compute_history_for_itr=history, history_avg_beta=BETA, **args, **kw), o


def split(ms, outs):
    L = np.cumsum([0] + [m["s"].nr_layers() for m in ms])
    B = np.cumsum([0] + [m["s"].nr_bdds() for m in ms])
    return [[outs[0][L[i]:L[i + 1]], outs[1][B[i]:B[i + 1]], outs[2][B[i]:B[i + 1]]] for i in range(len(ms))]


def assert_arrays(got, want, names, exact, precision, what):
    for x, y, nm in zip(got, want, names):
        if exact:
            np.testing.assert_array_equal(x, y, err_msg=f"{what} {nm}")
        else:
            rel, y64 = ISO_TOL[precision], np.asarray(y, np.float64)
            np.testing.assert_allclose(np.asarray(x, np.float64), y64, rtol=rel, atol=rel * max(1.0, float(np.abs(y64).max())), err_msg=f"{what} {nm}")


def compare(ms, counts, outs, num_itr, slope, history, with_ov, precision, label, follow_up=True):
    """every member of the batch against its twin given the per-member call; returns the twins' counts"""
    per_member = split(ms, outs) if history else [None] * len(ms)
    twins = []
    for m, c, o in zip(ms, counts, per_member):
        what = f"{label} {m['name']} {precision}"
        ref_c, ref_o = member_call(m["t"], m, num_itr, slope, history, with_ov)
        twins.append(ref_c)
        if m["exact"]:
            assert c == ref_c, (what, c, ref_c)
        elif c != ref_c:      # a set cover in double whose test fell differently: nothing further to compare
            print(f"[batch stop] {what}: count {c}, twin {ref_c} (not compared)")
            continue
        assert_arrays(state(m["s"]), state(m["t"]), ("lo", "hi", "deferred mm", "delta", "lower bound"), m["exact"], precision, what)
        if history:
            assert_arrays(o, ref_o, NAMES, m["exact"], precision, what)
        if follow_up:   # the next learned call of both handles, per member: its test scales with the initial change the call above has set
            a, _ = member_call(m["s"], m, 40, slope, 0, with_ov)
            b, _ = member_call(m["t"], m, 40, slope, 0, with_ov)
            if m["exact"]:
                assert a == b, (what, "follow-up", a, b)
            if a == b:
                assert_arrays(state(m["s"]), state(m["t"]), ("lo", "hi", "deferred mm", "delta", "lower bound"), m["exact"], precision, what + " follow-up")
    print(f"[batch stop] {label} {precision}: num_itr {num_itr} slope {slope} history {history}: batch {list(counts)} twins {twins}")
    return twins


def launch_of(count):
    """the launch of the call in which a member that ran `count` iterations stopped"""
    return (count - 1) // CHUNK


# ---------------------------------------------------------------- 1. no history: members stop at different counts, in different launches
@pytest.mark.parametrize("with_ov", [False, True], ids=["omega", "omega_vec"])
@pytest.mark.parametrize("precision", ["float", "double"])
def test_members_stop_at_their_own_counts(precision, with_ov):
    ms = members(precision)
    assert len(ms) == 10
    batch = bdd_hip_batch([m["s"] for m in ms])
    counts, _ = batch_call(batch, ms, NUM_ITR, SLOPE, 0, with_ov)
    twins = compare(ms, counts, None, NUM_ITR, SLOPE, 0, with_ov, precision, "stop")
    batch.close()
    if not with_ov:   # SPREAD (of the twins' counts, scalar omega): what makes this case a test of the rule
        stopped = [c for c in twins if c < NUM_ITR]
        assert len({launch_of(c) for c in stopped}) >= 2, twins   # members stop in different launches of the call
        assert NUM_ITR in twins, twins                               # one runs all of them
        assert len(set(twins)) >= 4, twins


# ---------------------------------------------------------------- 2. with a history: convergence before, inside and after the tail window
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("history", [1, 3])
@pytest.mark.parametrize("precision", ["float", "double"])
def test_history_window_opens_at_convergence_or_at_the_tail(precision, history, device):
    ms = members(precision)
    batch = bdd_hip_batch([m["s"] for m in ms])
    counts, outs = batch_call(batch, ms, NUM_ITR, SLOPE, history, False, device)
    twins = compare(ms, counts, outs, NUM_ITR, SLOPE, history, False, precision, f"history {history} {'device' if device else 'host'}")
    batch.close()
    # a member that converges in front of the tail window stops `history` iterations at most behind its count without a history; one that
    # does not converge runs all iterations
    assert any(c < NUM_ITR - history for c in twins) and NUM_ITR in twins, twins
    for m, o in zip(ms, split(ms, outs)):
        assert not np.any(o[0] == FILL), m["name"]                       # every call makes at least one history step
        assert np.all(o[1] == FILL) == (history < 2) and np.all(o[2] == FILL) == (history < 3), m["name"]


@pytest.mark.parametrize("precision", ["float", "double"])
def test_convergence_inside_the_tail_window(precision):
    """num_itr chosen per twin count: with num_itr = c + 1 (c: a member's count without a history) the member converges at its last but one
    iteration, inside the window of the last three — it runs all num_itr, tracking from num_itr - 3 on"""
    keys = ("assign8", "cover40x60", "assign12-uniform8")
    probe_m = members(precision, keys=keys)[0]   # (a handle of its own: the probe sets its initial change)
    probe, _ = member_call(probe_m["t"], probe_m, NUM_ITR, SLOPE, 0)
    assert 3 < probe < NUM_ITR, probe
    ms = members(precision, keys=keys)
    batch = bdd_hip_batch([m["s"] for m in ms])
    counts, outs = batch_call(batch, ms, probe + 1, SLOPE, 3)
    twins = compare(ms, counts, outs, probe + 1, SLOPE, 3, False, precision, "inside the tail")
    batch.close()
    assert twins[0] == probe + 1, (twins, probe)


# ---------------------------------------------------------------- 3. a member whose initial change is already set
@pytest.mark.parametrize("history", [0, 2])
@pytest.mark.parametrize("precision", ["float", "double"])
def test_warm_members_keep_their_initial_change(precision, history):
    """Members that have run a learned call before (their initial change is set, as tests/test_gpu_batch_history.py builds them), brought to
    a state near convergence: the test can fire at iteration 0.  Half of the batch is warm, half fresh."""
    ms = members(precision, keys=("assign3", "assign8", "cover40x60", "assign12-uniform1", "assign12-integer13", "assign12-uniform5"))
    for m in ms[::2]:
        for h in (m["s"], m["t"]):
            assert member_call(h, m, NUM_ITR, 0.0, 0)[0] == NUM_ITR   # sets the initial change at the start and ends near convergence
    batch = bdd_hip_batch([m["s"] for m in ms])
    counts, outs = batch_call(batch, ms, NUM_ITR, SLOPE, history)
    twins = compare(ms, counts, outs, NUM_ITR, SLOPE, history, False, precision, f"warm, history {history}")
    batch.close()
    assert min(twins[::2]) == 1 + history, twins    # a warm member converges at iteration 0 and stops once the history has its steps behind it


# ---------------------------------------------------------------- 4. no iterations; no slope
@pytest.mark.parametrize("precision", ["float", "double"])
def test_zero_iterations_and_zero_slope(precision):
    ms = members(precision, keys=("assign8", "cover67x100", "assign12-integer10"))
    batch = bdd_hip_batch([m["s"] for m in ms])
    before = [state(m["s"]) for m in ms]
    counts, outs = batch_call(batch, ms, 0, SLOPE, 3)
    assert counts == [0, 0, 0] and all(np.all(x == FILL) for x in outs)
    for m, b in zip(ms, before):
        for x, y in zip(state(m["s"]), b):
            np.testing.assert_array_equal(x, y)
    # slope 0 (and a negative one, and NaN) never stops: bddmma_learned_iterations_history_batch, every count num_itr
    for slope in (0.0, -1.0, float("nan")):
        counts, outs = batch_call(batch, ms, 7, slope, 3)
        assert counts == [7, 7, 7], (slope, counts)
        w = np.concatenate([m["w"] for m in ms])
        ref = filled(ms)
        twin_batch = bdd_hip_batch([m["t"] for m in ms])
        twin_batch.learned_iterations_history(w, 7, omega=OMEGA, compute_history_for_itr=3, history_avg_beta=BETA, **dict(zip(NAMES, ref)))
        twin_batch.close()
        for m, o, r in zip(ms, split(ms, outs), split(ms, ref)):
            assert_arrays(state(m["s"]), state(m["t"]), ("lo", "hi", "deferred mm", "delta", "lower bound"), True, precision, f"slope {slope} {m['name']}")
            assert_arrays(o, r, NAMES, True, precision, f"slope {slope} {m['name']}")
    batch.close()


# ---------------------------------------------------------------- 5. ordering against the members' streams
@pytest.mark.parametrize("precision", ["float", "double"])
def test_stop_batch_interleaved_with_other_calls(precision):
    """ordered after what is queued on every member's stream and in front of what a member does next, without the host having waited; a
    member whose costs-to-terminal are stale gets its backward run first (the bound on entry is read from what it leaves)"""
    ms = members(precision)
    batch = bdd_hip_batch([m["s"] for m in ms])
    rng = np.random.default_rng(23)
    batch.iterations(2)
    for i, m in enumerate(ms):
        m["t"].iterations(2)
        if i % 3 == 0:
            d = rng.uniform(-0.5, 0.5, size=m["s"].nr_variables())
            m["s"].update_costs([], d)
            m["t"].update_costs([], d)
        elif i % 3 == 1:
            m["s"].iteration()
            m["t"].iteration()
    counts, outs = batch_call(batch, ms, 40, SLOPE, 2)
    for i, m in enumerate(ms):
        if i % 2 == 0:      # right behind it
            m["s"].iteration()
    per_member = split(ms, outs)
    for i, (m, c, o) in enumerate(zip(ms, counts, per_member)):
        ref_c, ref_o = member_call(m["t"], m, 40, SLOPE, 2)
        if i % 2 == 0:
            m["t"].iteration()
        if m["exact"]:
            assert c == ref_c, (m["name"], c, ref_c)
        if c == ref_c:
            assert_arrays(state(m["s"]), state(m["t"]), ("lo", "hi", "deferred mm", "delta", "lower bound"), m["exact"], precision, m["name"])
            assert_arrays(o, ref_o, NAMES, m["exact"], precision, m["name"])
    batch.close()


# ---------------------------------------------------------------- 6. refusals
def test_stop_refusals_leave_every_member_unchanged():
    ms = members("float", keys=("assign8", "cover40x60", "cover67x100"))
    batch = bdd_hip_batch([m["s"] for m in ms])
    first, _ = batch_call(batch, ms, 2, SLOPE, 0)
    before = [state(m["s"]) for m in ms]
    w = np.concatenate([m["w"] for m in ms])
    outs = filled(ms)

    def unchanged():
        for m, b in zip(ms, before):
            for x, y in zip(state(m["s"]), b):
                np.testing.assert_array_equal(x, y)
        assert all(np.all(x == FILL) for x in outs)

    # the NULL count array: the C entry point itself
    lib = capi.lib()
    for slope in (SLOPE, 0.0):
        rc = lib.bddmma_learned_iterations_stop_batch(batch._h, w.ctypes.data, None, OMEGA, 5, slope, outs[0].ctypes.data, outs[1].ctypes.data, outs[2].ctypes.data,
                                                      2, BETA, 0, None)
        assert rc == capi.ERR_INVALID_ARGUMENT and b"iterations_done" in lib.bddmma_batch_last_error(batch._h)
        unchanged()
    # a null history array; a negative weight
    msg = refused(capi.ERR_INVALID_ARGUMENT, lambda: batch.learned_iterations_stopping(w, 5, improvement_slope=SLOPE, compute_history_for_itr=2, sol_avg=outs[0],
                                                                                lb_first_diff_avg=None, lb_second_diff_avg=outs[2]))
    assert "lb_first_diff_avg" in msg
    unchanged()
    bad = w.copy()
    bad[ms[0]["s"].nr_layers() + 3] = -0.5
    msg = refused(capi.ERR_INVALID_ARGUMENT, lambda: batch.learned_iterations_stopping(bad, 5, improvement_slope=SLOPE, compute_history_for_itr=2,
                                                                                **dict(zip(NAMES, outs))))
    assert "member 1" in msg and "dist_weights" in msg
    unchanged()
    batch.close()
    # the members go on as if nothing had been asked: the follow-up of the two iterations above on a fresh twin
    for m, c in zip(ms, first):
        assert member_call(m["t"], m, 2, SLOPE, 0)[0] == c
        a, b = member_call(m["s"], m, 3, SLOPE, 0)[0], member_call(m["t"], m, 3, SLOPE, 0)[0]
        assert a == b
        assert_arrays(state(m["s"]), state(m["t"]), ("lo", "hi", "deferred mm", "delta", "lower bound"), True, "float", m["name"])


def test_a_member_without_the_learned_form_is_refused():
    """cover160x240 in double is fused_small and not fused_small_learned (tests/test_gpu_small_learned.py), hence not fused_small_stop: the
    refusal names it and comes before any member, output or initial change is touched"""
    a = members("double", keys=("assign8",))[0]
    b = bdd_hip_parallel_mma(*instance("cover160x240", 0), precision="double")
    assert b.nr_packs() == 8 and b.fused_small() and not b.fused_small_learned() and not b.fused_small_stop() and a["s"].fused_small_stop()
    batch = bdd_hip_batch([a["s"], b])
    before = [state(s) for s in (a["s"], b)]
    w = np.concatenate([a["w"], dirichlet_weights(b, np.random.default_rng(41))])
    nl, nb = a["s"].nr_layers() + b.nr_layers(), a["s"].nr_bdds() + b.nr_bdds()
    outs = [np.full(nl, FILL), np.full(nb, FILL), np.full(nb, FILL)]
    msg = refused(capi.ERR_UNSUPPORTED, lambda: batch.learned_iterations_stopping(w, 5, improvement_slope=SLOPE, compute_history_for_itr=3, history_avg_beta=BETA,
                                                                           **dict(zip(NAMES, outs))))
    assert "member 1" in msg and "fused_small_stop" in msg
    for s, bf in zip((a["s"], b), before):
        for x, y in zip(state(s), bf):
            np.testing.assert_array_equal(x, y)
    assert all(np.all(x == FILL) for x in outs)
    batch.close()
    # the initial change of member 0 is still unset: its first learned call sets it, as its twin's does
    assert member_call(a["s"], a, NUM_ITR, SLOPE, 0)[0] == member_call(a["t"], a, NUM_ITR, SLOPE, 0)[0]
    assert_arrays(state(a["s"]), state(a["t"]), ("lo", "hi", "deferred mm", "delta", "lower bound"), True, "double", "assign8")


# ---------------------------------------------------------------- 7. against the restatement
def test_count_of_one_member_vs_restatement():
    """the Python model tests/test_gpu_learned_mma.py compares the per-member call's count with"""
    m = members("double", keys=("assign8",))[0]
    s, perm = m["s"], m["s"].bdd_major_order()
    r = LearnedMma(m["col"].instr, m["col"].delims, "double")
    r.update_costs_hi(np.asarray(m["costs"], np.float64))
    batch = bdd_hip_batch([s])
    counts, _ = batch_call(batch, [m], 500, SLOPE, 0)
    batch.close()
    assert 1 < counts[0] < 500 and counts[0] == r.iterations(m["w"][perm].astype(np.float64), 500, OMEGA, improvement_slope=SLOPE)


# ---------------------------------------------------------------- 8. DualIterations
@pytest.mark.parametrize("history", [0, 3])
@pytest.mark.parametrize("precision", ["float", "double"])
def test_dual_iterations_with_a_slope_take_the_batched_branch(precision, history, monkeypatch):
    """the forward of a batch with improvement_slope > 0: one set_solver_costs, one learned_iterations_stopping, one get_solver_costs of the
    batch and no learned call on a member (calls that returned are counted); results and gradients equal the list form's"""
    import torch
    from bdd_amd.autograd import DualIterations
    from test_gpu_small_learned import AUTOGRAD_MEMBERS, _assert_tiered
    tdt = torch.float64 if precision == "double" else torch.float32
    a = [bdd_hip_parallel_mma(*instance(n, 1), precision=precision) for n in AUTOGRAD_MEMBERS]
    b = [bdd_hip_parallel_mma(*instance(n, 1), precision=precision) for n in AUTOGRAD_MEMBERS]
    assert all(s.fused_small_stop() for s in a + b)
    batch = bdd_hip_batch(a)
    calls = {}

    def count(obj, name, key):
        inner = getattr(obj, name)

        def counted(*args, **kw):
            r = inner(*args, **kw)
            calls[key] = calls.get(key, 0) + 1
            return r
        monkeypatch.setattr(obj, name, counted)

    for s in a:
        count(s, "learned_iterations", "member")
        count(s, "set_solver_costs", "member")
        count(s, "get_solver_costs", "member")
    for s in b:
        count(s, "learned_iterations", "list")
    for name in ("set_solver_costs", "learned_iterations_stopping", "learned_iterations_history", "learned_iterations", "get_solver_costs"):
        count(batch, name, "batch." + name)
    rng = np.random.default_rng(25)
    costs = [s.get_solver_costs() for s in a]
    calls.clear()
    lo, hi = (np.concatenate([c[k] for c in costs]) for k in range(2))
    mm = rng.uniform(-0.25, 0.25, lo.size).astype(a[0].value_type)
    w = np.concatenate([dirichlet_weights(s, rng) for s in a])
    om = np.asarray([0.5], a[0].value_type)
    g = [rng.normal(0, 1, lo.size).astype(a[0].value_type) for _ in range(3)]
    results, done = [], []
    for solvers in (batch, list(b)):
        t = [torch.tensor(x, dtype=tdt, device="cuda", requires_grad=True) for x in (lo, hi, mm, w, om)]
        out = DualIterations.apply(solvers, *t[:4], 60, t[4], 3, SLOPE, 1, history, 0.9)
        torch.cuda.synchronize()
        if solvers is batch:
            forward_calls = dict(calls)
        done.append(list(out[0].grad_fn.iterations_done))
        torch.autograd.backward(out[:3], [torch.tensor(x, dtype=tdt, device="cuda") for x in g])
        torch.cuda.synchronize()
        results.append(([o.detach().cpu().numpy() for o in out if o is not None], [x.grad.cpu().numpy() for x in t]))
    batch.close()
    print(f"[batch stop] DualIterations {precision} history {history}: counts batch {done[0]} list {done[1]}")
    assert forward_calls == {"batch.set_solver_costs": 1, "batch.learned_iterations_stopping": 1, "batch.get_solver_costs": 1}, forward_calls
    assert calls.get("list") == len(b) and "batch.learned_iterations_history" not in calls and "batch.learned_iterations" not in calls, calls
    for i, n in enumerate(AUTOGRAD_MEMBERS):
        if precision == "float" or n.startswith("assign"):
            assert done[0][i] == done[1][i], (n, done)
    if done[0] == done[1]:
        (out_b, grad_b), (out_l, grad_l) = results
        assert len(out_b) == len(out_l) == (6 if history else 3)
        off = np.cumsum([0] + [s.nr_layers() for s in a])
        _assert_tiered(out_b, out_l, off, precision)
        _assert_tiered(grad_b, grad_l, off, precision)
