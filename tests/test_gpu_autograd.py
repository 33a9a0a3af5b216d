"""GPU tests of bdd_amd/autograd.py (the torch autograd Functions over the learned solver's operators), of bddmma_stream_wait /
bddmma_stream_signal, and of the combined load of grad_learned_iterations' device arguments (k_load_checked).

The yardstick of the Functions is the solver class itself: a Function is a sequence of bdd_hip_parallel_mma calls on slices of batch tensors,
so every forward output and every gradient must equal — bit for bit — the same methods driven by hand with NumPy copies of the same slices
on a second set of solvers built the same way (deterministic exchange: include/bdd_mma.h promises bit-reproducibility).  No tolerance
anywhere except the one finite-difference check, whose step and allowance are those of
test_gpu_grad_iterations.test_directional_derivative_on_the_device_in_double.

A batch is three solvers of different shape (every offset differs from every size): assignment8, knapsack_w64 and cover10_w64 on its
240-layer instance; one more batch has wide and huge packs (mixed, huge).  Inputs: grad_iterations_restatement.seeded_inputs on the seeds
tests/test_grad_iterations_restatement.py records as tie-free."""
import numpy as np
import pytest
import torch

from bdd_amd import capi
from bdd_amd.autograd import (ComputeAllMinMarginalsDiff, ComputeLowerBoundperBDD, ComputePerBDDSolutions, ComputePerBDDSolutionsIdentityBackward,
                              ComputePrimalSolution, DistributeDeferredDelta, DualIterations, GetMarginalProbability, GetSumMarginals, PerturbPrimalCosts,
                              batch_index)
from bdd_amd.capi import BddMmaError
from bdd_amd.solver import bdd_hip_lbfgs, bdd_hip_parallel_mma
from grad_iterations_restatement import grad_iterations_of, seeded_inputs
from test_grad_iterations_restatement import SEEDS, instance_of
from test_gpu_sum_marginals import FAMILIES

pytestmark = pytest.mark.gpu

SMALL = ("assignment8", "knapsack_w64", "cover10_w64")
WIDE = ("mixed", "huge")
TORCH = {np.float32: torch.float32, np.float64: torch.float64}


class Batch:
    """two sets of solvers built alike (`auto` for the Functions, `hand` for the methods called by hand), the restatement models and the
    seeded inputs of every member in the public layer order"""

    def __init__(self, families, precision):
        self.auto, self.hand, self.models, self.perms, self.pub = [], [], [], [], []
        for f in families:
            small = "float" if f.startswith("cover10") else precision   # the covering family: its 240-layer instance in both precisions
            col, costs = instance_of(f, small)
            for dst in (self.auto, self.hand):
                dst.append(bdd_hip_parallel_mma(col, costs, precision=precision, deterministic=True, **FAMILIES[f][1]))
            m = grad_iterations_of(col, precision)
            x = seeded_inputs(m, SEEDS[f][small][0] or SEEDS[f]["double"][0])
            perm = self.auto[-1].bdd_major_order()
            pub = {}
            for k, v in x.items():
                pub[k] = np.empty_like(v)
                pub[k][perm] = v
                pub[k] = pub[k].astype(self.auto[-1].value_type)
            self.models.append(m); self.perms.append(perm); self.pub.append(pub)
        self.vt = self.auto[0].value_type
        self.ix = batch_index(self.auto)
        self.L, self.B, self.V = self.ix.layer_offsets, self.ix.bdd_offsets, self.ix.variable_offsets

    def cat(self, key, scale=1.0):
        return np.concatenate([(p[key] * self.vt(scale)).astype(self.vt) for p in self.pub])

    def dev(self, a, grad=False):
        return torch.from_numpy(np.ascontiguousarray(a, self.vt)).to("cuda").requires_grad_(grad)

    def random(self, offsets, seed):
        """values that are exact in float32, one per entry of a batch tensor over `offsets`"""
        return np.random.Generator(np.random.PCG64(seed)).normal(0, 1, offsets[-1]).astype(np.float32).astype(self.vt)

    def close(self):
        for s in self.auto + self.hand:
            s.close()


def _same(got, want, what):
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    want = np.concatenate([np.atleast_1d(w) for w in want]) if isinstance(want, (list, tuple)) else np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    np.testing.assert_array_equal(got, want, err_msg=what)


def _dual_iterations_by_hand(b, lo, hi, mm, w, omega, num_itr, slope, history, beta):
    """learned_iterations of every `hand` solver from NumPy slices -> (outputs per solver, iterations done per solver)"""
    outs, done = [], []
    for i, s in enumerate(b.hand):
        l = slice(b.L[i], b.L[i + 1])
        s.set_solver_costs(lo[l], hi[l], mm[l])
        hist = [np.zeros(s.nr_layers(), b.vt), np.zeros(s.nr_bdds(), b.vt), np.zeros(s.nr_bdds(), b.vt)]
        kw = dict(sol_avg=hist[0], lb_first_diff_avg=hist[1], lb_second_diff_avg=hist[2]) if history else {}
        vec = np.ascontiguousarray(omega[l]) if omega.size > 1 else None
        done.append(s.learned_iterations(np.ascontiguousarray(w[l]), num_itr, omega=0.5 if vec is not None else float(omega[0]), improvement_slope=slope,
                                         compute_history_for_itr=history, history_avg_beta=beta, omega_vec=vec, **kw))
        outs.append(list(s.get_solver_costs()) + hist)
    return outs, done


def _grad_iterations_by_hand(b, lo, hi, mm, w, omega, g, done, max_itr, num_caches):
    res = []
    for i, s in enumerate(b.hand):
        l = slice(b.L[i], b.L[i + 1])
        s.set_solver_costs(lo[l], hi[l], mm[l])
        n = min(done[i], max_itr)
        vec = np.ascontiguousarray(omega[l]) if omega.size > 1 else None
        res.append(s.grad_iterations(np.ascontiguousarray(w[l]), g[0][l], g[1][l], g[2][l], 0.5 if vec is not None else float(omega[0]), done[i] - n, n, num_caches,
                                     omega_vec=vec))
    return res


def _sum_in_order(values, vt):
    total = vt(values[0])
    for v in values[1:]:
        total = vt(total + vt(v))
    return total


@pytest.mark.parametrize("slope,history", [(0.0, 0), (0.02, 3)], ids=["all_iterations", "slope_and_history"])
@pytest.mark.parametrize("omega_vec", [False, True], ids=["omega", "omega_vec"])
@pytest.mark.parametrize("precision", ["double", "float"])
def test_dual_iterations_equal_the_calls_they_make(precision, omega_vec, slope, history):
    b = Batch(SMALL, precision)
    lo, hi, mm, w = b.cat("lo"), b.cat("hi"), b.cat("g_mm", 0.25), b.cat("alpha")
    omega = b.cat("omega_vec") if omega_vec else np.array([0.5], b.vt)
    g = [b.cat("g_lo"), b.cat("g_hi"), b.cat("g_mm")]
    num_itr, max_itr, caches, beta = 24, 2, 2, 0.9
    t = [b.dev(a, True) for a in (lo, hi, mm, w, omega)]
    out = DualIterations.apply(b.auto, *t[:4], num_itr, t[4], max_itr, slope, caches, history, beta)
    want, done = _dual_iterations_by_hand(b, lo, hi, mm, w, omega, num_itr, slope, history, beta)
    print(f"{precision} {'omega_vec' if omega_vec else 'omega'} slope {slope}: iterations done per solver {done}")
    assert out[0].grad_fn.iterations_done == done
    if slope == 0.0:
        assert done == [num_itr] * len(b.auto)
    else:   # the stopping rule fired, every solver on its own bound
        assert all(history <= d < num_itr for d in done)
    for k, nm in enumerate(("lo", "hi", "def_mm")):
        _same(out[k], [x[k] for x in want], nm)
    if history:
        for k, nm in ((3, "sol_avg"), (4, "lb_first_diff_avg"), (5, "lb_second_diff_avg")):
            _same(out[k], [x[k] for x in want], nm)
            assert not out[k].requires_grad
        assert out[3].shape == (b.L[-1],) and out[4].shape == (b.B[-1],)
    else:
        assert out[3] is None and out[4] is None and out[5] is None
    torch.autograd.backward(list(out[:3]), [b.dev(x) for x in g])
    res = _grad_iterations_by_hand(b, lo, hi, mm, w, omega, g, done, max_itr, caches)
    for k, nm in enumerate(("grad lo", "grad hi", "grad def_mm", "grad dist_weights")):
        _same(t[k].grad, [r[k] for r in res], nm)
    if omega_vec:
        _same(t[4].grad, [r[4] for r in res], "grad omega_vec")
    else:   # one omega for all solvers: the sum of their values, in list order, in the solvers' precision
        _same(t[4].grad, np.array([_sum_in_order([r[4][0] for r in res], b.vt)]), "grad omega")
        assert any(r[4][0] != 0 for r in res)
    # a missing incoming gradient is zeros: only lo's output is used
    t2 = [b.dev(a, True) for a in (lo, hi, mm, w, omega)]
    out2 = DualIterations.apply(b.auto, *t2[:4], num_itr, t2[4], max_itr, slope, caches, 0, beta)
    counted = out2[0].grad_fn.iterations_done
    out2[0].backward(b.dev(g[0]))
    zero = np.zeros_like(g[0])
    done2 = _dual_iterations_by_hand(b, lo, hi, mm, w, omega, num_itr, slope, 0, beta)[1]
    assert counted == done2
    res2 = _grad_iterations_by_hand(b, lo, hi, mm, w, omega, [g[0], zero, zero], done2, max_itr, caches)
    for k in range(4):
        _same(t2[k].grad, [r[k] for r in res2], f"lo only, gradient {k}")
    b.close()


def _single_shot_functions(b):
    """every other Function and helper against the methods, on batch b"""
    vt = b.vt
    lo, hi, mm = b.cat("lo"), b.cat("hi"), b.cat("g_mm", 0.25)
    g_lo, g_hi, g_mm = b.cat("g_lo"), b.cat("g_hi"), b.cat("g_mm")
    zero = [np.zeros(s.nr_layers(), vt) for s in b.hand]
    sl = [slice(x, y) for x, y in zip(b.L[:-1], b.L[1:])]
    # DistributeDeferredDelta; its where() form against grad_distribute_delta
    t = [b.dev(a, True) for a in (lo, hi, mm)]
    out = DistributeDeferredDelta.apply(b.auto, *t)
    want, want_g = [], []
    for s, l in zip(b.hand, sl):
        s.set_solver_costs(lo[l], hi[l], mm[l])
        s.distribute_delta()
        want.append(s.get_solver_costs())
        assert not want[-1][2].any()
        want_g.append(s.grad_distribute_delta(g_lo[l], g_hi[l]))
    _same(out[0], [x[0] for x in want], "distribute lo")
    _same(out[1], [x[1] for x in want], "distribute hi")
    torch.autograd.backward(list(out), [b.dev(g_lo), b.dev(g_hi)])
    _same(t[0].grad, g_lo, "distribute grad lo")
    _same(t[1].grad, g_hi, "distribute grad hi")
    _same(t[2].grad, want_g, "distribute grad def_mm")
    assert (mm > 0).any() and (mm <= 0).any()
    # ComputeAllMinMarginalsDiff
    t = [b.dev(a, True) for a in (lo, hi)]
    out = ComputeAllMinMarginalsDiff.apply(b.auto, *t)
    want, want_g = [], []
    for s, l, z in zip(b.hand, sl, zero):
        s.set_solver_costs(lo[l], hi[l], z)
        want.append(s.min_marginal_diff())
        want_g.append(s.grad_all_min_marginal_differences(g_mm[l]))
    _same(out, want, "min-marginal differences")
    out.backward(b.dev(g_mm))
    _same(t[0].grad, [x[0] for x in want_g], "mm diff grad lo")
    _same(t[1].grad, [x[1] for x in want_g], "mm diff grad hi")
    # PerturbPrimalCosts
    p_lo, p_hi = b.random(b.V, 31), b.random(b.V, 32)
    vs = [slice(x, y) for x, y in zip(b.V[:-1], b.V[1:])]
    t = [b.dev(a, True) for a in (p_lo, p_hi, lo, hi)]
    out = PerturbPrimalCosts.apply(b.auto, *t)
    want, want_g = [], []
    for s, l, v, z in zip(b.hand, sl, vs, zero):
        s.set_solver_costs(lo[l], hi[l], z)
        s.update_costs(p_lo[v], p_hi[v])
        want.append(s.get_solver_costs())
        want_g.append(s.grad_cost_perturbation(g_lo[l], g_hi[l]))
    _same(out[0], [x[0] for x in want], "perturbed lo")
    _same(out[1], [x[1] for x in want], "perturbed hi")
    torch.autograd.backward(list(out), [b.dev(g_lo), b.dev(g_hi)])
    _same(t[0].grad, [x[0] for x in want_g], "grad lo perturbation")
    _same(t[1].grad, [x[1] for x in want_g], "grad hi perturbation")
    _same(t[2].grad, g_lo, "perturbation: grad lo")
    _same(t[3].grad, g_hi, "perturbation: grad hi")
    # ComputeLowerBoundperBDD, plain and smooth gradients
    g_lb = b.random(b.B, 33)
    bs = [slice(x, y) for x, y in zip(b.B[:-1], b.B[1:])]
    for temp in (0.0, 2.0):
        t = [b.dev(a, True) for a in (lo, hi)]
        out = ComputeLowerBoundperBDD.apply(b.auto, *t, temp)
        want, want_g = [], []
        for s, l, bb, z in zip(b.hand, sl, bs, zero):
            s.set_solver_costs(lo[l], hi[l], z)
            want.append(s.lower_bound_per_bdd())
            if temp > 0:
                s.set_solver_costs(lo[l] / vt(temp), hi[l] / vt(temp), z)
                want_g.append(s.grad_smooth_lower_bound_per_bdd(g_lb[bb]))
            else:
                want_g.append(s.grad_lower_bound_per_bdd(g_lb[bb]))
        _same(out, want, f"lower bound per BDD, temperature {temp}")
        out.backward(b.dev(g_lb))
        _same(t[0].grad, [x[0] for x in want_g], f"grad lo of the bound, temperature {temp}")
        _same(t[1].grad, [x[1] for x in want_g], f"grad hi of the bound, temperature {temp}")
    # the solutions, with the straight-through backward; sum-marginals; the smooth solution
    want_sol, want_sm, want_log, want_p = [], [], [], []
    for s, l, z in zip(b.hand, sl, zero):
        s.set_solver_costs(lo[l], hi[l], z)
        want_sol.append(s.bdds_solution_vec().astype(vt))
        want_log.append(s.sum_marginals_cuda(False, True)[1:])
        want_sm.append(s.sum_marginals_cuda(False, False)[1:])
        want_p.append(s.smooth_solution_per_bdd())
    _same(ComputePerBDDSolutions(b.auto, b.dev(lo), b.dev(hi)), want_sol, "solutions")
    for norm in (None, 0.25):
        t = [b.dev(a, True) for a in (lo, hi)]
        out = ComputePerBDDSolutionsIdentityBackward.apply(b.auto, *t, norm)
        _same(out, want_sol, "solutions (identity backward)")
        out.backward(b.dev(g_mm))
        _same(t[0].grad, g_mm * vt(norm or 1.0), "identity backward lo")
        _same(t[1].grad, -g_mm * vt(norm or 1.0), "identity backward hi")
    for logits, want in ((True, want_log), (False, want_sm)):
        got = GetSumMarginals(b.auto, b.dev(lo), b.dev(hi), logits)
        _same(got[0], [x[0] for x in want], f"sum-marginals lo, logits {logits}")
        _same(got[1], [x[1] for x in want], f"sum-marginals hi, logits {logits}")
    _same(GetMarginalProbability(b.auto, b.dev(lo), b.dev(hi)), want_p, "marginal probability")


@pytest.mark.parametrize("precision", ["double", "float"])
def test_single_shot_functions_equal_the_calls_they_make(precision):
    b = Batch(SMALL, precision)
    _single_shot_functions(b)
    # the rounding helper: the same solutions, and a batch's worth of them
    lo, hi, mm = b.cat("lo"), b.cat("hi"), np.zeros(b.L[-1], b.vt)
    got = ComputePrimalSolution(b.auto, b.dev(lo), b.dev(hi), b.dev(mm), 0.1, 1.2, 5)
    for i, s in enumerate(b.hand):
        l = slice(b.L[i], b.L[i + 1])
        s.set_solver_costs(lo[l], hi[l], mm[l])
        assert got[i] == s.primal_rounding_incremental(0.1, 1.2, 5)
        assert len(got[i]) in (0, s.nr_variables())
    b.close()


@pytest.mark.parametrize("precision", ["double", "float"])
def test_wide_and_huge_packs(precision):
    b = Batch(WIDE, precision)
    _single_shot_functions(b)
    lo, hi, mm, w, omega = b.cat("lo"), b.cat("hi"), b.cat("g_mm", 0.25), b.cat("alpha"), np.array([0.5], b.vt)
    g = [b.cat("g_lo"), b.cat("g_hi"), b.cat("g_mm")]
    t = [b.dev(a, True) for a in (lo, hi, mm, w, omega)]
    out = DualIterations.apply(b.auto, *t[:4], 3, t[4], 2, 0.0, 1, 0, 0.9)
    want, done = _dual_iterations_by_hand(b, lo, hi, mm, w, omega, 3, 0.0, 0, 0.9)
    for k in range(3):
        _same(out[k], [x[k] for x in want], f"output {k}")
    torch.autograd.backward(list(out[:3]), [b.dev(x) for x in g])
    res = _grad_iterations_by_hand(b, lo, hi, mm, w, omega, g, done, 2, 1)
    for k in range(4):
        _same(t[k].grad, [r[k] for r in res], f"gradient {k}")
    _same(t[4].grad, np.array([_sum_in_order([r[4][0] for r in res], b.vt)]), "grad omega")
    b.close()


UNTRACKED, TRACKED = 1, 2


def _chain(b, lo, hi, mm, w, omega, c, untracked=UNTRACKED):
    lo1, hi1, mm1, _, _, _ = DualIterations.apply(b.auto, lo, hi, mm, w, untracked + TRACKED, omega, TRACKED, 0.0, 1, 0, 0.9)
    lo2, hi2 = DistributeDeferredDelta.apply(b.auto, lo1, hi1, mm1)
    return (ComputeLowerBoundperBDD.apply(b.auto, lo2, hi2) * c).sum()


@pytest.mark.parametrize("precision", ["double", "float"])
def test_a_whole_chain_through_autograd(precision):
    """DualIterations (1 untracked + 2 tracked) -> DistributeDeferredDelta -> ComputeLowerBoundperBDD -> a weighted sum -> backward(): the
    leaves' gradients equal the chain composed by hand from the methods, bit for bit.  In double also one directional derivative against
    finite differences of the autograd forward.  As in the reference, DualIterations backpropagates through its tracked iterations only:
    what it returns for (lo, hi, def_mm) is the gradient with respect to the state after the untracked iteration, the untracked one being
    treated as a constant.  So the differences are taken there: the same chain's forward with the two tracked iterations alone, started
    from the device's own state after the untracked one, moved along a direction |dir| <= 1.  Step and allowance are those of
    test_gpu_grad_iterations.test_directional_derivative_on_the_device_in_double: eps = the smallest decision gap of the tracked
    trajectory / (8 * layers of the longest BDD), allowance 64 eps(double) * sum |incoming| * M / eps, where incoming are the gradients that
    enter the iterations' backward (each layer of BDD b carries |c_b|: the rounding of a bound is that of a path's costs) and M the largest
    |path cost|; the allowance must stay below a hundredth of the derivative."""
    b = Batch(SMALL, precision)
    vt = b.vt
    lo, hi, mm, w = b.cat("lo"), b.cat("hi"), np.zeros(b.L[-1], vt), b.cat("alpha")
    omega = np.array([0.5], vt)
    c = np.abs(b.random(b.B, 41)) + vt(0.5)
    t = [b.dev(a, True) for a in (lo, hi, mm, w, omega)]
    loss = _chain(b, *t, b.dev(c))
    loss.backward()
    # by hand
    res, after, incoming, states = [], [], [], []
    for i, s in enumerate(b.hand):
        l, bb = slice(b.L[i], b.L[i + 1]), slice(b.B[i], b.B[i + 1])
        s.set_solver_costs(lo[l], hi[l], mm[l])
        assert s.learned_iterations(np.ascontiguousarray(w[l]), UNTRACKED, 0.5, improvement_slope=0.0) == UNTRACKED
        states.append([v.copy() for v in s.get_solver_costs()])
        assert s.learned_iterations(np.ascontiguousarray(w[l]), TRACKED, 0.5, improvement_slope=0.0) == TRACKED
        s.distribute_delta()
        after.append(s.lower_bound_per_bdd())
        g_lo, g_hi = s.grad_lower_bound_per_bdd(np.ascontiguousarray(c[bb]))
        g_mm = s.grad_distribute_delta(g_lo, g_hi)
        incoming.append((g_lo, g_hi, g_mm))
        s.set_solver_costs(lo[l], hi[l], mm[l])
        res.append(s.grad_iterations(np.ascontiguousarray(w[l]), g_lo, g_hi, g_mm, 0.5, UNTRACKED, TRACKED, 1))
    for k, nm in enumerate(("lo", "hi", "def_mm", "dist_weights")):
        _same(t[k].grad, [r[k] for r in res], "chain: grad " + nm)
    _same(t[4].grad, np.array([_sum_in_order([r[4][0] for r in res], vt)]), "chain: grad omega")
    want_loss = torch.from_numpy(np.concatenate(after) * c).to("cuda").sum()
    assert loss.item() == want_loss.item()
    if precision == "double":
        eps, mag, inc = np.inf, 0.0, 0.0
        for i, m in enumerate(b.models):
            perm, pub = b.perms[i], b.pub[i]
            major = lambda v: np.asarray(v, np.float64)[perm]
            st = states[i]
            gap, mg = m.trajectory_gap(major(st[0]), major(st[1]), major(st[2]), major(pub["alpha"]), 0.5, TRACKED, *(major(v) for v in incoming[i]), np.longdouble)
            eps = min(eps, float(gap.min()) / (8 * int(np.max(np.diff(m.bdd_layer_ptr)))))
            mag = max(mag, float(mg.max()))
            inc += float(sum(np.abs(v).sum() for v in incoming[i]))
        rng = np.random.Generator(np.random.PCG64(12))
        dirs = [rng.uniform(-1, 1, b.L[-1]) for _ in range(3)]
        with torch.no_grad():
            cd = b.dev(c)
            at = [np.concatenate([st[k] for st in states]) for k in range(3)]
            base = _chain(b, *(b.dev(a) for a in (*at, w, omega)), cd, 0).item()
            moved = _chain(b, *(b.dev(a + eps * d) for a, d in zip(at, dirs)), b.dev(w), b.dev(omega), cd, 0).item()
            assert base == loss.item()   # the same state, the same kernels: the chain's own loss
        lhs = (moved - base) / eps
        rhs = float(sum(np.dot(t[k].grad.cpu().numpy(), dirs[k]) for k in range(3)))
        allowed = 64 * np.finfo(np.float64).eps * inc * mag / eps
        print(f"chain: eps {eps:.3e}, finite differences {lhs:.12g}, J^T g . dir {rhs:.12g}, allowed {allowed:.3e}")
        assert eps > 1e-8 and allowed <= 1e-2 * abs(rhs)
        assert abs(lhs - rhs) <= allowed
    b.close()


def _sleep_cycles(ms):
    """cycles for torch.cuda._sleep that keep a stream busy for about `ms` (measured on a short spin; at most 2^31 cycles)"""
    a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    probe = 1 << 20
    torch.cuda._sleep(probe)
    torch.cuda.synchronize()
    a.record(); torch.cuda._sleep(probe); z.record()
    torch.cuda.synchronize()
    per_ms = probe / max(a.elapsed_time(z), 1e-3)
    return int(min(ms * per_ms, 2 ** 31 - 1))


@pytest.mark.parametrize("precision", ["double", "float"])
def test_stream_ordering_needs_no_host_synchronisation(precision):
    """On a torch stream of its own: a spin of a few tens of milliseconds, then the kernels that write the (zero-filled) inputs, then the
    Functions with no host synchronisation in between, the outputs read on the same stream.  Without stream_wait the solvers would read
    the zeros (stale memory, no fault) and the results would differ from the synchronised call's.  Likewise an input overwritten on that
    stream right after a Function returns must not change its result (stream_signal).
    Control, measured once with stream_wait turned into a no-op: with 16 hardware queues per process (GPU_MAX_HW_QUEUES) the comparison fails, as
    it should; with HIP's default of 4 the runtime multiplexes torch's stream pool and the solvers' streams over the same queues, serialises
    them, and the missing wait stays hidden.  The test asks for the ordering everywhere and can catch its absence only where the two streams
    run side by side."""
    b = Batch(SMALL, precision)
    src = [b.dev(b.cat(k)) for k in ("lo", "hi")] + [b.dev(b.cat("g_mm", 0.25)), b.dev(b.cat("alpha")), b.dev(np.array([0.5], b.vt))]
    args = (4, 2, 0.0, 1, 0, 0.9)
    torch.cuda.synchronize()
    want_mm = ComputeAllMinMarginalsDiff.apply(b.auto, src[0], src[1])
    want = DualIterations.apply(b.auto, *src[:4], args[0], src[4], *args[1:])
    torch.cuda.synchronize()
    want_mm, want = want_mm.cpu(), [x.cpu() for x in want[:3]]
    assert want_mm.abs().sum() > 0
    cycles = _sleep_cycles(30.0)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        t = [torch.zeros_like(x) for x in src[:4]]
        torch.cuda.synchronize()
        torch.cuda._sleep(cycles)
        for dst, s_ in zip(t, src):
            dst.copy_(s_, non_blocking=True)
        busy = not side.query()
        got_mm = ComputeAllMinMarginalsDiff.apply(b.auto, t[0], t[1])
        t[0].fill_(float("nan")); t[1].fill_(float("nan"))     # right behind the Function: must not reach what it queued
        for dst, s_ in zip(t[:2], src[:2]):
            dst.copy_(s_, non_blocking=True)
        got = DualIterations.apply(b.auto, *t, args[0], src[4], *args[1:])
        for x in t:
            x.fill_(float("nan"))
        got_mm, got = got_mm.cpu(), [x.cpu() for x in got[:3]]   # read on the same stream
    torch.cuda.synchronize()
    print(f"{precision}: spin of {cycles} cycles; the stream was still busy when the first Function was called: {busy}")
    assert torch.equal(got_mm, want_mm)
    for x, y in zip(got, want):
        assert torch.equal(x, y)
    b.close()


def _state(s):
    return list(s.get_solver_costs()) + [s.get_delta(), s.lower_bound()]


@pytest.mark.parametrize("precision", ["double", "float"])
def test_refusals_leave_every_solver_alone(precision):
    b = Batch(SMALL, precision)
    for s, p in zip(b.auto, b.pub):
        s.set_solver_costs(p["lo"], p["hi"], np.zeros(s.nr_layers(), b.vt))
        s.iterations(2)   # a state with deferred differences and a delta
    before = [_state(s) for s in b.auto]

    def untouched():
        for s, old in zip(b.auto, before):
            for x, y in zip(old, _state(s)):
                np.testing.assert_array_equal(np.asarray(x), np.asarray(y))

    lo, hi, mm, w, omega = (b.dev(b.cat(k)) for k in ("lo", "hi", "g_mm", "alpha", "omega_vec"))
    n = b.L[-1]
    other = torch.float32 if precision == "double" else torch.float64
    wrong = {"dtype": lo.to(other), "a host tensor": lo.cpu(), "not contiguous": torch.cat([lo, lo])[::2], "length": lo[:-1].clone()}
    for what, bad in wrong.items():
        assert bad.numel() in (n, n - 1)
        for name, call in (("hi_costs_batch", lambda: DualIterations.apply(b.auto, lo, bad, mm, w, 3, omega, 1, 0.0, 1, 0, 0.9)),
                           ("def_mm_batch", lambda: DistributeDeferredDelta.apply(b.auto, lo, hi, bad)),
                           ("lo_costs_batch", lambda: ComputeAllMinMarginalsDiff.apply(b.auto, bad, hi)),
                           ("hi_costs_batch", lambda: PerturbPrimalCosts.apply(b.auto, lo[:b.V[-1]].clone(), hi[:b.V[-1]].clone(), lo, bad)),
                           ("lo_costs_batch", lambda: ComputeLowerBoundperBDD.apply(b.auto, bad, hi)),
                           ("hi_costs_batch", lambda: ComputePerBDDSolutions(b.auto, lo, bad))):
            with pytest.raises(ValueError, match="^" + name + " "):
                call()
            untouched()
    # what the library refuses: today's codes and messages, as BddMmaError
    t = [x.clone().requires_grad_(True) for x in (lo, hi, mm, w)]
    out = DualIterations.apply(b.auto, *t, 3, omega, 2, 0.0, 1, 0, 0.9)
    g_hi = torch.zeros_like(hi)
    g_hi[b.L[1] + 1] = float("nan")
    with pytest.raises(BddMmaError, match=rf"error {capi.ERR_INVALID_ARGUMENT}: 1 values of grad_learned_iterations: grad_hi are not finite"):
        torch.autograd.backward(list(out[:3]), [torch.zeros_like(lo), g_hi, torch.zeros_like(lo)])
    bad_w = w.clone()
    bad_w[b.L[2] + 3] = -0.5
    with pytest.raises(BddMmaError, match=rf"error {capi.ERR_INVALID_ARGUMENT}: learned_iterations: 1 of the dist_weights are negative or not finite"):
        DualIterations.apply(b.auto, lo, hi, mm, bad_w, 3, omega, 1, 0.0, 1, 0, 0.9)
    out = DualIterations.apply(b.auto, *t, 3, omega, 2, 0.0, 1, 0, 0.9)
    wrapper = bdd_hip_lbfgs(b.auto[0])
    with pytest.raises(BddMmaError, match=f"error {capi.ERR_STATE}:"):
        out[0].sum().backward()
    wrapper.close()
    b.close()


@pytest.mark.parametrize("precision", ["double", "float"])
@pytest.mark.parametrize("family", ["knapsack_w64", "mixed", "huge"])
def test_combined_load_of_device_arguments(family, precision):
    """grad_iterations with every array on the device goes through one launch that copies and checks all of them: the arrays are still
    checked in the order omega_vec, dist_weights, grad_lo, grad_hi, grad_mm and the first offending one is reported in today's words; clean
    arrays give the host-input call's results bit for bit, whether or not the pointers allow 16-byte accesses."""
    b = Batch((family,), precision)
    s, pub = b.auto[0], b.pub[0]
    L = s.nr_layers()
    s.set_solver_costs(pub["lo"], pub["hi"], np.zeros(L, b.vt))
    s.iterations(2)
    before = _state(s)
    keys = ("alpha", "omega_vec", "g_lo", "g_hi", "g_mm")

    def on_device(arrays, shift):
        """device copies whose first element sits `shift` values behind a 256-byte boundary"""
        out = []
        for a in arrays:
            buf = torch.zeros(a.size + 64, dtype=TORCH[b.vt], device="cuda")
            buf[shift:shift + a.size] = torch.from_numpy(a)
            out.append(buf[shift:shift + a.size])
        return out

    def call(arrays, omega_vec, shift=0):
        d = on_device(arrays, shift)
        out = on_device([np.zeros(L, b.vt), np.zeros(L if omega_vec else 1, b.vt)], shift)
        s.grad_iterations(d[0], d[2], d[3], d[4], 0.5, 1, 2, 1, omega_vec=d[1] if omega_vec else None, out=out)
        return [x.cpu().numpy() for x in (d[2], d[3], d[4], out[0], out[1])]

    clean = [pub[k] for k in keys]
    for omega_vec in (False, True):
        host = s.grad_iterations(pub["alpha"], pub["g_lo"], pub["g_hi"], pub["g_mm"], 0.5, 1, 2, 1, omega_vec=pub["omega_vec"] if omega_vec else None)
        for shift in (0, 1, 3):
            for x, y in zip(host, call(clean, omega_vec, shift)):
                np.testing.assert_array_equal(x, y, err_msg=f"omega_vec {omega_vec}, shift {shift}")
    # the 2nd and the 4th array bad: the 2nd is named.  With omega_vec the arrays are (dist_weights, omega_vec, grad_lo, grad_hi, grad_mm) ...
    bad = [a.copy() for a in clean]
    bad[1][L // 3], bad[1][L - 1], bad[3][0] = -1.0, np.inf, np.nan
    with pytest.raises(BddMmaError, match=rf"error {capi.ERR_INVALID_ARGUMENT}: grad_learned_iterations: 2 of the omega_vec are negative or not finite"):
        call(bad, True)
    # ... and with a scalar omega (dist_weights, grad_lo, grad_hi, grad_mm)
    bad = [a.copy() for a in clean]
    bad[2][L // 2], bad[4][1], bad[4][L - 1] = np.nan, np.inf, -np.inf
    with pytest.raises(BddMmaError, match=rf"error {capi.ERR_INVALID_ARGUMENT}: 1 values of grad_learned_iterations: grad_lo are not finite"):
        call(bad, False, 1)
    # a later array alone, a negative gradient is fine, a negative weight is not
    bad = [a.copy() for a in clean]
    bad[4][L - 1] = -np.inf
    with pytest.raises(BddMmaError, match=rf"error {capi.ERR_INVALID_ARGUMENT}: 1 values of grad_learned_iterations: grad_mm are not finite"):
        call(bad, True, 3)
    bad = [a.copy() for a in clean]
    bad[0][L - 1] = -0.0625
    with pytest.raises(BddMmaError, match=rf"error {capi.ERR_INVALID_ARGUMENT}: grad_learned_iterations: 1 of the dist_weights are negative or not finite"):
        call(bad, False)
    for x, y in zip(before, _state(s)):
        np.testing.assert_array_equal(np.asarray(x), np.asarray(y))
    # the two-input single-shot operators share the load
    g = on_device([pub["g_lo"], pub["g_hi"]], 1)
    out = on_device([np.zeros(s.nr_variables(), b.vt)] * 2, 0)
    s.grad_cost_perturbation(g[0], g[1], out=out)
    for x, y in zip(s.grad_cost_perturbation(pub["g_lo"], pub["g_hi"]), out):
        np.testing.assert_array_equal(x, y.cpu().numpy())
    g[1][2] = float("inf")
    with pytest.raises(BddMmaError, match=rf"error {capi.ERR_INVALID_ARGUMENT}: 1 values of grad_cost_perturbation: grad_hi are not finite"):
        s.grad_cost_perturbation(g[0], g[1], out=out)
    b.close()
