"""GPU tests of the single-shot backward operators (bddmma_grad_min_marginal_diff: kernels/gradmm.hpp; bddmma_grad_lower_bound_per_bdd,
bddmma_grad_distribute_delta, bddmma_grad_cost_perturbation: kernels/elementwise.hpp) against the NumPy restatement tests/grad_restatement.py
(itself pinned to brute-force enumeration and finite differences by tests/test_grad_restatement.py).

Comparison with the restatement, on tie-free states only: the costs are seeded Gaussian lo / hi values set through set_solver_costs, the
incoming gradient g is seeded Gaussian, and tests/test_grad_restatement.py asserts for every (family, seed) used here that every deciding
minimum has a gap of at least 2^10 eps(REAL) times the BDD's largest |path cost|.  Then the device and the restatement take the same
arg-mins and every output is the same signed sum of g values, summed in another order.  Tolerance — measured, not chosen: `dev` = the
largest deviation between the restatement in REAL and in the next wider type; the device may differ from the wider run by 4 * dev, with a
floor of 16 eps * (sum of |g| over the layer's BDD).  Each case prints its figures (pytest -s).  Where ties are frequent (after
iterations, integer costs) only antisymmetry and determinism are checked."""
import numpy as np
import pytest
import torch

from bdd_amd import capi
from bdd_amd.capi import BddMmaError
from bdd_amd.solver import bdd_hip_lbfgs, bdd_hip_parallel_mma
from grad_restatement import Gradients, gradients_of, tie_free_state
from test_grad_restatement import SEEDS
from test_gpu_sum_marginals import FAMILIES, assert_chained

pytestmark = pytest.mark.gpu

WIDER = {np.float32: np.float64, np.float64: np.longdouble}


def _tie_free_solver(family, precision, **extra):
    """(solver with the family's seeded tie-free costs, the restatement holding the same costs, g in BDD-major order, perm)"""
    make, opts = FAMILIES[family]
    col, costs = make()
    s = bdd_hip_parallel_mma(col, costs, precision=precision, **opts, **extra)
    assert_chained(family, col, s)
    m = gradients_of(col, precision)
    lo, hi, g = tie_free_state(m, SEEDS[family])
    perm = s.bdd_major_order()
    m.lo, m.hi = lo.copy(), hi.copy()   # float64 holding float32 values: the same numbers in both precisions
    s.set_solver_costs(_to_public(lo, perm), _to_public(hi, perm), np.zeros(m.n_layers))
    return s, m, g, perm


def _to_public(x, perm):
    out = np.empty_like(x)
    out[perm] = x
    return out


def _floor(m, g, dt):
    """16 eps * sum of |g| over the layer's BDD, per layer (BDD-major)"""
    bdd = m.layer_bdd()
    return 16 * np.finfo(dt).eps * np.bincount(bdd, weights=np.abs(g), minlength=m.n_bdds)[bdd]


@pytest.mark.parametrize("precision", ["double", "float"])
@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_against_restatement(family, precision):
    s, m, g, perm = _tie_free_solver(family, precision)
    dt = s.value_type
    a = m.grad_mm_diff(g, dt)
    b = m.grad_mm_diff(g, WIDER[dt])
    dev = max(float(np.max(np.abs(x.astype(np.longdouble) - y))) for x, y in zip(a, b))
    floor = _floor(m, g, dt)
    tol = np.maximum(4 * dev, floor)
    lo, hi = s.grad_all_min_marginal_differences(_to_public(g, perm))
    assert lo.dtype == dt and hi.dtype == dt
    for got, ref, nm in ((lo[perm], b[0], "grad_lo"), (hi[perm], b[1], "grad_hi")):
        err = np.abs(got.astype(np.longdouble) - ref).astype(np.float64)
        print(f"{family} {precision} {nm}: restatement {np.dtype(dt).name} vs wider {dev:.3e}; device vs wider {err.max():.3e}; "
              f"allowed (min over layers) {tol.min():.3e}; largest |value| {float(np.abs(ref).max()):.3e}")
        assert np.all(err <= tol), (nm, float(err.max()), float(tol.min()))
    # antisymmetry: quasi-reduced BDDs, every path takes one arc per layer
    assert np.all(np.abs(lo[perm].astype(np.float64) + hi[perm].astype(np.float64)) <= floor)
    # bit for bit from call to call
    lo2, hi2 = s.grad_all_min_marginal_differences(_to_public(g, perm))
    np.testing.assert_array_equal(lo, lo2)
    np.testing.assert_array_equal(hi, hi2)
    s.close()


@pytest.mark.parametrize("precision", ["double", "float"])
@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_antisymmetry_and_determinism_where_ties_are_frequent(family, precision):
    make, opts = FAMILIES[family]
    col, costs = make()
    s = bdd_hip_parallel_mma(col, costs, precision=precision, **opts)
    assert_chained(family, col, s)
    m = gradients_of(col, precision)
    perm = s.bdd_major_order()
    g = np.random.Generator(np.random.PCG64(9)).normal(0, 1, s.nr_layers()).astype(s.value_type)
    floor = _to_public(_floor(m, g[perm].astype(np.float64), s.value_type), perm)
    for state in ("initial", "after 5 iterations", "integer costs"):
        if state == "after 5 iterations":
            s.iterations(5)
        if state == "integer costs":
            rng = np.random.Generator(np.random.PCG64(10))
            s.set_solver_costs(rng.integers(-2, 3, s.nr_layers()), rng.integers(-2, 3, s.nr_layers()), np.zeros(s.nr_layers()))
        lo, hi = s.grad_all_min_marginal_differences(g)
        lo2, hi2 = s.grad_all_min_marginal_differences(g)
        np.testing.assert_array_equal(lo, lo2, err_msg=state)
        np.testing.assert_array_equal(hi, hi2, err_msg=state)
        assert np.all(np.isfinite(lo)) and np.all(np.isfinite(hi))
        asym = np.abs(lo.astype(np.float64) + hi.astype(np.float64))
        print(f"{family} {precision} {state}: max |grad_lo + grad_hi| {asym.max():.3e}, floor (min) {floor.min():.3e}")
        assert np.all(asym <= floor), state
    s.close()


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_directional_derivative_on_the_device_in_double(family):
    """<g, mm_diff(c + eps d) - mm_diff(c)> = eps <J^T g, d> with the device's own min_marginal_diff; eps an eighth of the smallest decision
    gap (restatement, all-ones gradient: every layer's paths) over the layers of the longest BDD, |d| <= 1, so no arg-min moves.  Rounding: the
    differences of mm_diff values of magnitude M carry ~4 eps(double) M each; allowed 64 eps(double) * sum |g| M / eps."""
    s, m, g, perm = _tie_free_solver(family, "double")
    gap, mag = m.decision_gap(np.ones(m.n_layers), np.longdouble)
    k = int(np.max(np.diff(m.bdd_layer_ptr)))
    eps = float(gap.min()) / (8 * k)
    gp = _to_public(g, perm)
    lo, hi = s.grad_all_min_marginal_differences(gp)
    base = s.min_marginal_diff().astype(np.float64)
    fin = np.isfinite(base)
    rng = np.random.Generator(np.random.PCG64(12))
    d_lo, d_hi = rng.uniform(-1, 1, m.n_layers), rng.uniform(-1, 1, m.n_layers)
    c_lo, c_hi, c_mm = s.get_solver_costs()
    s.set_solver_costs(c_lo + eps * d_lo, c_hi + eps * d_hi, c_mm)
    moved = s.min_marginal_diff().astype(np.float64)
    lhs = float(np.dot(gp[fin], moved[fin] - base[fin])) / eps
    rhs = float(np.dot(lo, d_lo) + np.dot(hi, d_hi))
    allowed = 64 * np.finfo(np.float64).eps * float(np.abs(gp).sum()) * float(mag.max()) / eps
    print(f"{family}: eps {eps:.3e}, finite differences {lhs:.12g}, J^T g . d {rhs:.12g}, allowed {allowed:.3e}")
    assert abs(lhs - rhs) <= allowed
    s.close()


def _state(s):
    return [s.lower_bound()] + list(s.get_solver_costs()) + [s.get_delta()]


def _assert_same_state(before, s):
    for x, y in zip(before, _state(s)):
        np.testing.assert_array_equal(np.asarray(x), np.asarray(y))


@pytest.mark.parametrize("precision", ["double", "float"])
@pytest.mark.parametrize("family", ["cover10_w128", "mixed", "huge", "chained_general"])
def test_state_contract_and_errors(family, precision):
    s, m, g, perm = _tie_free_solver(family, precision, deterministic=True)
    L, B = s.nr_layers(), s.nr_bdds()
    s.iterations(3)
    mm = np.random.Generator(np.random.PCG64(2)).normal(0, 1, L)
    lo0, hi0, _ = s.get_solver_costs()
    s.set_solver_costs(lo0, hi0, mm)
    s.distribute_delta()   # the deferred differences grad_distribute_delta refers to
    s.iterations(2)
    before = _state(s)
    gp = _to_public(g, perm).astype(s.value_type)
    glb = np.random.Generator(np.random.PCG64(3)).normal(0, 1, B).astype(s.value_type)
    r = s.grad_all_min_marginal_differences(gp)
    _assert_same_state(before, s)
    s.grad_lower_bound_per_bdd(glb)
    _assert_same_state(before, s)
    s.grad_smooth_lower_bound_per_bdd(glb)
    _assert_same_state(before, s)
    s.grad_distribute_delta(r[0], r[1])
    _assert_same_state(before, s)
    s.grad_cost_perturbation(r[0], r[1])
    _assert_same_state(before, s)
    # directly after sum-marginals (which overwrite the stored potentials): the same result
    s.sum_marginals_cuda(False, True)
    r2 = s.grad_all_min_marginal_differences(gp)
    np.testing.assert_array_equal(r[0], r2[0])
    np.testing.assert_array_equal(r[1], r2[1])
    # errors: null pointers and non-finite incoming gradients, state untouched
    bad = gp.copy()
    bad[L // 2] = np.nan
    badb = glb.copy()
    badb[0] = np.inf
    P = lambda a: a.ctypes.data_as(__import__("ctypes").c_void_p)
    out0, out1 = np.zeros(L, s.value_type), np.zeros(L, s.value_type)
    for call in (lambda: s._L.bddmma_grad_min_marginal_diff(s._h, None, P(out0), P(out1), 0),
                 lambda: s._L.bddmma_grad_min_marginal_diff(s._h, P(gp), None, P(out1), 0),
                 lambda: s._L.bddmma_grad_min_marginal_diff(s._h, P(bad), P(out0), P(out1), 0),
                 lambda: s._L.bddmma_grad_lower_bound_per_bdd(s._h, None, P(out0), P(out1), 0, 0),
                 lambda: s._L.bddmma_grad_lower_bound_per_bdd(s._h, P(badb), P(out0), P(out1), 1, 0),
                 lambda: s._L.bddmma_grad_distribute_delta(s._h, P(bad), P(gp), P(out0), 0),
                 lambda: s._L.bddmma_grad_distribute_delta(s._h, P(gp), P(gp), None, 0),
                 lambda: s._L.bddmma_grad_cost_perturbation(s._h, P(gp), P(bad), P(out0), P(out1), 0),
                 lambda: s._L.bddmma_grad_cost_perturbation(s._h, P(gp), P(gp), P(out0), None, 0)):
        assert call() == capi.ERR_INVALID_ARGUMENT
        _assert_same_state(before, s)
    s.close()


@pytest.mark.parametrize("precision", ["double", "float"])
def test_with_lbfgs_wrapper_attached(precision):
    s, m, g, perm = _tie_free_solver("cover10_w128", precision, deterministic=True)
    gp = _to_public(g, perm)
    want = s.grad_all_min_marginal_differences(gp)
    w = bdd_hip_lbfgs(s)
    got = s.grad_all_min_marginal_differences(gp)
    np.testing.assert_array_equal(want[0], got[0])
    np.testing.assert_array_equal(want[1], got[1])
    w.iteration()
    lo, hi = s.grad_all_min_marginal_differences(gp)
    assert np.all(np.isfinite(lo)) and np.all(np.isfinite(hi))
    w.close()
    s.close()


@pytest.mark.parametrize("precision", ["double", "float"])
@pytest.mark.parametrize("family", ["cover10_w128", "mixed", "huge", "split_bdds", "chained_general"])
def test_small_operators(family, precision):
    """the three elementwise operators against their one-line NumPy formulas, host and device buffers"""
    make, opts = FAMILIES[family]
    col, costs = make()
    s = bdd_hip_parallel_mma(col, costs, precision=precision, **opts)
    assert_chained(family, col, s)
    dt = s.value_type
    tdt = torch.float64 if precision == "double" else torch.float32
    L, V, B = s.nr_layers(), s.nr_variables(), s.nr_bdds()
    rng = np.random.Generator(np.random.PCG64(5))
    g_lo, g_hi, glb = rng.normal(0, 1, L).astype(dt), rng.normal(0, 1, L).astype(dt), rng.normal(0, 1, B).astype(dt)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda")
    new = lambda n: torch.zeros(n, dtype=tdt, device="cuda")
    s.iterations(3)
    bdd = np.asarray(s.get_bdd_index())
    var = np.asarray(s.get_primal_variable_index())
    one = dt(1)
    # lower bound: hard and smooth
    for smooth in (False, True):
        x = s.smooth_solution_per_bdd() if smooth else s.bdds_solution_vec().astype(dt)
        fn = s.grad_smooth_lower_bound_per_bdd if smooth else s.grad_lower_bound_per_bdd
        lo, hi = fn(glb)
        np.testing.assert_array_equal(hi, x * glb[bdd])
        np.testing.assert_array_equal(lo, (one - x) * glb[bdd])
        out = fn(dev(glb), out=(new(L), new(L)))
        np.testing.assert_array_equal(out[0].cpu().numpy(), lo)
        np.testing.assert_array_equal(out[1].cpu().numpy(), hi)
    # distribute_delta: refused before the first distribute_delta, then by the sign of what it applied
    with pytest.raises(BddMmaError, match=f"error {capi.ERR_STATE}:"):
        s.grad_distribute_delta(g_lo, g_hi)
    _, _, mm = s.get_solver_costs()
    mm = mm.copy()
    mm[::7] = 0
    lo0, hi0, _ = s.get_solver_costs()
    s.set_solver_costs(lo0, hi0, mm)
    s.distribute_delta()
    s.iterations(1)   # the deferred differences move on; the call refers to what distribute_delta applied
    want = Gradients.grad_distribute_delta(g_lo, g_hi, mm)
    np.testing.assert_array_equal(s.grad_distribute_delta(g_lo, g_hi), want)
    np.testing.assert_array_equal(s.grad_distribute_delta(dev(g_lo), dev(g_hi), out=new(L)).cpu().numpy(), want)
    # cost perturbation: per variable the sum over its layers (by BDD) / nr_bdds, within the rounding of a sum of n terms
    p_lo, p_hi = s.grad_cost_perturbation(g_lo, g_hi)
    n = np.bincount(var, minlength=V)
    for got, gin in ((p_lo, g_lo), (p_hi, g_hi)):
        ref = np.bincount(var, weights=gin.astype(np.float64), minlength=V) / np.maximum(n, 1)
        mag = np.bincount(var, weights=np.abs(gin).astype(np.float64), minlength=V) / np.maximum(n, 1)
        assert np.all(np.abs(got - ref) <= (n + 2) * np.finfo(dt).eps * mag)
    out = s.grad_cost_perturbation(dev(g_lo), dev(g_hi), out=(new(V), new(V)))
    np.testing.assert_array_equal(out[0].cpu().numpy(), p_lo)
    np.testing.assert_array_equal(out[1].cpu().numpy(), p_hi)
    # the min-marginal gradient into device buffers: the host result bit for bit
    lo, hi = s.grad_all_min_marginal_differences(g_lo)
    out = s.grad_all_min_marginal_differences(dev(g_lo), out=(new(L), new(L)))
    np.testing.assert_array_equal(out[0].cpu().numpy(), lo)
    np.testing.assert_array_equal(out[1].cpu().numpy(), hi)
    # a NaN in a device buffer is refused as well
    bad = g_lo.copy()
    bad[3] = np.nan
    with pytest.raises(BddMmaError, match=f"error {capi.ERR_INVALID_ARGUMENT}:"):
        s.grad_all_min_marginal_differences(dev(bad), out=(new(L), new(L)))
    s.close()


def test_scratch_is_counted():
    make, opts = FAMILIES["huge"]
    col, costs = make()
    s = bdd_hip_parallel_mma(col, costs, precision="double", **opts)
    s.sum_marginals_cuda(False, True)   # the parent tables are the sum-marginals'
    before = s._L.bddmma_device_bytes(s._h)
    s.grad_all_min_marginal_differences(np.ones(s.nr_layers()))
    after = s._L.bddmma_device_bytes(s._h)
    assert after >= before + (8 + 8) * s.nr_layers()   # the gradient's copy and the arg-min slots, and the huge packs' scratch
    s.grad_all_min_marginal_differences(np.ones(s.nr_layers()))
    assert s._L.bddmma_device_bytes(s._h) == after
    s.close()
