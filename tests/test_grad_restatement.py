"""CPU tests that pin the yardstick of the gradient tests: the NumPy restatement (tests/grad_restatement.py) of the four single-shot backward
operators against brute-force enumeration and against finite differences of the forward operators, the tie-free condition of every
(family, seed) that tests/test_gpu_gradients.py compares with the restatement, and that the entry points exist in every layer."""
import inspect

import numpy as np
import pytest

from bdd_amd import capi
from bdd_amd.solver import bdd_hip_parallel_mma
from grad_restatement import GAP_FACTOR, Gradients, gradients_of, tie_free, tie_free_state
from test_capi_symbols import declared_symbols
from test_gpu_sum_marginals import FAMILIES
from test_sum_marginals_restatement import INSTANCES

# the seed of tie_free_state() per family of test_gpu_sum_marginals.FAMILIES: the first one for which tie_free() holds in both precisions
# (decided by the restatement alone; test_gpu_fixtures_are_tie_free asserts it)
SEEDS = {"assignment8": 1, "cover10_w64": 5, "cover10_w128": 5, "cover10_w256": 5, "huge": 1, "knapsack_w64": 1, "mixed": 2, "split_bdds": 1,
         "staggered_rows": 1, "wide2": 2,
         # the chained families: the instance, and so the seed, of staggered_rows, knapsack_w64 and mixed; chained_general: seed 1 is not tie-free in float
         "chained_rows": 1, "chained_knapsack": 1, "chained_wide": 2, "chained_wide2": 2, "chained_general": 2}


def _model(name, seed=7):
    col, _ = INSTANCES[name]()
    m = gradients_of(col, "double")
    rng = np.random.Generator(np.random.PCG64(seed))
    m.lo[:], m.hi[:] = rng.normal(0, 1, m.n_layers), rng.normal(0, 1, m.n_layers)
    return m, rng


@pytest.mark.parametrize("name", sorted(INSTANCES))
def test_grad_mm_diff_against_brute_force(name):
    """integer g: every output is an exact sum of a few g values on both sides, so equality is exact as long as both take the same
    minimum-cost paths — Gaussian costs in float64 make those unique (the decision gap is asserted positive)"""
    m, rng = _model(name)
    g = rng.integers(-8, 9, m.n_layers).astype(np.float64)
    gap, _ = m.decision_gap(g, np.float64)
    assert np.all(gap > 1e-9)
    lo, hi = m.grad_mm_diff(g, np.float64)
    for b in range(m.n_bdds):
        l0, l1 = m.bdd_layer_ptr[b], m.bdd_layer_ptr[b + 1]
        want_lo, want_hi = m.brute_force_grad(b, g)
        np.testing.assert_array_equal(lo[l0:l1], want_lo, err_msg=f"bdd {b} lo")
        np.testing.assert_array_equal(hi[l0:l1], want_hi, err_msg=f"bdd {b} hi")
    # quasi-reduced BDDs: every path takes one arc per layer
    np.testing.assert_array_equal(lo + hi, 0 * lo)


@pytest.mark.parametrize("name", sorted(INSTANCES))
def test_grad_mm_diff_against_finite_differences(name):
    """with tie-free costs mm_diff is linear in a neighbourhood: <g, mm_diff(c + eps d) - mm_diff(c)> = eps <J^T g, d> up to rounding.
    eps is an eighth of the smallest decision gap divided by the number of layers of the longest BDD, |d| <= 1: no path's cost moves by
    more than a quarter of a gap.  Rounding: mm_diff values are O(10), so differences carry ~1e-15 absolute error, divided by eps."""
    m, rng = _model(name)
    g = rng.normal(0, 1, m.n_layers)
    ones = np.ones(m.n_layers)
    gap, _ = m.decision_gap(ones, np.float64)
    k = int(np.max(np.diff(m.bdd_layer_ptr)))
    eps = float(gap.min()) / (8 * k)
    assert eps > 1e-7
    lo, hi = m.grad_mm_diff(g, np.float64)
    base = m.mm_diff(np.float64)
    fin = np.isfinite(base)
    for _ in range(3):
        d_lo, d_hi = rng.uniform(-1, 1, m.n_layers), rng.uniform(-1, 1, m.n_layers)
        m2 = Gradients.__new__(Gradients)
        m2.__dict__.update(m.__dict__)
        m2.lo, m2.hi = m.lo + eps * d_lo, m.hi + eps * d_hi
        moved = m2.mm_diff(np.float64)
        lhs = float(np.dot(g[fin], moved[fin] - base[fin])) / eps
        rhs = float(np.dot(lo, d_lo) + np.dot(hi, d_hi))
        assert abs(lhs - rhs) <= 1e-12 * m.n_layers * 50 / eps, (lhs, rhs, eps)


@pytest.mark.parametrize("name", sorted(INSTANCES))
def test_grad_lower_bound_hard(name):
    """x of the restatement's arg-min path equals the enumeration's, the formula, and the directional derivative of sum_b glb[b] lb[b]"""
    m, rng = _model(name)
    glb = rng.normal(0, 1, m.n_bdds)
    m.backward_run()
    x = np.asarray(m.bdds_solution(), np.float64)
    for b in range(m.n_bdds):
        xb, cost = m.brute_force_solution(b)
        np.testing.assert_array_equal(x[m.bdd_layer_ptr[b]:m.bdd_layer_ptr[b + 1]], xb)
        assert abs(cost - float(m.lower_bound_per_bdd()[b])) <= 1e-12 * max(1.0, abs(cost))
    lo, hi = m.grad_lower_bound(glb, x)
    np.testing.assert_array_equal(lo + hi, glb[m.layer_bdd()])
    eps = 1e-7
    d_lo, d_hi = rng.uniform(-1, 1, m.n_layers), rng.uniform(-1, 1, m.n_layers)
    base = np.asarray(m.lower_bound_per_bdd(), np.float64).copy()
    m.lo, m.hi = m.lo + eps * d_lo, m.hi + eps * d_hi
    m.backward_run()
    moved = np.asarray(m.lower_bound_per_bdd(), np.float64)
    assert abs(float(np.dot(glb, moved - base)) / eps - float(np.dot(lo, d_lo) + np.dot(hi, d_hi))) <= 1e-6


@pytest.mark.parametrize("name", sorted(INSTANCES))
def test_grad_lower_bound_smooth(name):
    """x = the smooth solution is the gradient of -log sum over paths exp(-cost) = -logaddexp(sm_lo, sm_hi) (any layer of the BDD): central
    differences of step 1e-5 carry a truncation error ~1e-10 and a rounding error ~1e-16 / 1e-5"""
    m, rng = _model(name)
    glb = rng.normal(0, 1, m.n_bdds)
    first = np.asarray(m.bdd_layer_ptr[:-1])

    def smooth_lb(lo, hi):
        m2 = Gradients.__new__(Gradients)
        m2.__dict__.update(m.__dict__)
        m2.lo, m2.hi = lo, hi
        sm_lo, sm_hi = m2.log_sum_marginals(np.float64)
        return -np.logaddexp(sm_lo, sm_hi)[first]

    x = Gradients.smooth_solution(*m.log_sum_marginals(np.float64))
    lo, hi = m.grad_lower_bound(glb, x)
    eps = 1e-5
    d_lo, d_hi = rng.uniform(-1, 1, m.n_layers), rng.uniform(-1, 1, m.n_layers)
    diff = (smooth_lb(m.lo + eps * d_lo, m.hi + eps * d_hi) - smooth_lb(m.lo - eps * d_lo, m.hi - eps * d_hi)) / (2 * eps)
    assert abs(float(np.dot(glb, diff)) - float(np.dot(lo, d_lo) + np.dot(hi, d_hi))) <= 1e-7 * m.n_bdds


def test_grad_distribute_delta_formula_and_finite_differences():
    rng = np.random.Generator(np.random.PCG64(3))
    n = 200
    mm = rng.normal(0, 1, n)
    mm[:5] = 0.0   # not > 0: the lo side
    g_lo, g_hi = rng.normal(0, 1, n), rng.normal(0, 1, n)
    out = Gradients.grad_distribute_delta(g_lo, g_hi, mm)
    np.testing.assert_array_equal(out[mm > 0], g_hi[mm > 0])
    np.testing.assert_array_equal(out[~(mm > 0)], -g_lo[~(mm > 0)])

    def forward(mm):   # distribute_deffered_mm_diff_func: hi += m where m > 0, else lo -= m
        return np.where(mm > 0, 0.0, -mm), np.where(mm > 0, mm, 0.0)

    eps, d = 1e-6, rng.uniform(-1, 1, n)
    away = np.abs(mm) > 2 * eps   # the sign of the moved value is the sign of mm
    a, b = forward(mm), forward(mm + eps * d)
    lhs = (np.dot(g_lo[away], (b[0] - a[0])[away]) + np.dot(g_hi[away], (b[1] - a[1])[away])) / eps
    assert abs(lhs - np.dot(out[away], d[away])) <= 1e-8


@pytest.mark.parametrize("name", sorted(INSTANCES))
def test_grad_cost_perturbation_is_the_adjoint_of_update_costs(name):
    """update_costs adds pert[var(l)] / nr_bdds(var(l)) to layer l: <g, A p> = <A^T g, p>, and per variable the brute-force mean"""
    m, rng = _model(name)
    g_lo, g_hi = rng.normal(0, 1, m.n_layers), rng.normal(0, 1, m.n_layers)
    out_lo, out_hi = m.grad_cost_perturbation(g_lo, g_hi)
    for v in range(m.n_vars):
        ls = np.flatnonzero(m.layer_var == v)
        assert abs(out_lo[v] - g_lo[ls].sum() / max(len(ls), 1)) <= 1e-14 * max(len(ls), 1)
        assert abs(out_hi[v] - g_hi[ls].sum() / max(len(ls), 1)) <= 1e-14 * max(len(ls), 1)
    p = rng.normal(0, 1, m.n_vars)
    m.hi[:] = 0
    m.update_costs_hi(p)
    assert abs(float(np.dot(g_hi, m.hi)) - float(np.dot(out_hi, p))) <= 1e-12 * m.n_layers


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_gpu_fixtures_are_tie_free(family):
    """the condition under which tests/test_gpu_gradients.py compares the device with the restatement: in the type wider than the solver's,
    every minimum that decides where a non-zero gradient goes is decided by at least 2^10 eps(REAL) times the BDD's largest |path cost|, so
    the device (whose potentials differ from the restatement's by a few eps of that magnitude) takes the same arg-mins.  Minima that no
    gradient passes through decide nothing and are not counted."""
    make, _ = FAMILIES[family]
    col, _ = make()
    m = gradients_of(col, "double")
    m.lo[:], m.hi[:], g = tie_free_state(m, SEEDS[family])
    for dt in (np.float32, np.float64):
        ok, ratio = tie_free(m, g, dt)
        print(f"{family} seed {SEEDS[family]} {np.dtype(dt).name}: smallest gap / (eps * largest |path cost|) = {ratio:.3g}, required {GAP_FACTOR:.0f}")
        assert ok, (family, np.dtype(dt).name, ratio)


def test_gradient_entry_points_are_declared_exported_and_bound():
    for name, nargs in (("bddmma_grad_min_marginal_diff", 5), ("bddmma_grad_lower_bound_per_bdd", 6), ("bddmma_grad_distribute_delta", 5),
                        ("bddmma_grad_cost_perturbation", 6)):
        assert name in declared_symbols()
        assert name in capi.SIGNATURES
        assert len(capi.SIGNATURES[name][1]) == nargs
        assert hasattr(capi.lib(), name)


def test_python_methods_exist():
    for name, first in (("grad_all_min_marginal_differences", ["grad_mm"]), ("grad_lower_bound_per_bdd", ["grad_lb_per_bdd"]),
                        ("grad_smooth_lower_bound_per_bdd", ["grad_lb_per_bdd"]), ("grad_distribute_delta", ["grad_lo", "grad_hi"]),
                        ("grad_cost_perturbation", ["grad_lo", "grad_hi"])):
        p = inspect.signature(getattr(bdd_hip_parallel_mma, name)).parameters
        assert list(p)[1:] == first + ["out"] and p["out"].default is None
