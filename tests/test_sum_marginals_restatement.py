"""CPU tests that pin the yardstick of the sum-marginal tests: the NumPy restatement (tests/sum_marginals_restatement.py) against brute-force
enumeration of every assignment of every BDD, against the closed forms of the reference's own test (test/test_bdd_cuda_sum_marginals.cpp),
and that the C-ABI entry points bddmma_sum_marginals / bddmma_smooth_solution and the Python methods exist.  The GPU side:
tests/test_gpu_sum_marginals.py."""
import inspect

import numpy as np
import pytest

from bdd_amd import capi, to_bdd_collection
from bdd_amd.instances import GRID_3X3, mrf_ilp
from bdd_amd.solver import bdd_hip_parallel_mma
from sum_marginals_restatement import TWO_SIMPLEX_CLOSED_FORMS, assignment8, cover10, general_rows, knapsack_rows, restatement_of, two_simplex
from test_capi_symbols import declared_symbols


def _cover10_small():
    return cover10(seed=5, V=60, rows=40)


def _mrf3x3():
    ilp = mrf_ilp(**GRID_3X3)
    return to_bdd_collection(ilp), np.asarray(ilp.objective, np.float64)


INSTANCES = {"cover10": _cover10_small, "assignment8": assignment8, "knapsack_rows": knapsack_rows, "mrf3x3": _mrf3x3, "general_rows": general_rows}


@pytest.mark.parametrize("name", sorted(INSTANCES))
def test_restatement_against_brute_force(name):
    """both sides are float64 sums of at most 2^19 positive terms (general_rows; worst-case rounding 2^19 * 1.1e-16 = 6e-11): rtol 1e-10"""
    col, costs = INSTANCES[name]()
    m = restatement_of(col, costs, "double")
    sm_lo, sm_hi = m.log_sum_marginals(np.float64)
    for b in range(m.n_bdds):
        l0, l1 = m.bdd_layer_ptr[b], m.bdd_layer_ptr[b + 1]
        p_lo, p_hi = m.brute_force(b)
        np.testing.assert_allclose(np.exp(sm_lo[l0:l1]), p_lo, rtol=1e-10, atol=0, err_msg=f"bdd {b} lo")
        np.testing.assert_allclose(np.exp(sm_hi[l0:l1]), p_hi, rtol=1e-10, atol=0, err_msg=f"bdd {b} hi")
        assert np.all(np.isneginf(sm_lo[l0:l1]) == (p_lo == 0)) and np.all(np.isneginf(sm_hi[l0:l1]) == (p_hi == 0))


@pytest.mark.parametrize("log_probs", [False, True])
def test_restatement_two_simplex_closed_forms(log_probs):
    """the reference's own check, at its own 1e-5, through this repository's .lp reader"""
    col, costs = two_simplex()
    m = restatement_of(col, costs, "double")
    assert m.n_layers == 6 and list(np.bincount(m.layer_var)) == [1] * 6
    sm_lo, sm_hi = m.log_sum_marginals()
    if not log_probs:
        sm_lo, sm_hi = np.exp(sm_lo), np.exp(sm_hi)
    for l in range(6):
        want = TWO_SIMPLEX_CLOSED_FORMS[m.layer_var[l]]
        got = (np.exp(sm_lo[l]), np.exp(sm_hi[l])) if log_probs else (sm_lo[l], sm_hi[l])
        assert abs(got[0] - want[0]) <= 1e-5 and abs(got[1] - want[1]) <= 1e-5, (l, got, want)


def test_path_counts_are_the_marginals_at_cost_zero():
    col, costs = knapsack_rows()
    m = restatement_of(col, 0 * costs, "double")
    sm_lo, sm_hi = m.log_sum_marginals()
    n_lo, n_hi = m.path_counts()
    np.testing.assert_allclose(np.exp(sm_lo), n_lo, rtol=1e-12)
    np.testing.assert_allclose(np.exp(sm_hi), n_hi, rtol=1e-12)


def test_smooth_solution_formula():
    sm_lo = np.array([0.0, -np.inf, -3.0, -np.inf, 500.0])
    sm_hi = np.array([0.0, 2.0, -np.inf, -np.inf, 498.0])
    from sum_marginals_restatement import SumMarginals
    np.testing.assert_allclose(SumMarginals.smooth_solution(sm_lo, sm_hi), [0.5, 1.0, 0.0, 0.5, np.exp(-2) / (1 + np.exp(-2))], rtol=1e-15)


def test_sum_marginal_entry_points_are_declared_exported_and_bound():
    for name, nargs in (("bddmma_sum_marginals", 7), ("bddmma_smooth_solution", 3)):
        assert name in declared_symbols()
        assert name in capi.SIGNATURES
        assert len(capi.SIGNATURES[name][1]) == nargs
        assert hasattr(capi.lib(), name)


def test_python_methods_exist():
    p = inspect.signature(bdd_hip_parallel_mma.sum_marginals_cuda).parameters
    assert list(p)[1:] == ["get_sorted", "get_log_probs", "out"]
    assert p["get_sorted"].default is True and p["get_log_probs"].default is True and p["out"].default is None
    assert inspect.signature(bdd_hip_parallel_mma.sum_marginals).parameters["get_log_probs"].default is True
    assert inspect.signature(bdd_hip_parallel_mma.smooth_solution_per_bdd).parameters["out"].default is None
