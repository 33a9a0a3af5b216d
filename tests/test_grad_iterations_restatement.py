"""CPU tests that pin the yardstick of tests/test_gpu_grad_iterations.py: the NumPy restatement of the backward of the learned iterations
(tests/grad_iterations_restatement.py) against finite differences of its own forward iterations and against the single-shot operator it
reduces to, the tie-free condition of every (family, precision, seed) the GPU tests compare with it, and that the entry point exists in
every layer."""
import inspect
import os

import numpy as np
import pytest

from bdd_amd import capi
from bdd_amd.solver import bdd_hip_parallel_mma
from grad_iterations_restatement import GAP_FACTOR, grad_iterations_of, seeded_inputs, trajectory_tie_free
from test_capi_symbols import declared_symbols
from test_gpu_sum_marginals import FAMILIES
from test_sum_marginals_restatement import INSTANCES, cover10

# Per family of test_gpu_sum_marginals.FAMILIES and precision: (seed for the scalar omega 0.5, seed for the seeded omega_vec) of seeded_inputs(),
# found by a search over 1..32 with the restatement alone: a seed whose whole trajectory (one untracked iteration, two tracked) is tie-free in
# that precision, for both forms of omega where one exists, else for the scalar alone.  None: no seed in the range — that form is compared in
# double only (staggered_rows in float: best ratios 130 / 74 of the 1024 required; mixed / wide2 with omega_vec: 564).  The covering families
# have no float seed on their 3 000 layers (nor on 300 - 1 500 layers of the same generator); in float they use a smaller instance of it,
# 240 layers (FLOAT_INSTANCE), which still spans several packs at every width.  test_gpu_fixtures_are_tie_free asserts each entry.
SEEDS = {
    "assignment8": {"double": (1, 1), "float": (1, 1)},
    "cover10_w64": {"double": (1, 1), "float": (22, 22)},
    "cover10_w128": {"double": (1, 1), "float": (22, 22)},
    "cover10_w256": {"double": (1, 1), "float": (22, 22)},
    "huge": {"double": (1, 1), "float": (13, 13)},
    "knapsack_w64": {"double": (1, 1), "float": (1, 1)},
    "mixed": {"double": (1, 1), "float": (23, None)},
    "split_bdds": {"double": (1, 1), "float": (5, 5)},
    "staggered_rows": {"double": (1, 1), "float": (None, None)},
    "wide2": {"double": (1, 1), "float": (23, None)},
    # the chained families: the instance, and so the seeds, of staggered_rows, knapsack_w64 and mixed.  chained_general: every seed in 1..32 is
    # tie-free in double; seed 1's smallest gap gives tests/test_gpu_grad_iterations.py::test_directional_derivative_on_the_device_in_double a
    # step of 7.0e-9, under the 1e-8 it requires, seed 2's gives 2.6e-8.  No float seed in 1..32 (best ratios 310 / 147 of the 1024 required)
    "chained_rows": {"double": (1, 1), "float": (None, None)},
    "chained_knapsack": {"double": (1, 1), "float": (1, 1)},
    "chained_wide": {"double": (1, 1), "float": (23, None)},
    "chained_wide2": {"double": (1, 1), "float": (23, None)},
    "chained_general": {"double": (2, 2), "float": (None, None)},
}


def _cover10_tiny():
    return cover10(seed=5, V=16, rows=24)


FLOAT_INSTANCE = {"cover10_w64": _cover10_tiny, "cover10_w128": _cover10_tiny, "cover10_w256": _cover10_tiny}


def instance_of(family, precision):
    """(collection, costs) of the family's fixture in that precision"""
    make = FLOAT_INSTANCE.get(family) if precision == "float" else None
    return (make or FAMILIES[family][0])()


def _start(name, seed, omega_vec):
    """(model, inputs, omega, the state after one untracked iteration) in float64"""
    col, _ = INSTANCES[name]()
    m = grad_iterations_of(col, "double")
    x = seeded_inputs(m, seed)
    omega = x["omega_vec"] if omega_vec else 0.5
    return m, x, omega, m.iterate(x["lo"], x["hi"], np.zeros(m.n_layers), x["alpha"], omega, 1, np.float64)


@pytest.mark.parametrize("omega_vec", [False, True], ids=["omega", "omega_vec"])
@pytest.mark.parametrize("n", [1, 2])
@pytest.mark.parametrize("name", sorted(INSTANCES))
def test_against_finite_differences(name, n, omega_vec):
    """loss = <a, lo_out> + <b, hi_out> + <c, mm_out> after n iterations.  With a tie-free trajectory it is piecewise linear in (lo, hi, d) and
    piecewise polynomial in the weights and omega.  eps = the smallest decision gap / (8 * layers of the longest BDD), |direction| <= 1, one
    group at a time; lo / hi / d by a forward difference, the weights and omega by a central one (its truncation error is O(eps^2) times
    third derivatives, which are products of a few S, m and g values: far below the rounding term).  Rounding: the outputs have magnitude
    M = the largest |path cost| printed below and carry ~1e-15 M each: allowed 1e-12 * n_layers * 50 / eps, as
    test_grad_mm_diff_against_finite_differences."""
    m, x, omega, (lo, hi, d) = _start(name, 3, omega_vec)
    gap, mag = m.trajectory_gap(lo, hi, d, x["alpha"], omega, n, x["g_lo"], x["g_hi"], x["g_mm"], np.float64)
    eps = float(gap.min()) / (8 * int(np.max(np.diff(m.bdd_layer_ptr))))
    assert eps > 1e-8
    G = m.grad_iterations(lo, hi, d, x["alpha"], omega, n, x["g_lo"], x["g_hi"], x["g_mm"], np.float64)
    om = np.broadcast_to(np.asarray(omega, np.float64), (m.n_layers,))

    def loss(args):
        o = m.iterate(*args, n, np.float64)
        return float(np.dot(x["g_lo"], o[0]) + np.dot(x["g_hi"], o[1]) + np.dot(x["g_mm"], o[2]))

    point = [lo, hi, d, x["alpha"], om]
    base = loss(point)
    allowed = 1e-12 * m.n_layers * 50 / eps
    rng = np.random.Generator(np.random.PCG64(11))
    for grp, nm in enumerate(("lo", "hi", "d", "dist_weights", "omega")):
        direction = np.ones(m.n_layers) if (nm == "omega" and not omega_vec) else rng.uniform(-1, 1, m.n_layers)
        moved = lambda sgn: [p + sgn * eps * direction if i == grp else p for i, p in enumerate(point)]
        lhs = (loss(moved(1)) - base) / eps if grp < 3 else (loss(moved(1)) - loss(moved(-1))) / (2 * eps)
        rhs = float(np.dot(G[grp], direction))
        print(f"{name} n={n} {nm}: eps {eps:.3e}, largest |path cost| {mag.max():.3g}, finite differences {lhs:.12g}, J^T g . dir {rhs:.12g}, allowed {allowed:.3e}")
        assert abs(lhs - rhs) <= allowed, (nm, lhs, rhs)


@pytest.mark.parametrize("name", sorted(INSTANCES))
def test_reduction_to_the_single_shot_operator(name):
    m, x, _, (lo, hi, d) = _start(name, 3, False)
    zero = np.zeros(m.n_layers)
    # omega = 0, weights = 0, one iteration: the costs do not move, so grad_lo / grad_hi pass through and nothing reaches d, the weights see S g
    g = m.grad_iterations(lo, hi, d, zero, 0.0, 1, x["g_lo"], x["g_hi"], x["g_mm"], np.float64)
    np.testing.assert_array_equal(g[0], x["g_lo"])
    np.testing.assert_array_equal(g[1], x["g_hi"])
    np.testing.assert_array_equal(g[2], zero)
    # grad_mm the only input, one pass: take a pass that moves no cost (omega = 0, weights 0), so that its F and T are the plain potentials
    # of (lo, hi), and reverse it with multiplier omega' = 0.5.  The gradient that reaches mm[l] is dmm[l] = grad_mm[l] + the dual update's
    # feedback (last_dmm); the cost gradient — what the reverse sweep leaves plus what its gF carries on through F — is the single-shot
    # operator Gradients.grad_mm_diff applied to omega' * dmm: the same seeds at the same arg-mins, summed in another order.
    R = np.float64
    m._setup(R)
    om0, om = np.zeros(m.n_layers), np.full(m.n_layers, 0.5)
    f = m.forward_pass_rec(lo, hi, d, zero, om0, R)
    b = m.backward_pass_rec(f["post"][0], f["post"][1], f["mm"], f["F"], zero, om0, R)
    np.testing.assert_array_equal(b["post"][0], lo)
    np.testing.assert_array_equal(b["post"][1], hi)
    o_lo, o_hi, gd, gF, _, _ = m.reverse_backward_pass(b, zero, zero, x["g_mm"], np.zeros(m.n_nodes), zero, om, R)
    dmm = m.last_dmm.copy()
    o_lo, o_hi, _, gT, _, _ = m.reverse_forward_pass(f, o_lo, o_hi, zero, gF, zero, om0, R)
    assert not gT.any() and not gd.any()
    m.lo, m.hi = lo.copy(), hi.copy()
    s_lo, s_hi = m.grad_mm_diff(0.5 * dmm, R)
    scale = 1e-13 * float(np.abs(dmm).sum())
    assert np.max(np.abs(o_lo - s_lo)) <= scale and np.max(np.abs(o_hi - s_hi)) <= scale


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_gpu_fixtures_are_tie_free(family):
    """the condition under which tests/test_gpu_grad_iterations.py compares the device with the restatement: in the type wider than the
    solver's, every decision of the trajectory that routes a non-zero gradient — arg-min over a layer's nodes, over a node's arcs, over a
    node's parents, the sign of mm and of a consumed difference — is decided by at least 2^10 eps(REAL) times the BDD's largest |path cost|.
    Double must hold for every family, float for at least six of them (test_enough_float_fixtures)."""
    assert None not in SEEDS[family]["double"]
    for prec, dt in (("double", np.float64), ("float", np.float32)):
        col, _ = instance_of(family, prec)
        m = grad_iterations_of(col, "double")
        for form, seed in zip(("omega", "omega_vec"), SEEDS[family][prec]):
            if seed is None:
                print(f"{family} {prec} {form}: no seed in 1..32, compared in double only")
                continue
            x = seeded_inputs(m, seed)
            ok, ratio = trajectory_tie_free(m, x, 0.5 if form == "omega" else x["omega_vec"], dt)
            print(f"{family} seed {seed} {prec} {form}: smallest gap / (eps * largest |path cost|) = {ratio:.3g}, required {GAP_FACTOR:.0f}")
            assert ok, (family, prec, form, ratio)


def test_enough_float_fixtures():
    assert set(SEEDS) == set(FAMILIES)
    assert sum(1 for f in SEEDS if SEEDS[f]["float"][0] is not None) >= 6


def test_entry_point_is_declared_exported_and_bound():
    name = "bddmma_grad_learned_iterations"
    assert name in declared_symbols()
    assert name in capi.SIGNATURES
    assert len(capi.SIGNATURES[name][1]) == 15
    assert hasattr(capi.lib(), name)


def test_python_method_and_pybind_method_exist():
    p = inspect.signature(bdd_hip_parallel_mma.grad_iterations).parameters
    assert list(p)[1:] == ["dist_weights", "grad_lo", "grad_hi", "grad_mm", "omega", "track_grad_after_itr", "track_grad_for_num_itr", "num_caches",
                           "omega_vec", "out"]
    assert p["out"].default is None and p["omega_vec"].default is None
    from bdd_amd import bdd_solver_py
    assert hasattr(bdd_solver_py.bdd_hip_parallel_mma, "grad_iterations")
    hpp = open(os.path.join(os.path.dirname(capi.__file__), "csrc", "bdd_hip_parallel_mma.hpp")).read()
    assert "void grad_iterations(" in hpp and "bddmma_grad_learned_iterations(" in hpp
