"""The solve sweeps of iteration() that rebuild F and T on chip (kernels/narrow4.hpp: k_fwd_narrow4 / k_bwd_narrow4) against their twin,
the same solver with variant_flags bit 21 (the third generation with both potentials through memory): every result bit for bit, the state
transitions into everything that reads the stored potentials, and the oracle.  Deterministic exchange, so that "bit for bit" is a
statement about the sweeps.

The kernels serve packs that start from the resident headers: one stage group per pack, so at most 640 layers in a pack.  Packs of 16-hop
rows filled to all 128 slots hold 1 024, and 128 one-variable rows are more than the 64 layers a hop of the third generation takes; those
shapes therefore fill fewer slots per hop (pack_fill), which is what brings them under the rule the tests are about."""
import os
import tempfile

import numpy as np
import pytest

from bdd_amd import BddCollection, capi
from bdd_amd.solver import bdd_hip_parallel_mma, run_solver
from oracle.oracle import Oracle

pytestmark = pytest.mark.gpu

KEEP_IN_MEMORY = 0x200000   # variant_flags bit 21
TOL = dict(abs=2e-4, rel=1e-5)   # float, as tests/test_gpu_parity.py


def close(a, b, precision, scale=1.0):
    assert precision == "float"
    return abs(a - b) <= TOL["abs"] * max(1.0, scale) + TOL["rel"] * abs(b)


def _rows(shape):
    rng = np.random.Generator(np.random.PCG64({"cover10": 5, "mixed_short": 6, "tiny": 8, "rows16": 9, "rows10_16": 10, "rows17": 11}[shape]))
    col = BddCollection()
    V = 500
    if shape == "cover10":        # 1 500 covering rows of 10
        for _ in range(1500):
            col.add_covering(np.sort(rng.choice(V, size=10, replace=False)))
    elif shape == "mixed_short":  # 1 501 rows of 2-10: a partly filled last pack, a last workgroup with missing packs, BDDs ending at different hops
        for _ in range(1501):
            k = int(rng.integers(2, 11))
            (col.add_covering if rng.random() < 0.5 else col.add_simplex)(np.sort(rng.choice(V, size=k, replace=False)))
    elif shape == "tiny":         # 200 rows of 1-2 variables: packs shorter than any look-ahead
        for _ in range(200):
            k = int(rng.integers(1, 3))
            col.add_covering(np.sort(rng.choice(V, size=k, replace=False)))
    elif shape == "rows16":       # the 16-hop kernels
        for _ in range(600):
            col.add_covering(np.sort(rng.choice(V, size=16, replace=False)))
    elif shape == "rows10_16":    # different hop counts in one workgroup
        for i in range(900):
            (col.add_covering if i % 3 else col.add_simplex)(np.sort(rng.choice(V, size=10 if (i // 64) % 2 else 16, replace=False)))
    else:                         # rows of 17: beyond the kernels' capacity
        for _ in range(400):
            col.add_covering(np.sort(rng.choice(V, size=17, replace=False)))
    costs = rng.normal(0, 3, col.nr_variables()).round(3)
    return col, costs


_CACHE = {}


def rows(shape):
    if shape not in _CACHE:
        _CACHE[shape] = _rows(shape)
    return _CACHE[shape]


PACK_FILL = {"tiny": 64, "rows16": 76, "rows10_16": 76, "rows17": 64}


def pair(shape, wpb, expect_on_chip=True):
    col, costs = rows(shape)
    opts = dict(precision="float", pack_width=128, waves_per_block=wpb, resident_sweeps=1, deterministic=True, pack_fill=PACK_FILL.get(shape, 0))
    s = bdd_hip_parallel_mma(col, costs, variant_flags=0x2000, **opts)
    t = bdd_hip_parallel_mma(col, costs, variant_flags=0x2000 | KEEP_IN_MEMORY, **opts)
    assert s.potentials_on_chip() == expect_on_chip and not t.potentials_on_chip()
    assert s.solve_sweep_kind() == "streaming3" and t.solve_sweep_kind() == "streaming3"
    return s, t


def assert_same_state(s, t):
    for a, b in zip(s.get_solver_costs(), t.get_solver_costs()):
        np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(s.get_delta(), t.get_delta())
    assert s.lower_bound() == t.lower_bound()
    np.testing.assert_array_equal(s.lower_bound_per_bdd(), t.lower_bound_per_bdd())


@pytest.mark.parametrize("n", [1, 2, 7])
@pytest.mark.parametrize("wpb", [4, 8])
@pytest.mark.parametrize("shape", ["cover10", "mixed_short", "tiny", "rows16", "rows10_16", "rows17"])
def test_iterations_equal_the_twin_bit_for_bit(shape, wpb, n):
    s, t = pair(shape, wpb, expect_on_chip=shape != "rows17")
    s.iterations(n); t.iterations(n)
    assert_same_state(s, t)


@pytest.mark.parametrize("part", [0x400000, 0x800000])
def test_pairs_that_keep_one_potential_on_chip_equal_the_twin(part):
    """variant_flags bits 22 / 23 (4 packs per workgroup, <= 10 hops): only T / only F rebuilt on chip, the other potential through memory."""
    col, costs = rows("mixed_short")
    opts = dict(precision="float", pack_width=128, waves_per_block=4, resident_sweeps=1, deterministic=True)
    s = bdd_hip_parallel_mma(col, costs, variant_flags=0x2000 | part, **opts)
    t = bdd_hip_parallel_mma(col, costs, variant_flags=0x2000 | KEEP_IN_MEMORY, **opts)
    assert s.potentials_on_chip() and not t.potentials_on_chip()
    s.iterations(3); t.iterations(3)
    assert_same_state(s, t)
    s.iterations(2); t.iterations(2)
    assert_same_state(s, t)


@pytest.mark.parametrize("wpb", [4, 8])
@pytest.mark.parametrize("what", ["min_marginals", "explicit_mm", "learned", "solution", "set_costs", "checkpoint", "run_solver"])
def test_state_transitions_equal_the_twin(what, wpb):
    """What follows iterations(3): everything that reads d_F / d_T gets a plain sweep first, everything that changes costs drops the bound."""
    s, t = pair("mixed_short", wpb)
    s.iterations(3); t.iterations(3)
    if what == "min_marginals":
        for a, b in zip(s.min_marginals_cuda(get_sorted=False), t.min_marginals_cuda(get_sorted=False)):
            np.testing.assert_array_equal(a, b)
    elif what == "explicit_mm":
        V = s.nr_variables()
        ds, dt = np.zeros(2 * V, s.value_type), np.zeros(2 * V, s.value_type)
        for _ in range(8):
            s.forward_mm(0.5, ds); t.forward_mm(0.5, dt)
            np.testing.assert_array_equal(ds, dt)
            s.backward_mm(0.5, ds); t.backward_mm(0.5, dt)
            np.testing.assert_array_equal(ds, dt)
    elif what == "learned":
        w = s.get_isotropic_dist_weights()
        assert s.learned_iterations(w, 3, improvement_slope=0.0) == t.learned_iterations(w, 3, improvement_slope=0.0)
    elif what == "solution":
        np.testing.assert_array_equal(s.bdds_solution_vec(), t.bdds_solution_vec())
    elif what == "set_costs":
        s.set_solver_costs(*t.get_solver_costs())
        s.iterations(2); t.iterations(2)
    elif what == "checkpoint":
        with tempfile.TemporaryDirectory() as d:
            path = os.path.join(d, "s.ckpt")
            s.save(path)
            s = bdd_hip_parallel_mma.load(path)
        assert s.potentials_on_chip()
        s.iterations(2); t.iterations(2)
    else:
        rs, rt = run_solver(s, max_iter=20), run_solver(t, max_iter=20)
        assert (rs["iterations"], rs["lb_initial"], rs["lb_final"], rs["stop_reason"]) == (rt["iterations"], rt["lb_initial"], rt["lb_final"], rt["stop_reason"])
    assert_same_state(s, t)
    s.iterations(1); t.iterations(1)
    assert_same_state(s, t)


def test_bound_after_iterations_needs_no_plain_sweep():
    s, _ = pair("cover10", 4)
    s.set_profiling(True, 1)
    s.iterations(4)
    s.lower_bound()
    prof = s.get_profile()
    assert prof["launches"][capi.K_OTHER] == 0, prof
    assert prof["launches"][capi.K_FORWARD_MM] == 4 and prof["launches"][capi.K_BACKWARD_MM] == 4, prof


@pytest.mark.parametrize("wpb", [4, 8])
@pytest.mark.parametrize("shape", ["cover10", "mixed_short"])
def test_iteration_vs_oracle(shape, wpb):
    s, _ = pair(shape, wpb)
    col, costs = rows(shape)
    o = Oracle(col, costs, "float")
    for _ in range(6):
        s.iteration(); o.iteration()
        assert close(s.lower_bound(), o.lower_bound(), "float", 10)
