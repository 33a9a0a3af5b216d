"""The forward solve sweep that keeps the gathered child potentials of every hop in registers (kernels/narrow4.hpp: k_fwd_narrow4 with
REBUILD_T) against its twin, the same solver with variant_flags bit 21 (both potentials through memory): every result bit for bit.
Deterministic exchange, float, packs of 128 slots.  What the kernel's walk changed is its lower end — hop 0 is a gather-only step of the
upward walk — so the instances are packs of exactly 1, 2 and 3 hops, and rows of 2-10 with packs of different hop counts in one
workgroup and a last workgroup with missing packs (tests/onchip_forward_shapes.py; tests/test_onchip_forward_layout.py shows on the CPU
that each of them lands on these kernels).  The same change lets the forward form fit 12 hops: rows of 11, 12, 10 and 12 mixed run the
12-hop pair, rows of 13 the 16-hop backward kernel behind k_fwd_narrow3 (onchip_hops())."""
import numpy as np
import pytest

from bdd_amd.solver import bdd_hip_parallel_mma
from onchip_forward_shapes import CAPACITY, PACK_FILL, rows
from oracle.oracle import Oracle

pytestmark = pytest.mark.gpu

KEEP_IN_MEMORY = 0x200000   # variant_flags bit 21
T_ON_CHIP = 0x400000        # variant_flags bit 22: k_fwd_narrow4<1, 1> (T rebuilt, F stored) with k_bwd_narrow4<0, 0>
TOL = dict(abs=2e-4, rel=1e-5)   # float, as tests/test_gpu_onchip_sweeps.py::test_iteration_vs_oracle


def pair(shape, wpb, part=0):
    col, costs = rows(shape)
    opts = dict(precision="float", pack_width=128, waves_per_block=wpb, resident_sweeps=1, deterministic=True, pack_fill=PACK_FILL.get(shape, 0))
    s = bdd_hip_parallel_mma(col, costs, variant_flags=0x2000 | part, **opts)
    t = bdd_hip_parallel_mma(col, costs, variant_flags=0x2000 | KEEP_IN_MEMORY, **opts)
    assert s.potentials_on_chip() and not t.potentials_on_chip()
    assert s.onchip_hops() == CAPACITY[shape] and t.onchip_hops() == 0
    assert s.solve_sweep_kind() == "streaming3" and t.solve_sweep_kind() == "streaming3"
    return s, t


def assert_same_state(s, t):
    for a, b in zip(s.get_solver_costs(), t.get_solver_costs()):
        np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(s.get_delta(), t.get_delta())
    assert s.lower_bound() == t.lower_bound()
    np.testing.assert_array_equal(s.lower_bound_per_bdd(), t.lower_bound_per_bdd())


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("wpb", [4, 8])
@pytest.mark.parametrize("shape", ["hop1", "hop2", "hop3", "rows2_10"])
def test_iterations_equal_the_twin_bit_for_bit(shape, wpb, n):
    s, t = pair(shape, wpb)
    s.iterations(n); t.iterations(n)
    assert_same_state(s, t)


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("wpb", [4, 8])
@pytest.mark.parametrize("shape", ["rows11", "rows12", "rows10_12", "rows13"])
def test_longer_packs_equal_the_twin_bit_for_bit(shape, wpb, n):
    """The 12-hop capacity of the pair with both potentials on chip (rows of 11 and 12, rows of 10 and 12 side by side), and rows of 13, which
    stay with the 16-hop backward kernel behind k_fwd_narrow3: pair() asserts onchip_hops() == 12 / 16."""
    s, t = pair(shape, wpb)
    s.iterations(n); t.iterations(n)
    assert_same_state(s, t)


@pytest.mark.parametrize("wpb", [4, 8])
def test_rows_of_12_vs_oracle(wpb):
    s, _ = pair("rows12", wpb)
    col, costs = rows("rows12")
    o = Oracle(col, costs, "float")
    for _ in range(6):
        s.iteration(); o.iteration()
        a, b = s.lower_bound(), o.lower_bound()
        assert abs(a - b) <= TOL["abs"] * 10 + TOL["rel"] * abs(b), (a, b)


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("shape", ["hop2", "hop3", "rows2_10"])
def test_forward_sweep_that_also_stores_F_equals_the_twin(shape, n):
    """variant_flags bit 22, four packs per workgroup: the instantiation <1, 1> changes with <1, 0>."""
    s, t = pair(shape, 4, part=T_ON_CHIP)
    s.iterations(n); t.iterations(n)
    assert_same_state(s, t)


@pytest.mark.parametrize("what", ["min_marginals", "lower_bound_per_bdd"])
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("shape", ["hop1", "rows2_10"])
def test_getter_straight_after_iterations(shape, n, what):
    """No getter between iterations(n) and the one under test: it finds the stored potentials stale and has to bring them up itself."""
    s, t = pair(shape, 4)
    s.iterations(n); t.iterations(n)
    if what == "min_marginals":
        for a, b in zip(s.min_marginals_cuda(get_sorted=False), t.min_marginals_cuda(get_sorted=False)):
            np.testing.assert_array_equal(a, b)
    else:
        np.testing.assert_array_equal(s.lower_bound_per_bdd(), t.lower_bound_per_bdd())
    assert_same_state(s, t)
