"""The lane-per-BDD solve sweeps (kernels/narrow5.hpp: k_fwd_narrow5 / k_bwd_narrow5) against their twins, bit for bit — needs an MI355X.

Three solvers on one instance: the default (the walks in registers), the twin with variant_flags bit 24 (k_fwd_narrow4 / k_bwd_narrow4: the
same sweeps with the walks through LDS) and the twin with bit 21 (both potentials through memory, narrow3).  Float, packs of 128 slots, 4
and 8 packs per workgroup, the default and the deterministic exchange; the shapes of tests/onchip_forward_shapes.py (tests/test_lane_codes.py
shows on the CPU that they are lane-affine): packs of 1, 2 and 3 hops, rows of 2-10 (packs of different hop counts in one workgroup, a last
workgroup with missing packs, idle lanes), rows of 11 and 12 and of 10 and 12 mixed (the 12-hop pair).  Then the getters that find the
stored potentials stale, run_solver, a fixture that is not lane-affine (the rule has to fall back), the dyadic fixtures against the double
oracle, and blocked arcs (+inf costs).  Every case first asserts the path it is about."""
import numpy as np
import pytest

import test_gpu_dyadic_parity as dyadic
from bdd_amd.solver import bdd_hip_parallel_mma, run_solver
from lane_sweep_shapes import NO_LANE_SWEEPS, NOT_AFFINE_OPTS, not_affine_rows
from onchip_forward_shapes import CAPACITY, PACK_FILL, rows

pytestmark = pytest.mark.gpu

KEEP_IN_MEMORY = 0x200000   # variant_flags bit 21
SHAPES = ["hop1", "hop2", "hop3", "rows2_10", "rows11", "rows12", "rows10_12"]
EXCHANGES = {"atomics": dict(), "deterministic": dict(deterministic=True)}


def make(col, costs, flags, **opts):
    return bdd_hip_parallel_mma(col, costs, precision="float", variant_flags=0x2000 | flags, **opts)


def trio(shape, wpb, exchange):
    """(default, bit-24 twin, bit-21 twin), each on the path it stands for"""
    col, costs = rows(shape)
    opts = dict(pack_width=128, waves_per_block=wpb, resident_sweeps=1, pack_fill=PACK_FILL.get(shape, 0), **EXCHANGES[exchange])
    s, t, m = make(col, costs, 0, **opts), make(col, costs, NO_LANE_SWEEPS, **opts), make(col, costs, KEEP_IN_MEMORY, **opts)
    assert s.lane_sweeps() and not t.lane_sweeps() and not m.lane_sweeps()
    assert s.onchip_hops() == CAPACITY[shape] and t.onchip_hops() == CAPACITY[shape] and m.onchip_hops() == 0
    assert s.potentials_on_chip() and t.potentials_on_chip() and not m.potentials_on_chip()
    assert all(x.solve_sweep_kind() == "streaming3" for x in (s, t, m))
    assert s.nr_packs() == t.nr_packs() == m.nr_packs() and s.nr_packs() > 4        # four packs per workgroup: more than one workgroup
    return s, t, m


def assert_same_state(s, t, what=""):
    for a, b, name in zip(s.get_solver_costs(), t.get_solver_costs(), ("lo", "hi", "deferred differences")):
        np.testing.assert_array_equal(a, b, err_msg=f"{what}: {name}")
    np.testing.assert_array_equal(s.get_delta(), t.get_delta(), err_msg=f"{what}: delta")
    np.testing.assert_array_equal(s.lower_bound_per_bdd(), t.lower_bound_per_bdd(), err_msg=f"{what}: lower_bound_per_bdd")
    a, b = s.lower_bound(), t.lower_bound()
    assert a == b or (a != a and b != b), (what, a, b)      # equal as doubles (NaN at the same place counts as equal, as in the arrays)


@pytest.mark.parametrize("exchange", sorted(EXCHANGES))
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("wpb", [4, 8])
@pytest.mark.parametrize("shape", SHAPES)
def test_every_iteration_equals_both_twins(shape, wpb, n, exchange):
    s, t, m = trio(shape, wpb, exchange)
    for it in range(n):
        for x in (s, t, m):
            x.iteration()
        assert_same_state(s, t, f"iteration {it + 1}, bit-24 twin")
        assert_same_state(s, m, f"iteration {it + 1}, bit-21 twin")


@pytest.mark.parametrize("what", ["min_marginals", "lower_bound_per_bdd"])
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("wpb", [4, 8])
@pytest.mark.parametrize("shape", ["hop1", "rows2_10", "rows12"])
def test_getter_straight_after_iterations(shape, wpb, n, what):
    """No getter between iterations(n) and the one under test: it finds the stored potentials stale and has to bring them up itself."""
    s, t, m = trio(shape, wpb, "deterministic")
    for x in (s, t, m):
        x.iterations(n)
    for other in (t, m):
        if what == "min_marginals":
            for a, b in zip(s.min_marginals_cuda(get_sorted=False), other.min_marginals_cuda(get_sorted=False)):
                np.testing.assert_array_equal(a, b)
        else:
            np.testing.assert_array_equal(s.lower_bound_per_bdd(), other.lower_bound_per_bdd())
        assert_same_state(s, other)


@pytest.mark.parametrize("wpb", [4, 8])
@pytest.mark.parametrize("shape", ["rows2_10", "rows10_12"])
def test_run_solver_stops_where_the_twin_stops(shape, wpb):
    s, t, _ = trio(shape, wpb, "deterministic")
    a, b = (run_solver(x, max_iter=60, tolerance=1e-4, improvement_slope=1e-6) for x in (s, t))
    assert a["iterations"] == b["iterations"] and a["stop_reason"] == b["stop_reason"]
    assert a["lb_initial"] == b["lb_initial"] and a["lb_final"] == b["lb_final"]
    assert 1 <= a["iterations"]
    assert_same_state(s, t)


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("wpb", [4, 8])
def test_not_lane_affine_keeps_the_lds_walks(wpb, n):
    """a shorter BDD before a longer one in a pack: lane_sweeps() is 0 and the sweeps are narrow4's, equal to the bit-21 twin"""
    col, costs = not_affine_rows()
    opts = dict(waves_per_block=wpb, resident_sweeps=1, deterministic=True, **NOT_AFFINE_OPTS)
    s, m = make(col, costs, 0, **opts), make(col, costs, KEEP_IN_MEMORY, **opts)
    assert not s.lane_sweeps() and not m.lane_sweeps()
    assert s.onchip_hops() == 10 and s.potentials_on_chip() and m.onchip_hops() == 0
    assert s.nr_packs() == m.nr_packs() and s.nr_packs() > wpb
    for it in range(n):
        s.iteration(); m.iteration()
        assert_same_state(s, m, f"iteration {it + 1}")


ORACLE_FILL = {"rows11": 76, "rows2": 64}   # tests/test_gpu_dyadic_parity.py: ONCHIP_FILL


@pytest.mark.parametrize("exchange", sorted(EXCHANGES))
@pytest.mark.parametrize("wpb", [4, 8])
@pytest.mark.parametrize("shape", ["rows10", "rows2_10", "rows11", "rows2"])
def test_against_the_double_oracle(shape, wpb, exchange):
    """the dyadic fixtures at their float iteration counts: the double oracle's trajectory, cast to float, after every iteration, the
    min-marginals after the last, and once more with all iterations in one call"""
    opts = dict(pack_width=128, resident_sweeps=1, waves_per_block=wpb, variant_flags=0x2000, pack_fill=ORACLE_FILL.get(shape, 0), **EXCHANGES[exchange])
    path = dict(kind="streaming3", on_chip=True, packs=5)
    n = dyadic.n_iterations(shape, "float")
    ref = dyadic.reference(shape, n)
    what = f"{shape} wpb {wpb} {exchange}"
    s, perm = dyadic.solver(shape, "float", opts, path)
    assert s.lane_sweeps() and s.onchip_hops() == (12 if shape == "rows11" else 10)
    for it, rec in enumerate(ref):
        s.iteration()
        dyadic.check_state(s, perm, rec, "float", f"{what}, iteration {it + 1}")
    dyadic.check_min_marginals(s, perm, ref[-1], what)
    s.close()
    s, perm = dyadic.solver(shape, "float", opts, path)
    assert s.lane_sweeps()
    s.iterations(n)
    dyadic.check_min_marginals(s, perm, ref[-1], f"{what}, iterations({n})")
    dyadic.check_state(s, perm, ref[-1], "float", f"{what}, iterations({n})")
    s.close()


@pytest.mark.parametrize("wpb", [4, 8])
@pytest.mark.parametrize("shape", ["hop3", "rows2_10", "rows12"])
def test_blocked_arcs_equal_the_twin(shape, wpb):
    """lo = hi = +inf on one layer of a few BDDs (min-marginals of +inf on both sides, inf - inf inside the deferred difference): the same
    bits as the bit-24 twin, NaNs — if any — at the same places"""
    s, t, _ = trio(shape, wpb, "deterministic")
    bdd = s.get_bdd_index()
    rng = np.random.Generator(np.random.PCG64(152))
    blocked = np.array([rng.choice(np.flatnonzero(bdd == b)) for b in rng.choice(s.nr_bdds(), size=7, replace=False)])
    np.testing.assert_array_equal(bdd, t.get_bdd_index())
    for x in (s, t):
        lo, hi, mm = x.get_solver_costs()
        lo[blocked] = hi[blocked] = np.inf
        x.set_solver_costs(lo, hi, mm)
    for it in range(3):
        s.iteration(); t.iteration()
        assert_same_state(s, t, f"iteration {it + 1}")
    lo, hi, _ = s.get_solver_costs()
    assert np.isinf(lo[blocked]).all() and np.isinf(hi[blocked]).all()
