"""CPU tests that pin the yardstick of tests/test_gpu_dyadic_parity.py: on the fixtures of tests/dyadic_fixtures.py the double `Oracle`
is exact for ITERATIONS[shape] iterations — every recorded value finite and on a grid with two bits of headroom under the mantissa, the
float `Oracle` bit-equal to it — and the trajectory is not degenerate.  All conditions are on the reference alone; the iteration counts
are recomputed here, not trusted.  Each case prints its figures (pytest -s)."""
import numpy as np
import pytest

from dyadic_fixtures import ARRAYS, HEADROOM, ITERATIONS, LONG, MAX_ITERATIONS, SHAPES, dyadic_rows, headrooms, largest_n, reference, rows, trajectory
from oracle.oracle import Oracle

FLOORS = {False: (2, 4), True: (1, 2)}   # (float, double) iterations a shape has to allow; True: the long, wide and huge shapes
MIN_MM_SHARE = 0.25


def test_the_table_names_every_shape():
    assert sorted(ITERATIONS) == sorted(SHAPES)


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_counts(shape):
    col, costs = rows(shape)
    nb = Oracle(col, None, "double").nr_bdds_per_var()
    assert len(nb) == len(costs)
    want = {2} if SHAPES[shape] is None else set(SHAPES[shape][1])
    assert set(np.unique(nb).tolist()) == want and want <= {1, 2, 4}
    if SHAPES[shape] is not None:   # exactly counts[v % len(counts)], so no row repeats a variable
        V, counts, _ = SHAPES[shape]
        np.testing.assert_array_equal(nb, np.asarray(counts)[np.arange(V) % len(counts)])
    np.testing.assert_array_equal(costs, np.round(costs))
    assert np.abs(costs).max() <= 2
    col2, costs2 = dyadic_rows(shape)   # a function of (shape, seed) alone
    np.testing.assert_array_equal(col2.instr, col.instr)
    np.testing.assert_array_equal(costs2, costs)


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_headroom(shape):
    (n_float, n_double), seen = largest_n(shape)
    print(f"{shape}: log2(largest |value| / grid step) after 1 ... {len(seen)} iterations: {' '.join(f'{np.log2(h):.1f}' for h in seen)}; "
          f"float {n_float}, double {n_double} iterations")
    assert ITERATIONS[shape] == (n_float, n_double)
    assert n_double < MAX_ITERATIONS            # the search stopped because the headroom ran out, not at its cap
    floor = FLOORS[shape in LONG]
    assert n_float >= floor[0] and n_double >= floor[1]
    h = headrooms(shape, n_double)
    assert h[n_float - 1] <= HEADROOM["float"] and h[n_double - 1] <= HEADROOM["double"]
    assert len(seen) == n_double + 1 and seen[n_double] > HEADROOM["double"]
    assert n_float == n_double or seen[n_float] > HEADROOM["float"]


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_finite(shape):
    """no forced variable: the GPU comparison leaves out no value"""
    t = trajectory(shape)
    assert np.isfinite(t.initial["bound"]) and np.all(np.isfinite(t.initial["lb_per_bdd"]))
    for rec in reference(shape, ITERATIONS[shape][1]):
        assert np.isfinite(rec["bound"])
        for k in ARRAYS:
            assert np.all(np.isfinite(rec[k])), k


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_float_oracle_equals_double_oracle(shape):
    """the statement the GPU test makes about the kernels, made about the reference first"""
    n = ITERATIONS[shape][0]
    for it, (f, d) in enumerate(zip(reference(shape, n, "float"), reference(shape, n, "double"))):
        for k in ARRAYS:
            assert f[k].dtype == (np.float64 if k == "min_marginals" else np.float32)   # (min_marginals: the oracle's own doubles of float potentials)
            np.testing.assert_array_equal(f[k].astype(np.float64), d[k], err_msg=f"{shape}: {k} after iteration {it + 1}")
        assert f["bound"] == d["bound"]


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_not_degenerate(shape):
    n_float, n_double = ITERATIONS[shape]
    ref = reference(shape, n_double)
    bounds = [trajectory(shape).initial["bound"]] + [r["bound"] for r in ref]
    assert all(b > a for a, b in zip(bounds, bounds[1:])), bounds
    for n in (n_float, n_double):   # the last iteration of a float run and of a double run
        mm = ref[n - 1]["mm_last"]
        share = float(np.mean(mm != 0))
        print(f"{shape}: after iteration {n} mm > 0 in {int(np.sum(mm > 0))}, < 0 in {int(np.sum(mm < 0))} of {mm.size} layers ({share:.1%} non-zero)")
        assert np.any(mm > 0) and np.any(mm < 0) and share >= MIN_MM_SHARE
