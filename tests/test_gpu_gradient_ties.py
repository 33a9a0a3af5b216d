"""GPU tests of the tie rules of the gradient operators (bddmma_grad_min_marginal_diff: kernels/gradmm.hpp; bddmma_grad_learned_iterations:
kernels/graditer.hpp; the layer folds of kernels/pull.hpp) against the NumPy restatements, bit for bit, on the fixtures of
tests/exact_fixtures.py: integer costs, gradients and weights, omega in {1, 1/2}.  Every value is a dyadic rational far below 2^24 grid
steps and every sum is exact in any order (tests/test_exact_fixtures.py asserts that for each fixture used here, and that between a tenth
and all of the deciding minima are exact ties), so the device equals the restatement if and only if it takes the same arg-mins — the ones
include/bdd_mma.h publishes: lowest slot first among a layer's nodes, first in parent table order among a node's parents, lo before hi,
`>= 0` takes the hi side in the dual update and for the consumed differences.  No tolerance anywhere: every comparison is an array equality.

A mismatch reports the first differing layer (BDD-major), its BDD, both values and whether each lies on the fixture's grid: an off-grid
device value means rounding (the fixture or its headroom is at fault), an on-grid difference means another arg-min.

Not compared here: grad_iterations reduced to one min-marginal step against grad_all_min_marginal_differences on the device.  The reduction of
tests/test_grad_iterations_restatement.py reverses a pass with another omega (1/2) than the pass ran with (0, so that it moves no cost) and
reads the gradient that reached each mm (last_dmm) — neither can be asked of bddmma_grad_learned_iterations, which reverses the iterations it
ran itself and feeds the dual update back into mm.  tests/test_exact_fixtures.py::test_the_two_restatements_agree_at_ties holds the
reduction with exact equality on the tied states between the two restatements, each of which the device must equal here."""
import numpy as np
import pytest

from bdd_amd.solver import bdd_hip_parallel_mma
from exact_fixtures import (ITERATION_CASES, STATES, TRACKED, UNTRACKED, certificate, iterations_reference, model_of, on_grid, recorded_values,
                            single_shot_reference)
from test_gpu_sum_marginals import FAMILIES, assert_chained

pytestmark = pytest.mark.gpu


class _Solvers:
    """the solvers of one (family, precision): built on first use, reused across seeds, states and forms of omega"""

    def __init__(self, family, precision):
        self.family, self.precision = family, precision
        self.col, self.m = model_of(family)
        self._s = {}

    def get(self, deterministic=False):
        if deterministic not in self._s:
            self._s[deterministic] = bdd_hip_parallel_mma(self.col, None, precision=self.precision, deterministic=deterministic, **FAMILIES[self.family][1])
            assert_chained(self.family, self.col, self._s[deterministic])
        s = self._s[deterministic]
        return s, s.bdd_major_order()

    def close(self):
        for s in self._s.values():
            s.close()


# a family whose omega_vec form has no exact fixture (exact_fixtures.ITERATION_SEEDS: chained_general) runs the single-shot states and the
# scalar omega through a fixture and tests of its own
SCALAR_OMEGA_ONLY = [f for f in sorted(FAMILIES) if (f, True) not in ITERATION_CASES]


def _solvers_fixture(families):
    @pytest.fixture(scope="module", params=[(f, p) for f in families for p in ("double", "float")], ids=lambda fp: f"{fp[0]}-{fp[1]}")
    def fixture(request):
        x = _Solvers(*request.param)
        yield x
        x.close()
    return fixture


solvers = _solvers_fixture([f for f in sorted(FAMILIES) if f not in SCALAR_OMEGA_ONLY])
solvers_scalar_omega = _solvers_fixture(SCALAR_OMEGA_ONLY)


def _to_public(x, perm, dt):
    out = np.empty(len(x), dt)
    out[perm] = x
    return out


def _assert_same(got, want, what, m, q):
    """got (device, BDD-major or a single value) equals want (restatement, float64 holding exact values) bit for bit in the device's type"""
    want = np.asarray(want).astype(got.dtype)
    bad = np.flatnonzero(~((got == want) | (np.isnan(got) & np.isnan(want))))
    msg = what
    if bad.size:
        i = int(bad[0])
        where = f"layer {i} (BDD-major) of BDD {int(m.layer_bdd()[i])}" if got.size == m.n_layers else f"entry {i}"
        msg = (f"{what}: {bad.size} of {got.size} differ; first at {where}: device {got[i]!r} ({'on' if on_grid(got[i], q) else 'OFF'} the grid {q:g}), "
               f"restatement {want[i]!r} ({'on' if on_grid(want[i], q) else 'OFF'} the grid) — off the grid: rounding, the fixture or its headroom is at fault; "
               f"on the grid: another arg-min")
    np.testing.assert_array_equal(got, want, err_msg=msg)


@pytest.mark.parametrize("state", STATES)
def test_single_shot_gradient(solvers, state):
    """two integer states and the all-zero costs with g on a grid of 2^-8 (every finite minimum a tie): min_marginal_diff() first — the
    forward kernels have no tie rule, this pins the fixture on the device —, then grad_all_min_marginal_differences(g)"""
    _single_shot_gradient(solvers, state)


@pytest.mark.parametrize("state", STATES)
def test_single_shot_gradient_scalar_omega_families(solvers_scalar_omega, state):
    """test_single_shot_gradient on the families of SCALAR_OMEGA_ONLY"""
    _single_shot_gradient(solvers_scalar_omega, state)


def _single_shot_gradient(solvers, state):
    s, perm = solvers.get()
    dt, m = s.value_type, solvers.m
    ref = single_shot_reference(solvers.family, state)
    q, _ = certificate([ref[k] for k in ("lo", "hi", "g", "mm_diff", "grad_lo", "grad_hi")])
    s.set_solver_costs(_to_public(ref["lo"], perm, dt), _to_public(ref["hi"], perm, dt), np.zeros(m.n_layers, dt))
    what = f"{solvers.family} {solvers.precision} {state}"
    _assert_same(s.min_marginal_diff()[perm], ref["mm_diff"], f"{what}: min_marginal_diff", m, q)
    lo, hi = s.grad_all_min_marginal_differences(_to_public(ref["g"], perm, dt))
    assert lo.dtype == dt and hi.dtype == dt
    _assert_same(lo[perm], ref["grad_lo"], f"{what}: grad_lo", m, q)
    _assert_same(hi[perm], ref["grad_hi"], f"{what}: grad_hi", m, q)


@pytest.mark.parametrize("deterministic", [False, True], ids=["default_exchange", "deterministic"])
@pytest.mark.parametrize("omega_vec", [False, True], ids=["omega", "omega_vec"])
def test_learned_iterations_and_their_gradient(solvers, omega_vec, deterministic):
    """one untracked and two tracked iterations from the exact state with d = 0: the forward iterations first (the `mm >= 0` and `d >= 0` rules
    of the forward passes decide a fifth to three quarters of the layer-passes), then all five outputs of grad_iterations with one cache and with
    two.  Exact sums do not depend on the order of the exchange's atomics: the default exchange must match as the deterministic one does."""
    _learned_iterations_and_their_gradient(solvers, omega_vec, deterministic)


@pytest.mark.parametrize("deterministic", [False, True], ids=["default_exchange", "deterministic"])
def test_learned_iterations_and_their_gradient_scalar_omega_families(solvers_scalar_omega, deterministic):
    """test_learned_iterations_and_their_gradient with the scalar omega on the families of SCALAR_OMEGA_ONLY"""
    _learned_iterations_and_their_gradient(solvers_scalar_omega, False, deterministic)


def _learned_iterations_and_their_gradient(solvers, omega_vec, deterministic):
    s, perm = solvers.get(deterministic)
    dt, m = s.value_type, solvers.m
    ref = iterations_reference(solvers.family, omega_vec)
    x = ref["x"]
    q, _ = certificate(list(ref["grads"]) + recorded_values(ref) + list(ref["end"]))
    pub = {k: _to_public(v, perm, dt) for k, v in x.items() if isinstance(v, np.ndarray)}
    omega = dict(omega_vec=pub["omega_vec"]) if omega_vec else dict(omega=x["omega"])
    start = (pub["lo"], pub["hi"], np.zeros(m.n_layers, dt))
    what = f"{solvers.family} {solvers.precision} {'omega_vec' if omega_vec else 'omega'} {'deterministic' if deterministic else 'default exchange'}"
    s.set_solver_costs(*start)
    assert s.learned_iterations(pub["alpha"], UNTRACKED + TRACKED, improvement_slope=0.0, **omega) == UNTRACKED + TRACKED
    for got, want, nm in zip(s.get_solver_costs(), ref["end"], ("lo", "hi", "d")):
        _assert_same(got[perm], want, f"{what}: {nm} after {UNTRACKED + TRACKED} learned iterations", m, q)
    for num_caches in (1, 2):
        s.set_solver_costs(*start)
        got = s.grad_iterations(pub["alpha"], pub["g_lo"], pub["g_hi"], pub["g_mm"], track_grad_after_itr=UNTRACKED, track_grad_for_num_itr=TRACKED,
                                num_caches=num_caches, **omega)
        for g, want, nm in zip(got, ref["grads"], ("grad_lo", "grad_hi", "grad_mm", "grad_dist_weights", "grad_omega")):
            assert g.dtype == dt
            if nm == "grad_omega" and not omega_vec:   # the scalar: the per-layer values summed in double (exact: integers)
                assert g.size == 1
                _assert_same(g, np.array([want.astype(np.float64).sum()]), f"{what}, {num_caches} caches: {nm}", m, q)
            else:
                _assert_same(g[perm], want, f"{what}, {num_caches} caches: {nm}", m, q)
        for got_c, want_c, nm in zip(s.get_solver_costs(), start, ("lo", "hi", "d")):   # the state contract: the entry state bit for bit
            np.testing.assert_array_equal(got_c, want_c, err_msg=f"{what}: {nm} after grad_iterations")
