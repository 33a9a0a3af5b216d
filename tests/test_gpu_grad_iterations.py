"""GPU tests of the backward of the learned iterations (bddmma_grad_learned_iterations: kernels/graditer.hpp, solver_gi.hpp) against the NumPy
restatement tests/grad_iterations_restatement.py (itself pinned to finite differences and to the single-shot operator by
tests/test_grad_iterations_restatement.py).

Fixtures: grad_iterations_restatement.seeded_inputs on the seed tests/test_grad_iterations_restatement.py records per family and precision
(it asserts that the whole trajectory — one untracked iteration, two tracked — is decided by gaps of at least 2^10 eps(REAL) times the
BDD's largest |path cost|; a family and form of omega with no float seed is compared in double only; the
covering families use a smaller instance of their generator in float).  Tolerance of the comparison — measured: `dev` = the
largest deviation between the restatement in REAL and in the next wider type, per output; the device may differ from the wider run by
4 * dev, with a floor of 16 eps * (sum of the |incoming gradients| over the layer's BDD; for grad_mm over the layer's variable; for a scalar
omega over everything).  Each case prints its figures (pytest -s)."""
import ctypes as C

import numpy as np
import pytest
import torch

from bdd_amd import capi
from bdd_amd.capi import BddMmaError
from bdd_amd.solver import bdd_hip_lbfgs, bdd_hip_parallel_mma
from grad_iterations_restatement import grad_iterations_of, seeded_inputs
from test_grad_iterations_restatement import SEEDS, instance_of
from test_gpu_sum_marginals import FAMILIES, assert_chained

pytestmark = pytest.mark.gpu

WIDER = {np.float32: np.float64, np.float64: np.longdouble}
UNTRACKED, TRACKED = 1, 2
CASES = [(f, p, ov) for f in sorted(FAMILIES) for p in ("double", "float") for ov in (False, True) if SEEDS[f][p][ov] is not None]


def _to_public(x, perm):
    out = np.empty_like(x)
    out[perm] = x
    return out


def _setup(family, precision, omega_vec=False, **extra):
    """(solver holding the seeded costs and no deferred differences, restatement, inputs in BDD-major order, perm, inputs in public order
    and the solver's type)"""
    col, costs = instance_of(family, precision)
    s = bdd_hip_parallel_mma(col, costs, precision=precision, **FAMILIES[family][1], **extra)
    assert_chained(family, col, s)
    m = grad_iterations_of(col, precision)
    x = seeded_inputs(m, SEEDS[family][precision][omega_vec] or SEEDS[family]["double"][omega_vec])   # (compared with the restatement: tie-free seeds only, CASES)
    perm = s.bdd_major_order()
    pub = {k: _to_public(v, perm).astype(s.value_type) for k, v in x.items()}
    s.set_solver_costs(pub["lo"], pub["hi"], np.zeros(m.n_layers))
    return s, m, x, perm, pub


def _call(s, pub, omega_vec, after=UNTRACKED, n=TRACKED, num_caches=1):
    return s.grad_iterations(pub["alpha"], pub["g_lo"], pub["g_hi"], pub["g_mm"], 0.5, after, n, num_caches, omega_vec=pub["omega_vec"] if omega_vec else None)


def _reference(m, x, omega, R):
    lo, hi, d = m.iterate(x["lo"], x["hi"], np.zeros(m.n_layers), x["alpha"], omega, UNTRACKED, R)
    return m.grad_iterations(lo, hi, d, x["alpha"], omega, TRACKED, x["g_lo"], x["g_hi"], x["g_mm"], R)


@pytest.mark.parametrize("family,precision,omega_vec", CASES)
def test_against_restatement(family, precision, omega_vec):
    s, m, x, perm, pub = _setup(family, precision, omega_vec)
    dt = s.value_type
    eps = np.finfo(dt).eps
    omega = x["omega_vec"] if omega_vec else 0.5
    a, b = _reference(m, x, omega, dt), _reference(m, x, omega, WIDER[dt])
    got = _call(s, pub, omega_vec)
    inc = np.abs(x["g_lo"]) + np.abs(x["g_hi"]) + np.abs(x["g_mm"])
    bdd = m.layer_bdd()
    per_bdd = 16 * eps * np.bincount(bdd, weights=inc, minlength=m.n_bdds)[bdd]
    per_var = 16 * eps * np.bincount(m.layer_var, weights=inc, minlength=m.n_vars)[m.layer_var]
    floors = [per_bdd, per_bdd, per_var, per_bdd, per_bdd if omega_vec else np.array([16 * eps * inc.sum()])]
    for i, nm in enumerate(("grad_lo", "grad_hi", "grad_mm", "grad_dist_weights", "grad_omega")):
        assert got[i].dtype == dt
        ref, low = b[i], a[i]
        g = got[i][perm] if got[i].size == m.n_layers else got[i]
        if nm == "grad_omega" and not omega_vec:   # the scalar: the per-layer values summed in double
            ref, low = np.array([ref.sum()]), np.array([low.astype(np.float64).sum()])
        dev = float(np.max(np.abs(low.astype(np.longdouble) - ref)))
        err = np.abs(g.astype(np.longdouble) - ref).astype(np.float64)
        tol = np.maximum(4 * dev, floors[i])
        print(f"{family} {precision} {'omega_vec' if omega_vec else 'omega'} {nm}: restatement {np.dtype(dt).name} vs wider {dev:.3e}; device vs wider "
              f"{err.max():.3e}; allowed (min over entries) {tol.min():.3e}; largest |value| {float(np.abs(ref).max()):.3e}")
        assert np.all(err <= tol), (nm, float(err.max()), float(tol.min()))
    s.close()


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_directional_derivative_on_the_device_in_double(family):
    """<a, lo_out> + <b, hi_out> + <c, mm_out> after two of the device's own learned iterations is linear in (lo, hi, d) near a tie-free
    state: its difference over a step eps along a direction |dir| <= 1 equals eps <gradient, dir> up to rounding.  eps = the smallest gap
    of the restatement's trajectory / (8 * layers of the longest BDD).  Rounding: outputs of magnitude M carry ~4 eps(double) M each; allowed
    64 eps(double) * sum |incoming| * M / eps, which must itself stay below a hundredth of the derivative.  (The weights and omega enter bilinearly; their gradients are compared with the restatement,
    which tests/test_grad_iterations_restatement.py pins with central differences.)"""
    s, m, x, perm, pub = _setup(family, "double", deterministic=True)
    L = m.n_layers
    s.learned_iterations(pub["alpha"], UNTRACKED, 0.5, improvement_slope=0.0)
    lo, hi, d = (v.copy() for v in s.get_solver_costs())
    to_major = lambda v: np.asarray(v, np.float64)[perm]
    gap, mag = m.trajectory_gap(to_major(lo), to_major(hi), to_major(d), x["alpha"], 0.5, TRACKED, x["g_lo"], x["g_hi"], x["g_mm"], np.longdouble)
    eps = float(gap.min()) / (8 * int(np.max(np.diff(m.bdd_layer_ptr))))
    s.set_solver_costs(lo, hi, d)
    g = _call(s, pub, False, after=0)

    def loss(lo_, hi_, d_):
        s.set_solver_costs(lo_, hi_, d_)
        s.learned_iterations(pub["alpha"], TRACKED, 0.5, improvement_slope=0.0)
        o = s.get_solver_costs()
        return float(np.dot(pub["g_lo"], o[0]) + np.dot(pub["g_hi"], o[1]) + np.dot(pub["g_mm"], o[2]))

    rng = np.random.Generator(np.random.PCG64(12))
    dirs = [rng.uniform(-1, 1, L) for _ in range(3)]
    base = loss(lo, hi, d)
    lhs = (loss(lo + eps * dirs[0], hi + eps * dirs[1], d + eps * dirs[2]) - base) / eps
    rhs = float(sum(np.dot(g[i], dirs[i]) for i in range(3)))
    inc = float(np.abs(pub["g_lo"]).sum() + np.abs(pub["g_hi"]).sum() + np.abs(pub["g_mm"]).sum())
    allowed = 64 * np.finfo(np.float64).eps * inc * float(mag.max()) / eps
    print(f"{family}: eps {eps:.3e}, finite differences {lhs:.12g}, J^T g . dir {rhs:.12g}, allowed {allowed:.3e}")
    assert eps > 1e-8 and allowed <= 1e-2 * abs(rhs)   # the comparison says something: the allowance is far below the derivative itself
    assert abs(lhs - rhs) <= allowed
    s.close()


def _state(s):
    return list(s.get_solver_costs()) + [s.get_delta(), s.lower_bound()]


def _assert_same_state(before, s):
    for x, y in zip(before, _state(s)):
        np.testing.assert_array_equal(np.asarray(x), np.asarray(y))


@pytest.mark.parametrize("precision", ["double", "float"])
@pytest.mark.parametrize("family", ["cover10_w128", "mixed", "huge", "chained_general"])
def test_state_contract_and_errors(family, precision):
    s, m, x, perm, pub = _setup(family, precision, deterministic=True)
    L = s.nr_layers()
    s.iterations(2)   # a state with deferred differences and a delta
    before = _state(s)
    n = 3
    want = _call(s, pub, False, 1, n, 1)
    _assert_same_state(before, s)
    for nc in (0, 1, 2, n, 1):
        got = _call(s, pub, False, 1, n, nc)
        for a, b in zip(want, got):
            np.testing.assert_array_equal(a, b, err_msg=f"num_caches {nc}")
        _assert_same_state(before, s)
    want_v = _call(s, pub, True, 1, n, 2)
    s.sum_marginals_cuda(False, True)   # overwrites the stored potentials
    for a, b in zip(want_v, _call(s, pub, True, 1, n, n)):
        np.testing.assert_array_equal(a, b)
    _assert_same_state(before, s)
    # no tracked iteration: nothing runs, the in-out arrays are unchanged, the outputs are zero
    z = _call(s, pub, False, 2, 0, 1)
    for a, b in zip(z[:3], (pub["g_lo"], pub["g_hi"], pub["g_mm"])):
        np.testing.assert_array_equal(a, b)
    assert not z[3].any() and not z[4].any() and z[4].size == 1
    _assert_same_state(before, s)
    # refusals, the state untouched
    P = lambda a: a.ctypes.data_as(C.c_void_p)
    bad_g, bad_w, bad_ov = pub["g_hi"].copy(), pub["alpha"].copy(), pub["omega_vec"].copy()
    bad_g[L // 2], bad_w[1], bad_ov[L - 1] = np.nan, -0.5, np.inf
    o = [np.zeros(L, s.value_type) for _ in range(2)]
    fn = s._L.bddmma_grad_learned_iterations
    ok = lambda: [pub["g_lo"].copy(), pub["g_hi"].copy(), pub["g_mm"].copy()]
    for call in (lambda g: fn(s._h, None, 0, 0.5, None, 0, P(g[0]), P(g[1]), P(g[2]), P(o[0]), P(o[1]), 1, 2, 1, 0),
                 lambda g: fn(s._h, P(pub["alpha"]), 0, 0.5, None, 0, P(g[0]), None, P(g[2]), P(o[0]), P(o[1]), 1, 2, 1, 0),
                 lambda g: fn(s._h, P(pub["alpha"]), 0, 0.5, None, 0, P(g[0]), P(g[1]), P(g[2]), P(o[0]), None, 1, 2, 1, 0),
                 lambda g: fn(s._h, P(pub["alpha"]), 0, 0.5, None, 0, P(g[0]), P(bad_g), P(g[2]), P(o[0]), P(o[1]), 1, 2, 1, 0),
                 lambda g: fn(s._h, P(bad_w), 0, 0.5, None, 0, P(g[0]), P(g[1]), P(g[2]), P(o[0]), P(o[1]), 1, 2, 1, 0),
                 lambda g: fn(s._h, P(pub["alpha"]), 0, -0.5, None, 0, P(g[0]), P(g[1]), P(g[2]), P(o[0]), P(o[1]), 1, 2, 1, 0),
                 lambda g: fn(s._h, P(pub["alpha"]), 0, float("nan"), None, 0, P(g[0]), P(g[1]), P(g[2]), P(o[0]), P(o[1]), 1, 2, 1, 0),
                 lambda g: fn(s._h, P(pub["alpha"]), 0, 0.5, P(bad_ov), 0, P(g[0]), P(g[1]), P(g[2]), P(o[0]), P(o[1]), 1, 2, 1, 0)):
        assert call(ok()) == capi.ERR_INVALID_ARGUMENT
        _assert_same_state(before, s)
    w = bdd_hip_lbfgs(s)
    with pytest.raises(BddMmaError, match=f"error {capi.ERR_STATE}:"):
        _call(s, pub, False)
    w.close()
    _assert_same_state(before, s)
    s.close()


@pytest.mark.parametrize("precision", ["double", "float"])
@pytest.mark.parametrize("family", ["mixed", "huge", "split_bdds", "chained_general"])
def test_device_buffers_and_memory(family, precision):
    s, m, x, perm, pub = _setup(family, precision, deterministic=True)
    L = s.nr_layers()
    n = 3
    bytes0 = s.device_bytes()
    for omega_vec in (False, True):
        host = _call(s, pub, omega_vec, 1, n, n)
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda")
        g = [dev(pub[k]) for k in ("g_lo", "g_hi", "g_mm")]
        out = (torch.zeros(L, dtype=g[0].dtype, device="cuda"), torch.zeros(L if omega_vec else 1, dtype=g[0].dtype, device="cuda"))
        s.grad_iterations(dev(pub["alpha"]), g[0], g[1], g[2], 0.5, 1, n, n, omega_vec=dev(pub["omega_vec"]) if omega_vec else None, out=out)
        for a, b in zip(host, g + list(out)):
            np.testing.assert_array_equal(a, b.cpu().numpy())
    bytes1 = s.device_bytes()
    assert bytes1 >= bytes0 + n * 3 * L * np.dtype(s.value_type).itemsize   # at least the caches
    _call(s, pub, False, 1, n, n)
    assert s.device_bytes() == bytes1
    bad = pub["g_mm"].copy()
    bad[0] = np.inf
    with pytest.raises(BddMmaError, match=f"error {capi.ERR_INVALID_ARGUMENT}:"):
        s.grad_iterations(dev(pub["alpha"]), g[0], g[1], dev(bad), 0.5, 1, n, n, out=out)
    s.close()


@pytest.mark.parametrize("precision", ["double", "float"])
def test_chain_from_the_bound_to_the_cost_perturbation(precision):
    """grad_lower_bound_per_bdd -> grad_iterations -> grad_cost_perturbation: the gradient of the sum of the per-BDD bounds after three
    learned iterations with respect to a perturbation of the variables' costs"""
    make, opts = FAMILIES["mixed"]
    col, costs = make()
    s = bdd_hip_parallel_mma(col, costs, precision=precision, **opts)
    L = s.nr_layers()
    w = s.get_isotropic_dist_weights()
    start = [v.copy() for v in s.get_solver_costs()]
    s.learned_iterations(w, 3, 0.5, improvement_slope=0.0)
    g_lo, g_hi = s.grad_lower_bound_per_bdd(np.ones(s.nr_bdds(), s.value_type))
    s.set_solver_costs(*start)
    g_lo, g_hi, g_mm, g_w, g_om = s.grad_iterations(w, g_lo, g_hi, np.zeros(L, s.value_type), 0.5, 0, 3, 2)
    p_lo, p_hi = s.grad_cost_perturbation(g_lo, g_hi)
    for v in (g_lo, g_hi, g_mm, g_w, g_om, p_lo, p_hi):
        assert np.all(np.isfinite(v))
    assert np.abs(g_lo).sum() + np.abs(g_hi).sum() > 0
    s.close()
