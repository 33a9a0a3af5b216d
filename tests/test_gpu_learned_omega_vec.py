"""Learned MMA iterations with one omega per layer (bdd_hip_parallel_mma.learned_iterations(..., omega_vec);
include/bdd_mma.h: bddmma_learned_iterations_omega_vec) on the MI355X: a constant vector against the scalar call bit for bit in every sweep
family, random vectors against the NumPy restatement (tests/learned_omega_restatement.py), zero omega, the reparametrisation, the history and
the stopping rule, device input and the argument errors."""
import ctypes as C
import zlib

import numpy as np
import pytest

from bdd_amd import capi
from bdd_amd.capi import BddMmaError
from bdd_amd.instances import random_set_cover, random_set_cover_mt
from bdd_amd.solver import bdd_hip_lbfgs, bdd_hip_parallel_mma
from learned_omega_restatement import LearnedOmegaMma
from test_gpu_learned_mma import FAMILIES, ISO_TOL, NOFUSE, REF_TOL, _assert_close, _cover10, _dirichlet_weights, _same_state, assert_chained
from util import GOLDEN, load_golden, pad_costs

pytestmark = pytest.mark.gpu

OV_FAMILIES = dict(FAMILIES)
OV_FAMILIES.update({
    # forced non-temporal instantiations (variant_flags bit 20) of the first and second generation, 4 and 8 waves per workgroup
    "narrow2_nt": (_cover10, dict(pack_width=128, waves_per_block=4, resident_sweeps=1, deterministic=True, variant_flags=0x40000 | 0x100000),
                   "streaming2"),
    "narrow_gen1_nt": (_cover10, dict(pack_width=128, waves_per_block=8, resident_sweeps=1, deterministic=True,
                                      variant_flags=0x41000 | 0x100000), "streaming1"),
    # 64-bit staging addresses (variant_flags bit 14)
    "narrow3_big": (_cover10, dict(pack_width=128, waves_per_block=4, resident_sweeps=1, variant_flags=0x2000 | 0x4000), "streaming3"),
    "narrow2_big": (_cover10, dict(pack_width=128, waves_per_block=4, resident_sweeps=1, variant_flags=0x2000 | 0x40000 | 0x4000), "streaming2"),
    "narrow_gen1_nt_big": (_cover10, dict(pack_width=128, waves_per_block=8, resident_sweeps=1, deterministic=True,
                                          variant_flags=0x41000 | 0x100000 | 0x4000), "streaming1"),
})
NT_FAMILIES = ("narrow2_nt", "narrow_gen1_nt", "narrow_gen1_nt_big")
# Two solvers agree bit for bit only where the exchange's summation order is fixed: the LDS-atomic exchange adds a variable's differences in
# whatever order the atomics land, which shows in the last bit in double.  So the sweep families run with the deterministic exchange (their
# sweeps are what omega_vec changes); the exchange variants keep their own, and the one that is the LDS-atomic reduction is compared at
# ISO_TOL in double.
EXCHANGE_OPTS = ("deterministic", "exchange_by_variable", "vars_per_bin")
ATOMIC_EXCHANGE = ("reduce_lds_128k",)


def _bit_equal(a, b, what=""):
    for x, y, nm in zip(a.get_solver_costs(), b.get_solver_costs(), ("lo", "hi", "deferred mm")):
        np.testing.assert_array_equal(x, y, err_msg=f"{what} {nm}")
    np.testing.assert_array_equal(a.get_delta(), b.get_delta(), err_msg=f"{what} delta")
    assert a.lower_bound() == b.lower_bound(), what


def _constant_vs_scalar(col, costs, precision, opts, kind=None, nt=False, exact=True):
    if not any(k in opts for k in EXCHANGE_OPTS):
        opts = dict(opts, deterministic=True)
    a = bdd_hip_parallel_mma(col, costs, precision=precision, **opts)
    b = bdd_hip_parallel_mma(col, costs, precision=precision, **opts)
    if kind is not None:
        assert a.solve_sweep_kind() == kind, a.solve_sweep_kind()
    if nt:
        assert a.nontemporal_loads()
    rng = np.random.Generator(np.random.PCG64(zlib.crc32(repr(sorted(opts.items())).encode())))
    w = _dirichlet_weights(a, rng, a.value_type, normalised=False)
    vec = np.full(a.nr_layers(), 0.5, a.value_type)
    for n in (1, 3):
        assert a.learned_iterations(w, n, 0.9, improvement_slope=0.0, omega_vec=vec) == n   # the scalar is ignored
        assert b.learned_iterations(w, n, 0.5, improvement_slope=0.0) == n
        if exact:
            _bit_equal(a, b, f"after {n}")
        else:
            _same_state(a, b, precision, ISO_TOL)
    return a


@pytest.mark.parametrize("precision", ["double", "float"])
@pytest.mark.parametrize("family", list(OV_FAMILIES))
def test_constant_omega_vec_equals_scalar_bit_for_bit(family, precision):
    make, opts, kind = OV_FAMILIES[family]
    col, costs = make()
    assert_chained(family, col, opts)
    a = _constant_vs_scalar(col, costs, precision, opts, kind, nt=family in NT_FAMILIES and (precision == "double" or "gen1" in family),
                            exact=not (family in ATOMIC_EXCHANGE and precision == "double"))
    if family == "wide2":
        assert a.solve_sweep_kind() != "mixed"
    if "variant_flags" in opts and opts["variant_flags"] & NOFUSE:
        assert not a.fused_small()


def _omega_with_zeros(rng, n, dtype):
    """random omega in [0, 1] per layer with about 30 % exact zeros: a lane that reads another layer's omega shows as a deferred difference
    that is not 0 on a layer whose omega is 0, or as a mismatch against the restatement"""
    vec = rng.uniform(0.0, 1.0, n).astype(dtype)
    vec[rng.random(n) < 0.3] = 0
    return vec


def _zero_omega_layers_have_zero_mm(s, vec, what):
    _, _, mm = s.get_solver_costs()
    zero = vec == 0
    assert np.all(mm[zero] == 0), (what, int(np.count_nonzero(mm[zero])))
    assert np.count_nonzero(mm[~zero]) > 0.9 * np.count_nonzero(~zero), what


def test_constant_omega_vec_narrow3_nontemporal_headline_size():
    """double beyond the caches' reach: the third generation's non-temporal instantiation (10.5 M nodes, the benchmark's shape); then one
    iteration with random omega and zeros (too large for the restatement: the zero layers check the per-layer addressing)"""
    col, costs = random_set_cover_mt(1_000_000, 500_000, 10, seed=12345)
    a = _constant_vs_scalar(col, costs, "double", {}, "streaming3", nt=True)
    vec = _omega_with_zeros(np.random.Generator(np.random.PCG64(31)), a.nr_layers(), a.value_type)
    assert a.learned_iterations(a.get_isotropic_dist_weights(), 1, improvement_slope=0.0, omega_vec=vec) == 1
    _zero_omega_layers_have_zero_mm(a, vec, "headline")


@pytest.mark.parametrize("precision", ["double", "float"])
@pytest.mark.parametrize("family", list(OV_FAMILIES))
def test_random_omega_vec_in_every_family_vs_restatement(family, precision):
    """each family computes the address of a layer's omega its own way: random omega (with exact zeros) against the restatement"""
    make, opts, kind = OV_FAMILIES[family]
    col, costs = make()
    assert_chained(family, col, opts)
    s = bdd_hip_parallel_mma(col, None, precision=precision, **opts)
    if kind is not None:
        assert s.solve_sweep_kind() == kind, s.solve_sweep_kind()
    if family in NT_FAMILIES and (precision == "double" or "gen1" in family):
        assert s.nontemporal_loads()
    if family == "wide2":
        assert s.solve_sweep_kind() != "mixed"
    costs = pad_costs(costs, s.nr_variables())
    s.update_costs([], costs)
    m = _restatement_of(col, costs, precision)
    perm = s.bdd_major_order()
    assert m.n_layers == s.nr_layers()
    rng = np.random.Generator(np.random.PCG64(zlib.crc32(f"family/{family}".encode())))
    w = _dirichlet_weights(s, rng, s.value_type, normalised=False)
    vec = _omega_with_zeros(rng, s.nr_layers(), s.value_type)
    for it in range(3):
        assert s.learned_iterations(w, 1, 0.5, improvement_slope=0.0, omega_vec=vec) == 1
        m.learned_iteration(w[perm], vec[perm])
        _compare(s, m, perm, precision, f"{family} iteration {it}")
        _zero_omega_layers_have_zero_mm(s, vec, f"{family} iteration {it}")


# ---------------------------------------------------------------- random omega against the restatement
def _restatement_of(col, costs, precision):
    m = LearnedOmegaMma(col.instr, col.delims, precision)
    m.update_costs_hi(np.asarray(costs, np.float64))
    return m


def _solver_and_restatement(name, precision):
    if name == "random_cover":
        col, costs = random_set_cover(300, 200, 6, seed=11)
    else:
        col, z = load_golden(name)
        costs = None
    s = bdd_hip_parallel_mma(col, None, precision=precision)
    if costs is None:
        costs = pad_costs(z["costs"], s.nr_variables())
    s.update_costs([], costs)
    m = _restatement_of(col, costs, precision)
    perm = s.bdd_major_order()
    assert m.n_layers == s.nr_layers()
    return s, m, perm


def _compare(s, m, perm, precision, what):
    lo, hi, mm = s.get_solver_costs()
    rel = REF_TOL[precision]
    _assert_close(lo[perm], m.lo, rel, what + " lo")
    _assert_close(hi[perm], m.hi, rel, what + " hi")
    _assert_close(mm[perm], m.mm, rel, what + " deferred mm")
    lb, ref = s.lower_bound(), m.lower_bound()
    assert abs(lb - ref) <= rel * max(1.0, abs(ref)), (what, lb, ref)


@pytest.mark.parametrize("precision", ["double", "float"])
@pytest.mark.parametrize("name", GOLDEN + ["random_cover"])
def test_random_omega_vec_vs_restatement(name, precision):
    s, m, perm = _solver_and_restatement(name, precision)
    rng = np.random.Generator(np.random.PCG64(zlib.crc32(f"omega/{name}".encode())))
    w = _dirichlet_weights(s, rng, s.value_type)
    vec = rng.uniform(0.0, 1.0, s.nr_layers()).astype(s.value_type)
    for it in range(6):
        assert s.learned_iterations(w, 1, 0.5, improvement_slope=0.0, omega_vec=vec) == 1
        m.learned_iteration(w[perm], vec[perm])
        _compare(s, m, perm, precision, f"{name} iteration {it}")


@pytest.mark.parametrize("precision", ["double", "float"])
def test_zero_omega(precision):
    col, costs = random_set_cover(2000, 1500, 8, seed=3)
    s = bdd_hip_parallel_mma(col, costs, precision=precision)
    rng = np.random.Generator(np.random.PCG64(6))
    w = _dirichlet_weights(s, rng, s.value_type)
    vec = rng.uniform(0.2, 1.0, s.nr_layers()).astype(s.value_type)
    zero = rng.random(s.nr_layers()) < 0.3
    vec[zero] = 0
    s.iterations(2)   # deferred differences that are not zero at entry
    s.learned_iterations(w, 2, 0.5, improvement_slope=0.0, omega_vec=vec)
    _, _, mm = s.get_solver_costs()
    assert np.all(mm[zero] == 0) and np.any(mm[~zero] != 0)
    # omega 0 everywhere with the isotropic weights: the passes form no new differences, so after the first pass's exchange has handed out
    # what was deferred the costs stay where that exchange put them
    t = bdd_hip_parallel_mma(col, costs, precision=precision)
    t.iterations(3)
    iso = t.get_isotropic_dist_weights()
    z = np.zeros(t.nr_layers(), t.value_type)
    t.learned_iterations(iso, 1, improvement_slope=0.0, omega_vec=z)
    lo1, hi1, mm1 = t.get_solver_costs()
    assert np.all(mm1 == 0)
    t.learned_iterations(iso, 2, improvement_slope=0.0, omega_vec=z)
    lo2, hi2, mm2 = t.get_solver_costs()
    np.testing.assert_array_equal(lo1, lo2)
    np.testing.assert_array_equal(hi1, hi2)
    assert np.all(mm2 == 0)


@pytest.mark.parametrize("precision", ["double", "float"])
def test_reparametrisation_with_omega_vec(precision):
    col, z = load_golden("matching_3x3_first_row")
    s = bdd_hip_parallel_mma(col, None, precision=precision)
    costs = pad_costs(z["costs"], s.nr_variables())
    s.update_costs([], costs)
    rng = np.random.Generator(np.random.PCG64(13))
    for _ in range(10):
        w = _dirichlet_weights(s, rng, s.value_type)
        vec = rng.uniform(0.0, 1.0, s.nr_layers()).astype(s.value_type)
        s.learned_iterations(w, 3, improvement_slope=0.0, omega_vec=vec)
        assert s.lower_bound() <= -4.0 + 1e-9     # the LP optimum of this instance (oracle KAT)
    s.distribute_delta()
    tol = 1e-9 if precision == "double" else 1e-5
    np.testing.assert_allclose(s.get_primal_objective_vector_host(), costs, rtol=tol, atol=tol * max(1.0, np.abs(costs).max()))


# ---------------------------------------------------------------- history and early stop
@pytest.mark.parametrize("precision", ["double", "float"])
@pytest.mark.parametrize("cfi,slope", [(0, 1e-3), (3, 0.0), (3, 1e-3)])
def test_history_and_early_stop_vs_restatement(precision, cfi, slope):
    col, costs = random_set_cover(120, 90, 5, seed=7)
    s = bdd_hip_parallel_mma(col, costs, precision=precision)
    m = _restatement_of(col, costs, precision)
    perm = s.bdd_major_order()
    rng = np.random.Generator(np.random.PCG64(19))
    w = _dirichlet_weights(s, rng, s.value_type)
    vec = rng.uniform(0.3, 0.7, s.nr_layers()).astype(s.value_type)
    L, B, dt = s.nr_layers(), s.nr_bdds(), s.value_type
    h = [np.full(L, 7.0, dt), np.full(B, 7.0, dt), np.full(B, 7.0, dt)]
    r = [np.full(L, 7.0, dt), np.full(B, 7.0, dt), np.full(B, 7.0, dt)]
    args = dict(improvement_slope=slope, compute_history_for_itr=cfi, history_avg_beta=0.9)
    for call in range(2):
        ran = s.learned_iterations(w, 40, sol_avg=h[0], lb_first_diff_avg=h[1], lb_second_diff_avg=h[2], omega_vec=vec, **args)
        r_sol = r[0][perm]
        ran_ref = m.iterations(w[perm], 40, vec[perm], sol_avg=r_sol, lb_first_diff_avg=r[1], lb_second_diff_avg=r[2], **args)
        r[0][perm] = r_sol
        assert ran == ran_ref, (call, ran, ran_ref)
        if slope == 0.0:
            assert ran == 40
        rel = REF_TOL[precision]
        _assert_close(h[0], r[0], rel, "sol_avg")
        lb_scale = max(1.0, float(np.abs(m.lower_bound_per_bdd()).max()))
        np.testing.assert_allclose(h[1], r[1], rtol=rel, atol=4 * rel * lb_scale, err_msg="lb_first_diff_avg")
        np.testing.assert_allclose(h[2], r[2], rtol=rel, atol=8 * rel * lb_scale, err_msg="lb_second_diff_avg")
        _compare(s, m, perm, precision, f"call {call}")


# ---------------------------------------------------------------- device input
@pytest.mark.parametrize("precision", ["double", "float"])
def test_device_omega_vec_equals_host(precision):
    import torch
    col, costs = random_set_cover(2000, 1500, 8, seed=8)
    a = bdd_hip_parallel_mma(col, costs, precision=precision, deterministic=True)   # bit for bit: a fixed exchange order (see EXCHANGE_OPTS)
    b = bdd_hip_parallel_mma(col, costs, precision=precision, deterministic=True)
    rng = np.random.Generator(np.random.PCG64(21))
    w = _dirichlet_weights(a, rng, a.value_type)
    vec = rng.uniform(0.3, 0.7, a.nr_layers()).astype(a.value_type)
    tdt = torch.float64 if a.value_type == np.float64 else torch.float32
    a.learned_iterations(w, 4, improvement_slope=0.0, omega_vec=vec)
    b.learned_iterations(torch.tensor(w, dtype=tdt, device="cuda"), 4, improvement_slope=0.0,
                         omega_vec=torch.tensor(vec, dtype=tdt, device="cuda"))
    torch.cuda.synchronize()
    _bit_equal(a, b, "device input")


# ---------------------------------------------------------------- argument errors
@pytest.mark.parametrize("precision", ["double", "float"])
def test_argument_errors_leave_the_solver_untouched(precision):
    import torch
    col, costs = random_set_cover(300, 200, 6, seed=5)
    s = bdd_hip_parallel_mma(col, costs, precision=precision, deterministic=True)   # bit for bit: a fixed exchange order (see EXCHANGE_OPTS)
    ref = bdd_hip_parallel_mma(col, costs, precision=precision, deterministic=True)
    s.iterations(2)
    ref.iterations(2)
    iso = s.get_isotropic_dist_weights()
    vec = np.full(s.nr_layers(), 0.5, s.value_type)
    other = np.float32 if s.value_type == np.float64 else np.float64
    tdt = torch.float64 if s.value_type == np.float64 else torch.float32
    bad = {
        "wrong length": (vec[:-1], "has"),
        "NaN": (np.where(np.arange(vec.size) == 3, np.nan, vec).astype(s.value_type), "not finite"),
        "infinite": (np.where(np.arange(vec.size) == 5, np.inf, vec).astype(s.value_type), "not finite"),
        "negative": (np.where(np.arange(vec.size) == 7, -0.25, vec).astype(s.value_type), "negative"),
        "dtype": (vec.astype(other), "the solver's values are"),
    }
    for what, (v, msg) in bad.items():
        with pytest.raises(BddMmaError, match=r"bdd_mma error -1: .*" + msg):
            s.learned_iterations(iso, 3, omega_vec=v)
        if what != "dtype":
            with pytest.raises(BddMmaError, match=r"bdd_mma error -1: "):
                s.learned_iterations(iso, 3, omega_vec=torch.tensor(v, dtype=tdt, device="cuda"))
    with pytest.raises(BddMmaError, match=r"bdd_mma error -1: "):
        s.learned_iterations(iso, 3, omega_vec=torch.tensor(vec, dtype=torch.float32 if tdt == torch.float64 else torch.float64, device="cuda"))
    # a null omega_vec through the C-ABI
    done = C.c_uint64(77)
    rc = s._L.bddmma_learned_iterations_omega_vec(s._h, iso.ctypes.data_as(C.c_void_p), 0, 3, None, 0, 0.0, None, None, None, 0, 0.9, 0,
                                                   C.byref(done))
    assert rc == capi.ERR_INVALID_ARGUMENT and done.value == 0
    assert b"omega_vec" in s._L.bddmma_last_error(s._h)
    _bit_equal(s, ref, "after the refused calls")
    assert s.learned_iterations(iso, 3, improvement_slope=0.0, omega_vec=vec) == 3
    assert ref.learned_iterations(iso, 3, 0.5, improvement_slope=0.0) == 3
    _bit_equal(s, ref, "after a good call")


def test_lbfgs_wrapper_attached_is_refused():
    col, costs = random_set_cover(300, 200, 6, seed=6)
    s = bdd_hip_parallel_mma(col, costs, precision="double")
    iso = s.get_isotropic_dist_weights()
    vec = np.full(s.nr_layers(), 0.5)
    lb = bdd_hip_lbfgs(s)
    with pytest.raises(BddMmaError, match=r"bdd_mma error -4: .*L-BFGS"):
        s.learned_iterations(iso, 2, omega_vec=vec)
    lb.close()
    assert s.learned_iterations(iso, 2, improvement_slope=0.0, omega_vec=vec) == 2
