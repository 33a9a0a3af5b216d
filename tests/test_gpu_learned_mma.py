"""Learned MMA iterations (bdd_hip_parallel_mma.learned_iterations; include/bdd_mma.h: bddmma_learned_iterations) on the MI355X:
against the plain iterations with isotropic weights in every sweep family and exchange, against the NumPy restatement
(tests/learned_mma_restatement.py) with random weights, the history and the stopping rule, the state contract and the argument errors."""
import os
import tempfile
import zlib

import numpy as np
import pytest

from bdd_amd import BddCollection, to_bdd_collection
from bdd_amd.capi import BddMmaError
from bdd_amd.instances import assignment_ilp, random_set_cover, random_set_cover_mixed
from bdd_amd.solver import bdd_hip_lbfgs, bdd_hip_parallel_mma
from learned_mma_restatement import LearnedMma
from sum_marginals_restatement import knapsack_rows as _knapsack_rows
from test_gpu_sum_marginals import LAYOUT_OPTIONS, assert_chained_layout
from test_layout import Layout
from util import GOLDEN, load_golden, pad_costs

pytestmark = pytest.mark.gpu

ISO_TOL = {"double": 1e-12, "float": 1e-5}        # learned(iso) against the plain iterations
REF_TOL = {"double": 1e-9, "float": 1e-5}         # against the restatement (other summation orders in the exchange)


def _assert_close(a, b, rel, what=""):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    scale = max(1.0, float(np.abs(b).max())) if b.size else 1.0
    np.testing.assert_allclose(a, b, rtol=rel, atol=rel * scale, err_msg=what)


def _same_state(a, b, precision, tol):
    rel = tol[precision]
    la, lb = a.lower_bound(), b.lower_bound()
    assert abs(la - lb) <= rel * max(1.0, abs(lb)), (la, lb)
    for x, y, nm in zip(a.get_solver_costs(), b.get_solver_costs(), ("lo", "hi", "deferred mm")):
        _assert_close(x, y, rel, nm)
    _assert_close(a.get_delta(), b.get_delta(), rel, "delta")


# ---------------------------------------------------------------- instances of each sweep family / exchange
def _cover10(seed=5, V=500, rows=1500):
    rng = np.random.Generator(np.random.PCG64(seed))
    col = BddCollection()
    for _ in range(rows):
        col.add_covering(np.sort(rng.choice(V, size=10, replace=False)))
    return col, rng.normal(0, 3, col.nr_variables()).round(3)


def _wide(seed=21):
    rng = np.random.Generator(np.random.PCG64(seed))
    col = BddCollection()
    V = 40
    for _ in range(6):
        k = int(rng.integers(16, 22))
        vs = np.sort(rng.choice(V, size=k, replace=False))
        co = rng.integers(1, 40, size=k)
        col.add_linear(co, "<=", int(co.sum() // 2), vs)
    for _ in range(30):
        col.add_covering(np.sort(rng.choice(V, size=5, replace=False)))
    return col, rng.normal(0, 3, col.nr_variables()).round(3)


def _huge():
    from bdd_amd import native
    rng = np.random.Generator(np.random.PCG64(1))
    n = 28
    co = rng.integers(1, 5000, size=n)
    rows = [(co, np.arange(n), "<=", int(co.sum() // 2))]
    for _ in range(6):
        k = int(rng.integers(3, 9))
        rows.append((np.ones(k, int), np.sort(rng.choice(n, size=k, replace=False)), ">=", 1))
    c2 = rng.integers(1, 40, size=n)
    rows.append((c2, np.arange(n), ">=", int(c2.sum() // 3)))
    col = native.rows_to_bdd_collection(rows)
    assert max(col.layer_widths(0)) > 2048
    return col, rng.normal(0, 5, n).round(3)


def _assignment8():
    ilp = assignment_ilp(8, None)
    return to_bdd_collection(ilp), np.asarray(ilp.objective, np.float64)


def _mixed_rows():
    return random_set_cover_mixed(300, 200, 3, 16, seed=4)   # rows of 3 ... 16 variables


NOFUSE = 0x80000   # variant_flags bit 19: four launches per iteration (the fused single-workgroup kernel has its own exchange)
FAMILIES = {
    # name: (instance, options, expected solve_sweep_kind or None)
    "narrow3": (_cover10, dict(pack_width=128, waves_per_block=4, resident_sweeps=1, variant_flags=0x2000), "streaming3"),
    "narrow2": (_cover10, dict(pack_width=128, waves_per_block=4, resident_sweeps=1, variant_flags=0x2000 | 0x40000), "streaming2"),
    "narrow_gen1": (_cover10, dict(pack_width=128, waves_per_block=4, resident_sweeps=1, variant_flags=0x1000 | 0x40000), "streaming1"),
    "res2": (_cover10, dict(pack_width=64, resident_sweeps=2, variant_flags=NOFUSE), "resident2"),
    "res": (_cover10, dict(pack_width=64, resident_sweeps=2, variant_flags=NOFUSE | 0x800), "resident1"),
    "mixed": (_wide, dict(pack_width=64, wide_pack_width=512, resident_sweeps=1), "mixed"),
    "wide2": (_wide, dict(pack_width=64, wide_pack_width=512, resident_sweeps=1, variant_flags=0x3), None),
    "huge": (_huge, dict(), None),
    "deterministic_seg": (_cover10, dict(deterministic=True), None),
    "exchange_by_variable": (_cover10, dict(pack_width=64, exchange_by_variable=2), None),
    "deterministic_gathers": (_cover10, dict(deterministic=True, variant_flags=0x20000), None),
    "fused_small_off": (_assignment8, dict(variant_flags=NOFUSE), None),
    # exchanges whose LDS exceeds the 64 KiB a launch gets without the attribute: 1024-thread bins of 8 192 variables (128 KiB of
    # accumulators) and the deterministic schedule on bins of ~20 k entries (float: ~120 KiB of differences, pairs and counts)
    "reduce_lds_128k": (lambda: random_set_cover(20_000, 14_000, 8, seed=3), dict(vars_per_bin=8192), None),
    "deterministic_large_bins": (lambda: random_set_cover(40_000, 20_000, 10, seed=4), dict(deterministic=True, vars_per_bin=4096), None),
    # pack_stagger: chained packs (BDDs start below a pack's first hop, hop_root) — the general form of the streaming sweeps, in the first
    # generation and (bit 13) with records, and the wide sweeps with roots below the first hop, in one launch with the narrow ones and apart
    "chained_rows": (_mixed_rows, dict(resident_sweeps=1, pack_stagger=24), "streaming1"),
    "chained_rows_records": (_mixed_rows, dict(resident_sweeps=1, pack_stagger=24, variant_flags=0x2000), "streaming2"),
    "chained_knapsack": (_knapsack_rows, dict(pack_width=64, resident_sweeps=1, pack_stagger=24), "streaming1"),
    "chained_mixed": (_wide, dict(pack_width=64, wide_pack_width=192, resident_sweeps=1, pack_stagger=60), "mixed"),
    "chained_wide2": (_wide, dict(pack_width=64, wide_pack_width=192, resident_sweeps=1, pack_stagger=60, variant_flags=0x3), "streaming1"),
}
# the chained families and the family of test_gpu_sum_marginals.CHAINED whose instance and layout options they share
CHAINED = {"chained_rows": "chained_rows", "chained_rows_records": "chained_rows", "chained_knapsack": "chained_knapsack", "chained_mixed": "chained_wide",
           "chained_wide2": "chained_wide2"}


def assert_chained(family, col, opts):
    """a chained family's layout is chained: the recorded hops of every pack, a pack longer than the longest BDD (test_gpu_sum_marginals)"""
    if family in CHAINED:
        assert_chained_layout(CHAINED[family], col, Layout(col, **{k: v for k, v in opts.items() if k in LAYOUT_OPTIONS}))


@pytest.mark.parametrize("precision", ["double", "float"])
@pytest.mark.parametrize("family", list(FAMILIES))
def test_isotropic_weights_equal_plain_iterations(family, precision):
    make, opts, kind = FAMILIES[family]
    col, costs = make()
    assert_chained(family, col, opts)
    a = bdd_hip_parallel_mma(col, costs, precision=precision, **opts)
    b = bdd_hip_parallel_mma(col, costs, precision=precision, **opts)
    if kind is not None:
        assert a.solve_sweep_kind() == kind, a.solve_sweep_kind()
    if family == "wide2":
        assert a.solve_sweep_kind() != "mixed"
    if "variant_flags" in opts and opts["variant_flags"] & NOFUSE:
        assert not a.fused_small()
    iso = a.get_isotropic_dist_weights()
    assert iso.dtype == a.value_type and iso.size == a.nr_layers()
    np.testing.assert_array_equal(iso, (a.value_type(1) / a.get_num_bdds_per_var()[a.get_primal_variable_index()].astype(a.value_type)))
    for n in (1, 5):
        assert a.learned_iterations(iso, n, 0.5, improvement_slope=0.0) == n
        b.iterations(n)
        _same_state(a, b, precision, ISO_TOL)


# ---------------------------------------------------------------- random weights against the restatement
def _dirichlet_weights(s, rng, dtype, normalised=True):
    var = s.get_primal_variable_index()
    w = np.zeros(var.size)
    if not normalised:
        return rng.uniform(0.0, 0.8, var.size).astype(dtype)
    for v in np.unique(var):
        idx = np.flatnonzero(var == v)
        w[idx] = rng.dirichlet(np.ones(idx.size))
    return w.astype(dtype)


def _compare_with_restatement(s, m, perm, precision, what):
    lo, hi, mm = s.get_solver_costs()
    rel = REF_TOL[precision]
    _assert_close(lo[perm], m.lo, rel, what + " lo")
    _assert_close(hi[perm], m.hi, rel, what + " hi")
    _assert_close(mm[perm], m.mm, rel, what + " deferred mm")
    lb, ref = s.lower_bound(), m.lower_bound()
    assert abs(lb - ref) <= rel * max(1.0, abs(ref)), (what, lb, ref)


def _restatement_of(col, costs, precision):
    m = LearnedMma(col.instr, col.delims, precision)
    m.update_costs_hi(np.asarray(costs, np.float64))
    return m


@pytest.mark.parametrize("precision", ["double", "float"])
@pytest.mark.parametrize("normalised", [True, False])
@pytest.mark.parametrize("name", GOLDEN + ["random_cover"])
def test_random_weights_vs_restatement(name, normalised, precision):
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
    np.testing.assert_array_equal(m.layer_var, s.get_primal_variable_index()[perm])
    rng = np.random.Generator(np.random.PCG64(zlib.crc32(f"{name}/{normalised}".encode())))
    w = _dirichlet_weights(s, rng, s.value_type, normalised)
    w_bdd_major = w[perm]
    for it in range(6):
        assert s.learned_iterations(w, 1, 0.5, improvement_slope=0.0) == 1
        m.learned_iteration(w_bdd_major, 0.5)
        _compare_with_restatement(s, m, perm, precision, f"{name} iteration {it}")


# ---------------------------------------------------------------- reparametrisation
@pytest.mark.parametrize("precision", ["double", "float"])
def test_normalised_weights_reparametrise_and_bound_stays_below_lp_optimum(precision):
    col, z = load_golden("matching_3x3_first_row")
    s = bdd_hip_parallel_mma(col, None, precision=precision)
    costs = pad_costs(z["costs"], s.nr_variables())
    s.update_costs([], costs)
    rng = np.random.Generator(np.random.PCG64(3))
    for _ in range(10):
        w = _dirichlet_weights(s, rng, s.value_type)
        s.learned_iterations(w, 3, 0.5, improvement_slope=0.0)
        assert s.lower_bound() <= -4.0 + 1e-9     # the LP optimum of this instance (oracle KAT)
    s.distribute_delta()
    tol = 1e-9 if precision == "double" else 1e-5
    np.testing.assert_allclose(s.get_primal_objective_vector_host(), costs, rtol=tol, atol=tol * max(1.0, np.abs(costs).max()))


# ---------------------------------------------------------------- early stop and history
def _history_case(precision, cfi, slope, device, num_itr=12):
    col, costs = random_set_cover(120, 90, 5, seed=7)
    s = bdd_hip_parallel_mma(col, costs, precision=precision)
    m = _restatement_of(col, costs, precision)
    perm = s.bdd_major_order()
    rng = np.random.Generator(np.random.PCG64(9))
    w = _dirichlet_weights(s, rng, s.value_type)
    L, B, dt = s.nr_layers(), s.nr_bdds(), s.value_type
    h_sol, h_l1, h_l2 = np.full(L, 7.0, dt), np.full(B, 7.0, dt), np.full(B, 7.0, dt)
    r_sol, r_l1, r_l2 = np.full(L, 7.0, dt), np.full(B, 7.0, dt), np.full(B, 7.0, dt)
    args = dict(improvement_slope=slope, compute_history_for_itr=cfi, history_avg_beta=0.9)
    results = []
    for call in range(2):   # a second call: initial_lb_change is kept from the first
        if device:
            import torch
            tdt = torch.float64 if dt == np.float64 else torch.float32
            outs = [torch.tensor(x, dtype=tdt, device="cuda") for x in (h_sol, h_l1, h_l2)]
            wt = torch.tensor(w, dtype=tdt, device="cuda")
            ran = s.learned_iterations(wt, num_itr, 0.5, sol_avg=outs[0], lb_first_diff_avg=outs[1], lb_second_diff_avg=outs[2], **args)
            torch.cuda.synchronize()
            h_sol, h_l1, h_l2 = (o.cpu().numpy() for o in outs)
        else:
            ran = s.learned_iterations(w, num_itr, 0.5, sol_avg=h_sol, lb_first_diff_avg=h_l1, lb_second_diff_avg=h_l2, **args)
        r_sol_b = r_sol[perm]
        ran_ref = m.iterations(w[perm], num_itr, 0.5, sol_avg=r_sol_b, lb_first_diff_avg=r_l1, lb_second_diff_avg=r_l2, **args)
        r_sol[perm] = r_sol_b
        results.append((ran, ran_ref))
        assert ran == ran_ref, (call, ran, ran_ref)
        rel = REF_TOL[precision]
        _assert_close(h_sol, r_sol, rel, "sol_avg")
        # the averages are differences of per-BDD bounds: their error is the bounds' error, so the absolute bound scales with the bounds
        lb_scale = max(1.0, float(np.abs(m.lower_bound_per_bdd()).max()))
        np.testing.assert_allclose(h_l1, r_l1, rtol=rel, atol=4 * rel * lb_scale, err_msg="lb_first_diff_avg")
        np.testing.assert_allclose(h_l2, r_l2, rtol=rel, atol=8 * rel * lb_scale, err_msg="lb_second_diff_avg")
        _compare_with_restatement(s, m, perm, precision, f"call {call}")
    return results


@pytest.mark.parametrize("precision", ["double", "float"])
@pytest.mark.parametrize("cfi", [0, 1, 3])
@pytest.mark.parametrize("slope", [0.0, 1e-3])
@pytest.mark.parametrize("device", [False, True])
def test_history_and_early_stop_vs_restatement(precision, cfi, slope, device):
    results = _history_case(precision, cfi, slope, device)
    if slope == 0.0:
        assert all(r == (12, 12) for r in results)


def test_history_bit_for_bit_on_an_exact_instance():
    """8 x 8 assignment in float: every variable sits in two BDDs, so the exchange's double sum of two floats rounded once is the float sum
    of the restatement and the sweeps' arithmetic is the restatement's — the state, the per-BDD bounds and therefore the history agree bit
    for bit, which pins the EMA's rounding rule (beta * avg in REAL, the rest in double, one rounding) on the GPU."""
    rng = np.random.Generator(np.random.PCG64(12))
    ilp = assignment_ilp(8, rng.normal(0, 3, (8, 8)).round(4))
    col = to_bdd_collection(ilp)
    costs = np.asarray(ilp.objective, np.float64)
    s = bdd_hip_parallel_mma(col, costs, precision="float")
    m = _restatement_of(col, costs, "float")
    perm = s.bdd_major_order()
    w = _dirichlet_weights(s, rng, np.float32)
    L, B = s.nr_layers(), s.nr_bdds()
    h = [np.full(L, 7.0, np.float32), np.full(B, 7.0, np.float32), np.full(B, 7.0, np.float32)]
    r = [np.full(L, 7.0, np.float32), np.full(B, 7.0, np.float32), np.full(B, 7.0, np.float32)]
    ran = s.learned_iterations(w, 10, 0.5, improvement_slope=0.0, sol_avg=h[0], lb_first_diff_avg=h[1], lb_second_diff_avg=h[2],
                               compute_history_for_itr=10, history_avg_beta=0.7)
    r_sol = r[0][perm]
    assert ran == m.iterations(w[perm], 10, 0.5, improvement_slope=0.0, sol_avg=r_sol, lb_first_diff_avg=r[1], lb_second_diff_avg=r[2],
                               compute_history_for_itr=10, history_avg_beta=0.7) == 10
    r[0][perm] = r_sol
    lo, hi, mm = s.get_solver_costs()
    np.testing.assert_array_equal(lo[perm], m.lo)
    np.testing.assert_array_equal(hi[perm], m.hi)
    np.testing.assert_array_equal(mm[perm], m.mm)
    for x, y, nm in zip(h, r, ("sol_avg", "lb_first_diff_avg", "lb_second_diff_avg")):
        np.testing.assert_array_equal(x, y, err_msg=nm)
    assert len(np.unique(h[0])) > 2   # the solutions did change along the way: the EMA was exercised


def test_early_stop_fires():
    col, z = load_golden("matching_3x3_first_row")
    s = bdd_hip_parallel_mma(col, None, precision="double")
    s.update_costs([], pad_costs(z["costs"], s.nr_variables()))
    ran = s.learned_iterations(s.get_isotropic_dist_weights(), 500, 0.5, improvement_slope=1e-3)
    m = LearnedMma(z["instr"], z["delims"], "double")
    m.update_costs_hi(np.asarray(z["costs"], np.float64))
    assert 1 < ran < 500 and ran == m.iterations(m.isotropic_alpha(), 500, 0.5, improvement_slope=1e-3)


# ---------------------------------------------------------------- state hand-over
@pytest.mark.parametrize("precision", ["double", "float"])
def test_learned_then_plain_equals_plain(precision):
    col, costs = random_set_cover(2000, 1500, 8, seed=1)
    a = bdd_hip_parallel_mma(col, costs, precision=precision)
    b = bdd_hip_parallel_mma(col, costs, precision=precision)
    a.iterations(2)              # a pending isotropic delta at entry
    b.iterations(2)
    a.learned_iterations(a.get_isotropic_dist_weights(), 4, 0.5, improvement_slope=0.0)
    a.iterations(3)
    b.iterations(7)
    _same_state(a, b, precision, ISO_TOL)
    _, m0a, m1a = a.min_marginals_cuda(False)
    _, m0b, m1b = b.min_marginals_cuda(False)
    _assert_close(m0a, m0b, ISO_TOL[precision])
    _assert_close(m1a, m1b, ISO_TOL[precision])


@pytest.mark.parametrize("precision", ["double", "float"])
def test_save_load_after_learned_iterations(precision):
    col, costs = random_set_cover(2000, 1500, 8, seed=2)
    s = bdd_hip_parallel_mma(col, costs, precision=precision)
    rng = np.random.Generator(np.random.PCG64(4))
    s.learned_iterations(_dirichlet_weights(s, rng, s.value_type), 5, 0.5, improvement_slope=0.0)
    with tempfile.TemporaryDirectory() as d:
        p = os.path.join(d, "s.bin")
        s.save(p)
        t = bdd_hip_parallel_mma.load(p)
    for x, y in zip(s.get_solver_costs(), t.get_solver_costs()):
        np.testing.assert_array_equal(x, y)
    np.testing.assert_array_equal(s.get_delta(), t.get_delta())
    assert s.lower_bound() == t.lower_bound()
    s.iterations(3)
    t.iterations(3)
    assert s.lower_bound() == t.lower_bound()


@pytest.mark.parametrize("precision", ["double", "float"])
def test_fused_small_instance_takes_the_four_launch_path(precision):
    col, costs = _assignment8()
    f = bdd_hip_parallel_mma(col, costs, precision=precision)
    q = bdd_hip_parallel_mma(col, costs, precision=precision, variant_flags=NOFUSE)
    assert f.fused_small() and not q.fused_small()
    rng = np.random.Generator(np.random.PCG64(8))
    w = _dirichlet_weights(f, rng, f.value_type)
    L, B = f.nr_layers(), f.nr_bdds()
    outs = [[np.zeros(L, f.value_type), np.zeros(B, f.value_type), np.zeros(B, f.value_type)] for _ in range(2)]
    for s, o in zip((f, q), outs):
        assert s.learned_iterations(w, 6, 0.5, improvement_slope=0.0, sol_avg=o[0], lb_first_diff_avg=o[1], lb_second_diff_avg=o[2],
                                    compute_history_for_itr=3) == 6
        s.iterations(4)   # the fused kernel continues from the state the learned iterations leave
    for x, y in zip(f.get_solver_costs(), q.get_solver_costs()):
        _assert_close(x, y, ISO_TOL[precision])
    assert abs(f.lower_bound() - q.lower_bound()) <= ISO_TOL[precision] * max(1.0, abs(q.lower_bound()))
    for x, y in zip(*outs):
        _assert_close(x, y, ISO_TOL[precision])


# ---------------------------------------------------------------- argument errors
@pytest.mark.parametrize("precision", ["double", "float"])
def test_argument_errors_leave_the_solver_usable(precision):
    col, costs = random_set_cover(300, 200, 6, seed=5)
    s = bdd_hip_parallel_mma(col, costs, precision=precision)
    ref = bdd_hip_parallel_mma(col, costs, precision=precision)
    iso = s.get_isotropic_dist_weights()
    other = np.float32 if s.value_type == np.float64 else np.float64
    bad = {
        "wrong length": (iso[:-1], "has"),
        "NaN": (np.where(np.arange(iso.size) == 3, np.nan, iso).astype(s.value_type), "not finite"),
        "infinite": (np.where(np.arange(iso.size) == 5, np.inf, iso).astype(s.value_type), "not finite"),
        "negative": (np.where(np.arange(iso.size) == 7, -0.25, iso).astype(s.value_type), "negative"),
        "dtype": (iso.astype(other), "the solver's values are"),
    }
    import torch
    tdt = torch.float64 if s.value_type == np.float64 else torch.float32
    for what, (w, msg) in bad.items():
        with pytest.raises(BddMmaError, match=r"bdd_mma error -1: .*" + msg):
            s.learned_iterations(w, 3)
        if what != "dtype":
            wt = torch.tensor(w, dtype=tdt, device="cuda")
            with pytest.raises(BddMmaError, match=r"bdd_mma error -1: "):
                s.learned_iterations(wt, 3)
    wt = torch.tensor(np.repeat(iso, 2), dtype=tdt, device="cuda")[::2]   # right length and type, not contiguous
    assert not wt.is_contiguous()
    with pytest.raises(BddMmaError, match=r"bdd_mma error -1: .*contiguous"):
        s.learned_iterations(wt, 3)
    wt = torch.tensor(iso, dtype=torch.float32 if tdt == torch.float64 else torch.float64, device="cuda")
    with pytest.raises(BddMmaError, match=r"bdd_mma error -1: "):
        s.learned_iterations(wt, 3)
    # history outputs of the wrong size
    with pytest.raises(BddMmaError, match=r"bdd_mma error -1: "):
        s.learned_iterations(iso, 3, sol_avg=np.zeros(3, s.value_type), lb_first_diff_avg=np.zeros(s.nr_bdds(), s.value_type),
                             lb_second_diff_avg=np.zeros(s.nr_bdds(), s.value_type), compute_history_for_itr=1)
    # the solver is untouched and usable
    _same_state(s, ref, precision, {"double": 0.0, "float": 0.0})
    assert s.learned_iterations(iso, 3, 0.5, improvement_slope=0.0) == 3
    ref.iterations(3)
    _same_state(s, ref, precision, ISO_TOL)


def test_lbfgs_wrapper_attached_is_refused():
    col, costs = random_set_cover(300, 200, 6, seed=6)
    s = bdd_hip_parallel_mma(col, costs, precision="double")
    iso = s.get_isotropic_dist_weights()
    lb = bdd_hip_lbfgs(s)
    with pytest.raises(BddMmaError, match=r"bdd_mma error -4: .*L-BFGS"):
        s.learned_iterations(iso, 2)
    lb.close()
    assert s.learned_iterations(iso, 2, 0.5, improvement_slope=0.0) == 2
