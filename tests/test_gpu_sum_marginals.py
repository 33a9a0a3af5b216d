"""GPU tests of sum-marginals and the smooth solution (bddmma_sum_marginals / bddmma_smooth_solution; kernels/summarg.hpp) against the NumPy
restatement tests/sum_marginals_restatement.py (itself pinned to brute-force enumeration by tests/test_sum_marginals_restatement.py).

Tolerance of the comparisons with the restatement — measured, not chosen: the restatement runs on the same instance and costs once in the
solver's precision and once in the next wider type (float32 / float64, float64 / longdouble); `dev` = the largest absolute deviation of
the log values.  The device may differ from the wider run by 4 * dev (it sums a layer and a node's parents in another order than NumPy;
a wrong or missing term shows as a deviation of order 1), with a floor of 16 ulp of max(1, |log value|).  Absolute on the logs, relative
on the probabilities; -inf must match -inf exactly.  Each case prints its figures (pytest -s)."""
import numpy as np
import pytest

from bdd_amd import native
from bdd_amd.capi import BddMmaError
from bdd_amd.instances import assignment_ilp, random_set_cover_mixed
from bdd_amd.solver import bdd_hip_lbfgs, bdd_hip_parallel_mma
from sum_marginals_restatement import (TWO_SIMPLEX_CLOSED_FORMS, SumMarginals, assignment8 as _assignment8, cover10 as _cover10, huge_rows as _huge,
                                       general_rows as _general_rows, knapsack_rows as _knapsack_rows, restatement_of, two_simplex, wide_rows as _wide)
from test_layout import Layout
from util import pad_costs

pytestmark = pytest.mark.gpu

WIDER = {np.float32: np.float64, np.float64: np.longdouble}


def _cover10_small():
    return _cover10(seed=5, V=200, rows=300)


def _mixed_rows():
    return random_set_cover_mixed(300, 200, 3, 16, seed=4)   # rows of 3 ... 16 variables: staggered narrow packs


def _split():
    ilp = assignment_ilp(8, None)
    col = native.lp_to_bdd_collection(ilp.write_lp(), split=True, split_length=4)   # the "split bdds" output of the input stage
    return col, pad_costs(np.asarray(ilp.objective, np.float64), col.nr_variables())


# What reaches the two levels of the layer folds (kernels/pull.hpp: pull_layer_fold, runs of 16 slots), from the layouts alone: a layer that
# spans more than one run, so that its head folds several runs, and a run that starts at a multiple of 16 that is no layer head.
#   narrow packs  knapsack_w64 only (2 packs, widest layer 29 slots, 14 such run starts; a layer has at most 2 runs) — every other
#                 family's narrow packs hold covering / equality rows, whose layers have at most 2 nodes;
#   wide packs    wide2 / mixed (6 packs, widest layer 152 slots, 185 such run starts, up to 10 runs a layer), huge (1 pack, 180 slots);
#   huge packs    huge (1 pack, widest layer 7 843 slots, 2 191 such run starts, up to 491 runs a layer).
FAMILIES = {
    "cover10_w64": (_cover10_small, dict(pack_width=64)),
    "cover10_w128": (_cover10_small, dict(pack_width=128)),
    "cover10_w256": (_cover10_small, dict(pack_width=256)),
    "wide2": (_wide, dict(pack_width=64, wide_pack_width=512, resident_sweeps=1, variant_flags=0x3)),
    "mixed": (_wide, dict(pack_width=64, wide_pack_width=512, resident_sweeps=1)),
    "huge": (_huge, dict()),
    "knapsack_w64": (_knapsack_rows, dict(pack_width=64)),
    "assignment8": (_assignment8, dict()),
    "staggered_rows": (_mixed_rows, dict()),
    "split_bdds": (_split, dict()),
    # pack_stagger: chained packs — BDDs start below a pack's first hop (PackSet::hop_root), what the layout builds by itself for large
    # instances with general linear rows.  The instance of an existing family each (the same references, seeds and certificates: the
    # restatements never see the layout), and one with several chained workgroups of both kinds; CHAINED holds what the layout must show
    "chained_rows": (_mixed_rows, dict(pack_stagger=24)),
    "chained_knapsack": (_knapsack_rows, dict(pack_width=64, pack_stagger=24)),
    "chained_wide": (_wide, dict(pack_width=64, wide_pack_width=192, pack_stagger=60)),
    "chained_wide2": (_wide, dict(pack_width=64, wide_pack_width=192, pack_stagger=60, variant_flags=0x3)),
    "chained_general": (_general_rows, dict(pack_width=64, wide_pack_width=192, pack_stagger=30)),
}
# Per chained family: the hops of every narrow pack, of every wide pack (tests/test_layout.py::Layout, from the options above) and the
# solve_sweep_kind() observed on the MI355X (the kind is that of the narrow packs: the one narrow pack beside the chained wide pack is
# not chained and, with resident_sweeps left to the rules, resident; chained_general's sweeps run narrow and wide packs in one launch).
# A pack with more hops than the longest BDD has layers holds a BDD that starts below its first hop.
# tests/test_exact_fixtures.py::test_chained_families_are_chained asserts the layout without a GPU, assert_chained() on every solver
# built here: a change of the layout rules must not quietly move these cases back to side-by-side packs.
CHAINED = {
    "chained_rows": dict(narrow=(16, 24, 24, 24, 24, 3), wide=(), longest=16, kind="streaming1"),
    "chained_knapsack": dict(narrow=(17,), wide=(), longest=14, kind="streaming1"),
    "chained_wide": dict(narrow=(5,), wide=(36,), longest=20, kind="resident2"),
    "chained_wide2": dict(narrow=(5,), wide=(36,), longest=20, kind="resident2"),
    "chained_general": dict(narrow=(30, 30, 30, 5), wide=(29, 25, 16), longest=19, kind="mixed"),
}
LAYOUT_OPTIONS = ("pack_width", "wide_pack_width", "pack_stagger")


def assert_chained_layout(family, col, lay):
    """`lay`, the layout of the chained family's collection (a tests/test_layout.py::Layout built from the family's LAYOUT_OPTIONS), is
    chained: the pack counts and hops of CHAINED, some pack longer than the longest BDD, and wide BDDs sharing wide packs"""
    want = CHAINED[family]
    hops = [tuple(int(h) for h in np.diff(S["pack_hop_ptr"].astype(np.int64))) if S["P"] else () for S in lay.sets]
    longest = max(len(col.layer_widths(b)) for b in range(col.nr_bdds()))
    assert longest == want["longest"], (family, longest)
    assert (hops[0], hops[1], lay.np_h) == (want["narrow"], want["wide"], 0), (family, hops)
    assert max(hops[0] + hops[1]) > longest, (family, hops, longest)
    if want["wide"]:
        assert max(hops[1]) > longest, (family, hops, longest)
        n_wide_bdds = sum(1 for b in range(col.nr_bdds()) if max(col.layer_widths(b)) > lay.pack_width)
        assert 0 < lay.np_w < n_wide_bdds, (family, lay.np_w, n_wide_bdds)


def assert_chained(family, col, s):
    """where a chained family's solver is built: the layout its options give is chained and the solve sweeps are the observed kind"""
    if family not in CHAINED:
        return
    assert_chained_layout(family, col, Layout(col, **{k: v for k, v in FAMILIES[family][1].items() if k in LAYOUT_OPTIONS}))
    assert (s.nr_packs(), s.solve_sweep_kind()) == (len(CHAINED[family]["narrow"]) + len(CHAINED[family]["wide"]), CHAINED[family]["kind"]), \
        (family, s.nr_packs(), s.solve_sweep_kind())


def _tolerance(m, dt):
    """(reference logs in the wider type, allowed absolute deviation per layer) — see the module docstring"""
    a = m.log_sum_marginals(dt)
    b = m.log_sum_marginals(WIDER[dt])
    fin = [np.isfinite(y) for y in b]
    for x, y in zip(a, b):
        assert np.array_equal(np.isneginf(x), np.isneginf(y))
    dev = max(float(np.max(np.abs(x[f].astype(np.longdouble) - y[f]), initial=0.0)) for x, y, f in zip(a, b, fin))
    ref = [np.asarray(y, np.float64) for y in b]
    tol = [np.maximum(4 * dev, 16 * np.finfo(dt).eps * np.maximum(1.0, np.abs(np.where(f, r, 0.0)))) for r, f in zip(ref, fin)]
    return ref, tol, dev


def _check_logs(got, ref, tol, what):
    got = np.asarray(got, np.float64)
    ninf = np.isneginf(ref)
    assert np.array_equal(np.isneginf(got), ninf), what + ": -inf pattern"
    err = np.abs(got[~ninf] - ref[~ninf])
    print(f"{what}: max |dev| {err.max(initial=0.0):.3e}, allowed (min over layers) {tol[~ninf].min(initial=np.inf):.3e}")
    assert np.all(err <= tol[~ninf]), (what, float(err.max()), float(tol.min()))


def _sync_costs(s, m, perm):
    lo, hi, _ = s.get_solver_costs()
    m.lo[:], m.hi[:] = lo[perm], hi[perm]


@pytest.mark.parametrize("precision", ["double", "float"])
@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_against_restatement(family, precision):
    make, opts = FAMILIES[family]
    col, costs = make()
    s = bdd_hip_parallel_mma(col, costs, precision=precision, **opts)
    assert_chained(family, col, s)
    dt = s.value_type
    m = restatement_of(col, costs, precision)
    perm = s.bdd_major_order()
    var_l = s.get_primal_variable_index()
    for n_itr in (0, 5):
        if n_itr:
            s.iterations(n_itr)
        _sync_costs(s, m, perm)
        (ref_lo, ref_hi), (tol_lo, tol_hi), dev = _tolerance(m, dt)
        print(f"{family} {precision} after {n_itr} iterations: restatement {np.dtype(dt).name} vs wider: max |dev| of the logs {dev:.3e}")
        var, lo, hi = s.sum_marginals_cuda(get_sorted=False, get_log_probs=True)
        assert lo.dtype == dt and np.array_equal(var, var_l)
        _check_logs(lo[perm], ref_lo, tol_lo, "layer order lo")
        _check_logs(hi[perm], ref_hi, tol_hi, "layer order hi")
        # invariant: the log-partition of a BDD is the same whichever layer it is read from.  Two device values, each within its layer's
        # tolerance of the exact one: their difference is within twice the largest tolerance of the BDD.
        z = np.logaddexp(lo[perm].astype(np.float64), hi[perm].astype(np.float64))
        bdd = m.layer_bdd()
        for b in range(m.n_bdds):
            zb, tb = z[bdd == b], np.maximum(tol_lo, tol_hi)[bdd == b]
            assert np.all(np.abs(zb - zb[0]) <= 2 * tb.max()), (b, zb)
        # sorted order: the same values gathered by (variable, bdd), the order of min_marginals_cuda(True)
        var_s, lo_s, hi_s = s.sum_marginals_cuda(get_sorted=True, get_log_probs=True)
        var_m, _, _ = s.min_marginals_cuda(True)
        assert np.array_equal(var_s, var_m)
        order = np.lexsort((s.get_bdd_index(), var_l))
        np.testing.assert_array_equal(lo_s, lo[order])
        np.testing.assert_array_equal(hi_s, hi[order])
        # probabilities
        _, plo, phi = s.sum_marginals_cuda(get_sorted=False, get_log_probs=False)
        for got, ref, tol, nm in ((plo[perm], ref_lo, tol_lo, "lo"), (phi[perm], ref_hi, tol_hi, "hi")):
            got = got.astype(np.float64)
            want = np.exp(ref)
            rep = want >= np.finfo(dt).tiny   # representable as a normal number in the solver's precision
            assert np.all(got[np.isneginf(ref)] == 0)
            assert np.all(np.abs(got[rep] - want[rep]) <= (np.expm1(tol[rep]) + 4 * np.finfo(dt).eps) * want[rep]), nm
        # smooth solution: in [0, 1] and the formula applied to the returned logs
        sm = s.smooth_solution_per_bdd()
        assert sm.dtype == dt and np.all((sm >= 0) & (sm <= 1))
        np.testing.assert_allclose(sm, SumMarginals.smooth_solution(lo, hi), rtol=8 * np.finfo(dt).eps, atol=np.finfo(dt).tiny)
    mm = s.sum_marginals(True)
    assert len(mm) == s.nr_variables() and all(a.shape == (n, 2) for a, n in zip(mm, s.get_num_bdds_per_var()))
    s.close()


@pytest.mark.parametrize("precision", ["double", "float"])
@pytest.mark.parametrize("log_probs", [False, True])
def test_two_simplex_closed_forms(precision, log_probs):
    col, costs = two_simplex()
    s = bdd_hip_parallel_mma(col, costs, precision=precision)
    mm = s.sum_marginals(log_probs)
    assert len(mm) == 6 and all(a.shape == (1, 2) for a in mm)
    for v in range(6):
        got = np.exp(mm[v][0]) if log_probs else mm[v][0]
        assert abs(got[0] - TWO_SIMPLEX_CLOSED_FORMS[v][0]) <= 1e-5 and abs(got[1] - TWO_SIMPLEX_CLOSED_FORMS[v][1]) <= 1e-5, (v, got)
    s.close()


@pytest.mark.parametrize("precision", ["double", "float"])
def test_path_counts_at_cost_zero(precision):
    col, costs = _knapsack_rows()
    s = bdd_hip_parallel_mma(col, 0 * costs, precision=precision)
    m = restatement_of(col, 0 * costs, precision)
    perm = s.bdd_major_order()
    n_lo, n_hi = m.path_counts()
    _, (tol_lo, tol_hi), _ = _tolerance(m, s.value_type)
    _, plo, phi = s.sum_marginals_cuda(False, False)
    eps = 4 * np.finfo(s.value_type).eps
    assert np.all(np.abs(plo[perm] - n_lo) <= (np.expm1(tol_lo) + eps) * n_lo)
    assert np.all(np.abs(phi[perm] - n_hi) <= (np.expm1(tol_hi) + eps) * n_hi)
    s.close()


def _assignment8_normal():
    col, _ = _assignment8()
    return col, np.random.Generator(np.random.PCG64(11)).normal(0, 3, col.nr_variables()).round(3)


# share of the layers with |min-marginal difference| >= 0.25, from the CPU restatement (min-plus sweeps of learned_mma_restatement.py):
# 8 x 8 assignment with N(0, 3) costs 0.953, the knapsack rows (layers wider than two nodes) 0.870; BDDs of <= 14 variables
@pytest.mark.parametrize("precision", ["double", "float"])
@pytest.mark.parametrize("make", [_assignment8_normal, _knapsack_rows])
def test_sharp_costs_give_the_min_marginal_side(make, precision):
    """costs x 200: where the min-marginal difference (before scaling) is at least 0.25 the losing side weighs at most #paths * exp(-50)
    < 1e-16 (BDDs of <= 16 variables), so the smooth solution is the side the min-marginals prefer to 1e-6; nothing overflows in float"""
    col, costs = make()
    s = bdd_hip_parallel_mma(col, costs, precision=precision)
    _, m0, m1 = s.min_marginals_cuda(False)
    diff = m1.astype(np.float64) - m0.astype(np.float64)
    big = bdd_hip_parallel_mma(col, 200 * np.asarray(costs), precision=precision)
    _, lo, hi = big.sum_marginals_cuda(False, True)
    assert not np.any(np.isnan(lo)) and not np.any(np.isnan(hi)) and not np.any(np.isposinf(lo)) and not np.any(np.isposinf(hi))
    sm = big.smooth_solution_per_bdd().astype(np.float64)
    assert np.all(np.isfinite(sm))
    q = np.abs(diff) >= 0.25
    print(f"layers with |min-marginal difference| >= 0.25: {q.mean():.3f}")
    assert q.mean() >= 0.5
    np.testing.assert_allclose(sm[q], (diff[q] < 0).astype(np.float64), atol=1e-6, rtol=0)
    s.close()
    big.close()


def _state(s):
    return [s.lower_bound()] + list(s.get_solver_costs()) + [s.get_delta()] + list(s.min_marginals_cuda(False))


def _assert_same_state(a, b):
    for x, y in zip(_state(a), _state(b)):
        np.testing.assert_array_equal(np.asarray(x), np.asarray(y))


@pytest.mark.parametrize("precision", ["double", "float"])
@pytest.mark.parametrize("family", ["cover10_w128", "mixed", "huge", "chained_general"])
def test_state_contract(family, precision):
    make, opts = FAMILIES[family]
    col, costs = make()
    a = bdd_hip_parallel_mma(col, costs, precision=precision, deterministic=True, **opts)
    b = bdd_hip_parallel_mma(col, costs, precision=precision, deterministic=True, **opts)
    assert_chained(family, col, a)
    for s in (a, b):
        s.iterations(3)
    r1 = a.sum_marginals_cuda(False, True)
    _assert_same_state(a, b)
    a.smooth_solution_per_bdd()
    for s in (a, b):
        s.iteration()
    _assert_same_state(a, b)
    # between two learned_iterations calls
    iso = a.get_isotropic_dist_weights()
    for s in (a, b):
        s.learned_iterations(iso, 2, 0.5, improvement_slope=0.0)
    a.sum_marginals_cuda(True, False)
    for s in (a, b):
        s.learned_iterations(iso, 2, 0.5, improvement_slope=0.0)
    _assert_same_state(a, b)
    # repeated calls agree bit for bit (every sum runs in a fixed order)
    r2 = a.sum_marginals_cuda(False, True)
    r3 = a.sum_marginals_cuda(False, True)
    for x, y in zip(r2, r3):
        np.testing.assert_array_equal(x, y)
    assert not np.array_equal(r1[1], r2[1])   # the costs have moved in between
    # null pointers: an error, and the state is left alone
    with pytest.raises(BddMmaError):
        a._ck(a._L.bddmma_sum_marginals(a._h, 0, 1, None, None, None, 0))
    with pytest.raises(BddMmaError):
        a._ck(a._L.bddmma_smooth_solution(a._h, None, 0))
    _assert_same_state(a, b)
    a.close()
    b.close()


@pytest.mark.parametrize("precision", ["double", "float"])
def test_device_outputs_equal_host_outputs(precision):
    torch = pytest.importorskip("torch")
    col, costs = _wide()
    s = bdd_hip_parallel_mma(col, costs, precision=precision, pack_width=64, wide_pack_width=512, resident_sweeps=1)
    s.iterations(2)
    L = s.nr_layers()
    tdt = torch.float64 if precision == "double" else torch.float32
    for srt in (False, True):
        for logp in (False, True):
            out = (torch.zeros(L, dtype=torch.int32, device="cuda"), torch.zeros(L, dtype=tdt, device="cuda"), torch.zeros(L, dtype=tdt, device="cuda"))
            s.sum_marginals_cuda(srt, logp, out=out)
            host = s.sum_marginals_cuda(srt, logp)
            for d, h in zip(out, host):
                np.testing.assert_array_equal(d.cpu().numpy(), h)
    d = torch.zeros(L, dtype=tdt, device="cuda")
    s.smooth_solution_per_bdd(out=d)
    np.testing.assert_array_equal(d.cpu().numpy(), s.smooth_solution_per_bdd())
    s.close()


@pytest.mark.parametrize("precision", ["double", "float"])
def test_state_contract_with_lbfgs_wrapper(precision):
    col, costs = _cover10_small()
    pair = []
    for _ in range(2):
        s = bdd_hip_parallel_mma(col, costs, precision=precision, deterministic=True)
        pair.append((s, bdd_hip_lbfgs(s)))
    (a, la), (b, lb) = pair
    for _ in range(6):
        la.iteration()
        lb.iteration()
        a.sum_marginals_cuda(False, True)
    _assert_same_state(a, b)
    for s, l in pair:
        l.close()
        s.close()


def test_one_launch_per_direction_and_pack_family():
    """every sum-marginal kernel launch is a profiled group of its own (class "other"), so the profile's launch count counts kernels: one per
    direction and pack family present, whatever the number of hops (the reference: six per hop)"""
    for make, opts, families in ((_wide, dict(pack_width=64, wide_pack_width=512, resident_sweeps=1), 2), (_huge, dict(), None), (_cover10_small, dict(), 1)):
        col, costs = make()
        s = bdd_hip_parallel_mma(col, costs, precision="float", **opts)
        s.sum_marginals_cuda(False, True)   # parent tables built, states settled
        s.set_profiling(1)
        s.sum_marginals_cuda(False, True)
        p = s.get_profile()
        assert s.nr_hops() > 4
        if families is None:   # narrow, wide and huge packs as the layout chose: at most three families, at least the huge one
            assert p["launches"][3] in (2, 4, 6), p
        else:
            assert p["launches"][3] == 2 * families, p
        assert p["launches"][0] == p["launches"][1] == p["launches"][2] == 0
        s.close()


def test_cpp_members():
    """bdd_hip_parallel_mma<REAL>::sum_marginals_cuda / sum_marginals / smooth_solution_cuda and bdd_solver::sum_marginals (tests/cpp/test_sum_marginals.cpp)"""
    import os
    import subprocess
    exe = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpp", "test_sum_marginals")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout[-3000:], r.stderr[-1000:])
    assert r.returncode == 0 and "0 failure(s)" in r.stdout, r.stdout[-3000:]


def test_pybind_sum_marginals():
    from bdd_amd import bdd_solver_py
    from sum_marginals_restatement import TWO_SIMPLEX_LP
    cfg = {"precision": "double", "relaxation solver": "cuda parallel mma", "input": TWO_SIMPLEX_LP,
           "termination criteria": {"maximum iterations": 0, "improvement slope": 0.0, "minimum improvement": 0.0}}
    s = bdd_solver_py.bdd_solver(cfg, quiet=True).solve()
    for logp in (False, True):
        sm = s.sum_marginals(logp)
        assert len(sm) == 6 and len(s.min_marginals()) == 6
        for v in range(6):
            got = np.exp(sm[v][0]) if logp else np.asarray(sm[v][0])
            assert abs(got[0] - TWO_SIMPLEX_CLOSED_FORMS[v][0]) <= 1e-5 and abs(got[1] - TWO_SIMPLEX_CLOSED_FORMS[v][1]) <= 1e-5


def test_full_size_instance():
    """the benchmark's instance (10.5 M nodes, float): finite everywhere; on a 1 % sample of the BDDs the log-partition is the same from every
    layer.  Tolerance: a covering row of 10 variables sums at most 2^10 paths per value; the float restatement's measured deviation on such
    rows is below 4e-6 (profiles/sum_marginals.txt, cover10), 4 x that with the floor of 16 ulp of |log value|, twice for two values."""
    from bdd_amd.instances import random_set_cover_mt
    col, costs = random_set_cover_mt(1_000_000, 500_000, 10, seed=12345)
    s = bdd_hip_parallel_mma(col, costs, precision="float")
    assert col.nr_bdd_nodes() == 10_500_000
    s.iterations(5)
    _, lo, hi = s.sum_marginals_cuda(False, True)
    assert np.all(np.isfinite(lo)) and np.all(np.isfinite(hi))
    sm = s.smooth_solution_per_bdd()
    assert np.all(np.isfinite(sm)) and np.all((sm >= 0) & (sm <= 1))
    z = np.logaddexp(lo.astype(np.float64), hi.astype(np.float64))
    bdd = s.get_bdd_index()
    order = np.argsort(bdd, kind="stable")
    zb = z[order].reshape(-1, 10)   # every BDD has 10 layers
    assert np.array_equal(bdd[order].reshape(-1, 10)[:, 0], np.arange(500_000))
    sample = np.random.Generator(np.random.PCG64(1)).choice(500_000, size=5_000, replace=False)
    zs = zb[sample]
    tol = 2 * np.maximum(4 * 4e-6, 16 * np.finfo(np.float32).eps * np.maximum(1.0, np.abs(zs).max(axis=1)))
    spread = np.abs(zs - zs[:, :1]).max(axis=1)
    print(f"full size: largest spread of the log-partition inside a BDD {spread.max():.3e}, allowed (smallest) {tol.min():.3e}")
    assert np.all(spread <= tol)
    s.close()
