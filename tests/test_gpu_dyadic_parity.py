"""Every kernel family that runs iteration() against the oracle BIT FOR BIT, in both precisions — needs an MI355X.

On the fixtures of tests/dyadic_fixtures.py every value of ITERATIONS[shape] MMA iterations is a dyadic rational with two bits of
headroom under the mantissa (tests/test_dyadic_fixtures.py asserts that of the reference alone), so each operation is exact in float and
in double and every summation order gives the same bits: the double `Oracle`'s trajectory, cast to the solver's type, is what a kernel has
to produce — arc costs, deferred differences, delta, per-BDD bounds after EVERY iteration, min-marginals after the last, the delta of
every explicit forward_mm / backward_mm half-step of a second solver, and the state after iterations(n) in one call of a third.  The twin comparisons elsewhere in the suite show that the kernel
families agree with each other; these cases anchor each of them to the independent reference, the default (LDS-atomic) exchange included,
whose double results are otherwise not reproducible from run to run.

Each case first asserts the path it is about (solve_sweep_kind, potentials_on_chip, fused_small, nontemporal_loads, nr_packs), so that a
change of the selection rules cannot quietly move it onto another kernel.  A module-level summary prints the number of cases and the wall
time (pytest -s)."""
import ctypes as C
import time

import numpy as np
import pytest

from bdd_amd import capi
from bdd_amd.solver import bdd_hip_batch, bdd_hip_parallel_mma
from dyadic_fixtures import ITERATIONS, reference, rows, trajectory
from exact_fixtures import certificate
from test_gpu_parity import oracle_layer_perm
from test_layout import Layout

pytestmark = pytest.mark.gpu

FLOAT, DOUBLE = ("float",), ("double",)
BOTH = FLOAT + DOUBLE
EPS = {"float": 2.0 ** -24, "double": 2.0 ** -53}
_STATS = dict(cases=0, seconds=0.0)


@pytest.fixture(autouse=True)
def _count():
    t = time.perf_counter()
    yield
    _STATS["cases"] += 1
    _STATS["seconds"] += time.perf_counter() - t


@pytest.fixture(scope="module", autouse=True)
def _summary():
    yield
    print(f"\ntests/test_gpu_dyadic_parity.py: {_STATS['cases']} cases in {_STATS['seconds']:.1f} s")


def n_iterations(shape, precision):
    return ITERATIONS[shape][precision == "double"]


def same(got, want, what):
    """bit for bit after the exact cast of the reference to the solver's type (every value is representable)"""
    want = np.asarray(want)
    cast = want.astype(got.dtype)
    assert np.array_equal(cast.astype(np.float64), want.astype(np.float64)), what + ": the reference is not representable"
    np.testing.assert_array_equal(got, cast, err_msg=what)


def check_bound(s, per_bdd, precision, what):
    """lower_bound() is a sum over the BDDs and need not be exact: against the double sum of the exact per-BDD array, within the standard
    bound of a summation in the solver's type; equal where every partial sum is representable"""
    per_bdd = np.asarray(per_bdd, np.float64)
    lb, want, mass = s.lower_bound(), float(np.sum(per_bdd)), float(np.sum(np.abs(per_bdd)))
    q, _ = certificate([per_bdd])
    if mass / q <= 1.0 / EPS[precision]:
        assert lb == want, (what, lb, want)
    else:
        assert abs(lb - want) <= len(per_bdd) * EPS[precision] * mass, (what, lb, want)


def assert_path(s, path, what):
    double = s.value_type == np.float64
    kind, fused = path["kind"], path.get("fused", False)
    assert s.solve_sweep_kind() == (kind if isinstance(kind, str) else kind[double]), (what, s.solve_sweep_kind())   # a pair: (float, double)
    assert s.potentials_on_chip() == path.get("on_chip", False), (what, "potentials_on_chip", s.potentials_on_chip())
    assert s.fused_small() == (fused if isinstance(fused, bool) else fused[double]), (what, "fused_small", s.fused_small())
    assert s.nontemporal_loads() == path.get("nt", False), (what, "nontemporal_loads", s.nontemporal_loads())
    assert s.nr_packs() >= path.get("packs", 1), (what, "nr_packs", s.nr_packs())


def solver(shape, precision, opts, path):
    col, costs = rows(shape)
    s = bdd_hip_parallel_mma(col, costs, precision=precision, **opts)
    assert_path(s, path, (shape, precision, opts))
    return s, oracle_layer_perm(s, trajectory(shape).o)


def check_state(s, perm, rec, precision, what):
    lo, hi, mm = s.get_solver_costs()
    same(lo[perm], rec["lo"], what + ": lo")
    same(hi[perm], rec["hi"], what + ": hi")
    same(mm[perm], rec["mm_last"], what + ": deferred differences")
    same(s.get_delta(), rec["delta_in"], what + ": delta")
    same(s.lower_bound_per_bdd(), rec["lb_per_bdd"], what + ": lower_bound_per_bdd")
    check_bound(s, rec["lb_per_bdd"], precision, what)


def check_min_marginals(s, perm, rec, what):
    _, mm0, mm1 = s.min_marginals_cuda(get_sorted=False)
    same(mm0[perm], rec["min_marginals"][:, 0], what + ": min-marginals 0")
    same(mm1[perm], rec["min_marginals"][:, 1], what + ": min-marginals 1")


def drive(shape, precision, opts, path):
    """the comparison of the module docstring on one (shape, precision, options)"""
    n = n_iterations(shape, precision)
    ref = reference(shape, n)
    s, perm = solver(shape, precision, opts, path)
    what = f"{shape} {precision} {opts}"
    same(s.lower_bound_per_bdd(), trajectory(shape).initial["lb_per_bdd"], what + ": initial lower_bound_per_bdd")
    for it, rec in enumerate(ref):
        s.iteration()
        check_state(s, perm, rec, precision, f"{what}, iteration {it + 1}")
    check_min_marginals(s, perm, ref[-1], what)
    s.close()
    # the explicit half-steps, in a second solver of the same options (the delta is handed back undivided, as the reference's is)
    h, perm = solver(shape, precision, opts, path)
    d = np.zeros(2 * h.nr_variables(), h.value_type)
    for it, rec in enumerate(ref):
        h.forward_mm(0.5, d)
        same(d, rec["forward_delta"], f"{what}: forward_mm {it + 1}")
        h.backward_mm(0.5, d)
        same(d, rec["backward_delta"], f"{what}: backward_mm {it + 1}")
        lo, hi, _ = h.get_solver_costs()
        same(lo[perm], rec["half_lo"], f"{what}: lo after backward_mm {it + 1}")
        same(hi[perm], rec["half_hi"], f"{what}: hi after backward_mm {it + 1}")
        same(h.lower_bound_per_bdd(), rec["half_lb_per_bdd"], f"{what}: lower_bound_per_bdd after backward_mm {it + 1}")
    h.close()
    # and all iterations in one call, with no getter in between that could refresh a stale potential or bound
    s, perm = solver(shape, precision, opts, path)
    s.iterations(n)
    check_state(s, perm, ref[-1], precision, f"{what}, iterations({n})")
    check_min_marginals(s, perm, ref[-1], f"{what}, iterations({n})")
    s.close()


def drive_straight(shape, precision, opts, path):
    """iterations(n) in one call, then each consumer of the potentials straight away in a solver of its own: after the on-chip sweeps
    the stored potentials are stale and the consumer has to get a plain sweep first"""
    n = n_iterations(shape, precision)
    rec = reference(shape, n)[-1]
    what = f"{shape} {precision} {opts} straight after iterations({n})"
    s, perm = solver(shape, precision, opts, path)
    s.iterations(n)
    check_min_marginals(s, perm, rec, what)
    check_state(s, perm, rec, precision, what)
    s.close()
    s, perm = solver(shape, precision, opts, path)
    s.iterations(n)
    same(s.lower_bound_per_bdd(), rec["lb_per_bdd"], what + ": lower_bound_per_bdd")
    check_state(s, perm, rec, precision, what)
    check_min_marginals(s, perm, rec, what)
    s.close()


def params(cases):
    return [pytest.param(shape, precision, opts, path, id=f"{name}-{precision}") for name, shape, precisions, opts, path in cases for precision in precisions]


# ---------------------------------------------------------------- the sweeps that rebuild F and T on chip (kernels/narrow4.hpp), float
KEEP_IN_MEMORY, T_ONLY, F_ONLY = 0x200000, 0x400000, 0x800000   # variant_flags bits 21, 22, 23
ONCHIP_FILL = {"rows11": 76, "rows16": 76, "rows10_16": 76, "rows17": 64, "rows2": 64}   # pack_fill: a pack is one stage group (<= 640 layers) / a hop has <= 64 layers
EXCHANGES = {"atomics": dict(), "deterministic": dict(deterministic=True)}


def onchip_opts(shape, wpb, flags=0, **exchange):
    return dict(pack_width=128, resident_sweeps=1, waves_per_block=wpb, variant_flags=0x2000 | flags, pack_fill=ONCHIP_FILL.get(shape, 0), **exchange)


ONCHIP = [(f"{shape}-wpb{wpb}-{ex}", shape, FLOAT, onchip_opts(shape, wpb, **exo), dict(kind="streaming3", on_chip=shape != "rows17", packs=5))
          for shape in ("rows10", "rows2_10", "rows11", "rows16", "rows10_16", "rows17", "rows2") for wpb in (4, 8) for ex, exo in EXCHANGES.items()]
ONCHIP += [(f"rows2_10-wpb4-{name}-{ex}", "rows2_10", FLOAT, onchip_opts("rows2_10", 4, bit, **exo), dict(kind="streaming3", on_chip=True, packs=5))
           for name, bit in (("T_only", T_ONLY), ("F_only", F_ONLY)) for ex, exo in EXCHANGES.items()]
# min_marginals_cuda and lower_bound_per_bdd straight after the iterations: 10-hop and 16-hop mode, the pairs that keep one potential on
# chip, and the twin through memory (bit 21)
STRAIGHT = [(f"{shape}-wpb{wpb}-{name}-{ex}", shape, FLOAT, onchip_opts(shape, wpb, bit, **exo), dict(kind="streaming3", on_chip=bit != KEEP_IN_MEMORY, packs=5))
            for shape, wpb, pairs in (("rows2_10", 4, (("on_chip", 0), ("in_memory", KEEP_IN_MEMORY), ("T_only", T_ONLY), ("F_only", F_ONLY))),
                                      ("rows2_10", 8, (("on_chip", 0), ("in_memory", KEEP_IN_MEMORY))),
                                      ("rows11", 4, (("on_chip", 0), ("in_memory", KEEP_IN_MEMORY))),
                                      ("rows16", 8, (("on_chip", 0), ("in_memory", KEEP_IN_MEMORY))),
                                      ("rows10_16", 4, (("on_chip", 0), ("in_memory", KEEP_IN_MEMORY))))
            for name, bit in pairs for ex, exo in EXCHANGES.items()]


@pytest.mark.parametrize("shape,precision,opts,path", params(ONCHIP))
def test_on_chip_sweeps(shape, precision, opts, path):
    drive(shape, precision, opts, path)


@pytest.mark.parametrize("shape,precision,opts,path", params(STRAIGHT))
def test_consumers_straight_after_on_chip_iterations(shape, precision, opts, path):
    drive_straight(shape, precision, opts, path)


# ---------------------------------------------------------------- streaming 1 / 2 / 3 and resident 1 / 2
S1, S2, R1 = "streaming1", "streaming2", "resident1"
# what the rules choose under the option sets of test_long_bdds_vs_oracle, (float, double) for variant_flags 0 and 0x2000
LONG_BDDS_KINDS = {"rows10": {(64, 64, 4): ((S1, S2), (S2, S2)), (128, 640, 1): ((R1, R1), (R1, R1)), (256, 256, 2): ((S1, S1), (S2, S2)),
                              (64, 128, 8): ((S1, S2), (S2, S2)), (256, 640, 4): ((S1, S1), (S2, S1))},
                   "long": {(64, 64, 4): ((S1, S1), (S2, S2)), (128, 640, 1): ((S1, S1), (S2, S2)), (256, 256, 2): ((S1, S1), (S2, S2)),
                            (64, 128, 8): ((S1, S1), (S2, S2)), (256, 640, 4): ((S1, S1), (S2, S1))}}
STREAMING = []
for shape in ("rows10", "long"):
    packs = 5 if shape == "rows10" else 9
    # test_lane_per_layer_sweeps_vs_oracle_and_second_generation: the third generation (float: through memory, bit 21 — on chip is above) and
    # the second (double with eight packs per workgroup: its LDS exceeds 64 KiB and the first takes over)
    for wpb in (4, 8):
        base = dict(pack_width=128, waves_per_block=wpb, resident_sweeps=1, deterministic=True)
        STREAMING.append((f"{shape}-lane_per_layer-wpb{wpb}", shape, FLOAT, dict(base, variant_flags=0x2000 | KEEP_IN_MEMORY), dict(kind="streaming3", packs=packs)))
        STREAMING.append((f"{shape}-lane_per_layer-wpb{wpb}", shape, DOUBLE, dict(base, variant_flags=0x2000), dict(kind="streaming3", packs=packs)))
        STREAMING.append((f"{shape}-second_generation-wpb{wpb}", shape, FLOAT, dict(base, variant_flags=0x2000 | 0x40000), dict(kind="streaming2", packs=packs)))
        STREAMING.append((f"{shape}-second_generation-wpb{wpb}", shape, DOUBLE, dict(base, variant_flags=0x2000 | 0x40000),
                          dict(kind="streaming2" if wpb == 4 else "streaming1", packs=packs)))
    # test_long_bdds_vs_oracle
    for pw, cap, wpb in ((64, 64, 4), (128, 640, 1), (256, 256, 2), (64, 128, 8), (256, 640, 4)):
        for i, variant in enumerate((0, 0x2000)):
            STREAMING.append((f"{shape}-pw{pw}-cap{cap}-wpb{wpb}-v{variant:x}", shape, BOTH,
                              dict(pack_width=pw, stage_cap=cap, waves_per_block=wpb, variant_flags=variant), dict(kind=LONG_BDDS_KINDS[shape][pw, cap, wpb][i], packs=3)))
    # test_nontemporal_instantiations_of_the_first_and_second_generation (bit 13 beside bit 18 in double: these packs share no records, and
    # without it the second generation hands over to the first)
    for precision, flags, wpb, kind in ((FLOAT, 0x41000, 4, "streaming1"), (FLOAT, 0x41000, 8, "streaming1"), (DOUBLE, 0x41000, 4, "streaming1"),
                                        (DOUBLE, 0x40000, 8, "streaming1"), (DOUBLE, 0x40000 | 0x2000, 4, "streaming2"), (FLOAT, 0x41000 | 0x4000, 8, "streaming1"),
                                        (DOUBLE, 0x40000 | 0x2000 | 0x4000, 4, "streaming2")):
        STREAMING.append((f"{shape}-nontemporal-{flags:x}-wpb{wpb}", shape, precision,
                          dict(pack_width=128, waves_per_block=wpb, resident_sweeps=1, deterministic=True, variant_flags=flags | 0x100000),
                          dict(kind=kind, nt=True, packs=packs)))


# test_resident_sweeps_with_up_to_sixty_hops: a resident pack has at most 63 hops and one stage group (<= 640 layers), so rows of 17-60 with
# eight BDDs to a pack (pack_fill) stand in for the rows of 70-150 here — k_*_res2 walk them in blocks of 16 hops
for shape in ("rows10", "rows17_60"):
    for wpb in (0, 2, 4):
        for name, variant, kind in (("second", 0, "resident2"), ("first", 0x800, "resident1")):
            STREAMING.append((f"{shape}-resident-{name}-wpb{wpb}", shape, BOTH,
                              dict(pack_width=64, resident_sweeps=2, waves_per_block=wpb, variant_flags=variant, pack_fill=16 if shape == "rows17_60" else 0),
                              dict(kind=kind, packs=9)))


@pytest.mark.parametrize("shape,precision,opts,path", params(STREAMING))
def test_streaming_and_resident_sweeps(shape, precision, opts, path):
    if shape == "rows17_60":
        col, _ = rows(shape)
        assert max(len(col.layer_widths(b)) for b in range(col.nr_bdds())) == 60
    drive(shape, precision, opts, path)


# ---------------------------------------------------------------- mixed, chained, wide and huge packs
def staggered_width():
    """test_staggered_wide_packs_vs_oracle: the widest layer decides the pack width — one BDD per hop, so every further BDD of a pack has to
    start below the first hop; the layout really is staggered: fewer wide packs than wide BDDs"""
    col, _ = rows("wide_staggered")
    widths = [max(col.layer_widths(b)) for b in range(col.nr_bdds())]
    wpw = int(-(-max(widths) // 64) * 64)
    h = C.c_void_p()
    o = capi.Options(64, wpw, 0, 0, 0, 0)
    o.pack_stagger = 60
    L = capi.lib()
    capi.check(L.bddmma_layout_create(C.byref(h), np.ascontiguousarray(col.instr).ctypes.data_as(C.c_void_p),
                                      np.ascontiguousarray(col.delims).ctypes.data_as(C.c_void_p), col.nr_bdds(), C.byref(o)), None)
    n_wide_packs = int(L.bddmma_layout_size(h, 4))
    L.bddmma_layout_destroy(h)
    n_wide_bdds = sum(1 for w in widths if w > 64)
    assert 0 < n_wide_packs < n_wide_bdds, (n_wide_packs, n_wide_bdds)
    return wpw


WIDE = [("wide2", "wide", BOTH, dict(pack_width=64, wide_pack_width=512, resident_sweeps=1, variant_flags=0x3), dict(layout=(2, 6, 0), kind="streaming1", packs=2)),
        ("mixed", "wide", BOTH, dict(pack_width=64, wide_pack_width=512, resident_sweeps=1), dict(layout=(2, 6, 0), kind="mixed", packs=2)),
        ("huge", "huge", BOTH, dict(), dict(layout=(1, 1, 1), kind="resident2", packs=3)),                      # (the kind is that of the narrow packs beside the huge one)
        ("huge-small_frontiers", "huge", BOTH, dict(pack_width=64, wide_pack_width=64), dict(layout=(1, 0, 2), kind="resident2", packs=3)),
        ("knapsack_w64", "knapsack", BOTH, dict(pack_width=64), dict(layout=(2, 0, 0), kind="resident1", packs=2)),
        ("staggered_rows", "rows3_16", BOTH, dict(), dict(layout=(6, 0, 0), kind="resident2", fused=(True, False), packs=6)),   # float fits one workgroup's LDS, double does not
        # pack_stagger: BDDs of a narrow pack start below its first hop (hop_root) — the general form of the streaming sweeps, in the first
        # generation and (bit 13) with records
        ("chained_rows", "rows3_16", BOTH, dict(resident_sweeps=1, pack_stagger=24), dict(layout=(5, 0, 0), kind="streaming1", packs=5)),
        ("chained_rows-records", "rows3_16", BOTH, dict(resident_sweeps=1, pack_stagger=24, variant_flags=0x2000), dict(layout=(5, 0, 0), kind="streaming2", packs=5)),
        ("chained_knapsack", "knapsack", BOTH, dict(pack_width=64, resident_sweeps=1, pack_stagger=24), dict(layout=(1, 0, 0), kind="streaming1")),
        ("chained_knapsack-records", "knapsack", BOTH, dict(pack_width=64, resident_sweeps=1, pack_stagger=24, variant_flags=0x2000), dict(layout=(1, 0, 0), kind="streaming2"))]


@pytest.mark.parametrize("shape,precision,opts,path", params(WIDE))
def test_mixed_chained_wide_and_huge_packs(shape, precision, opts, path):
    col, _ = rows(shape)
    widest = max(max(col.layer_widths(b)) for b in range(col.nr_bdds()))
    assert widest > {"wide": 64, "huge": 2048, "knapsack": 2, "rows3_16": 1}[shape], widest
    lay = Layout(col, **{k: v for k, v in opts.items() if k in ("pack_width", "wide_pack_width", "pack_stagger")})
    assert (lay.np_n, lay.np_w, lay.np_h) == path["layout"]   # narrow, wide and huge packs
    if opts.get("pack_stagger"):   # the layout really is chained: a pack has more hops than the longest BDD has layers
        assert np.diff(lay.sets[0]["pack_hop_ptr"]).max() > max(len(col.layer_widths(b)) for b in range(col.nr_bdds()))
    drive(shape, precision, opts, path)


@pytest.mark.parametrize("precision", BOTH)
@pytest.mark.parametrize("variant", [0, 3])   # narrow + wide sweeps in one launch / as separate launches
def test_staggered_wide_packs(precision, variant):
    opts = dict(pack_width=64, wide_pack_width=staggered_width(), pack_stagger=60, variant_flags=variant)
    col, _ = rows("wide_staggered")
    lay = Layout(col, pack_width=64, wide_pack_width=opts["wide_pack_width"], pack_stagger=60)
    assert (lay.np_n, lay.np_w, lay.np_h) == (2, 2, 0)
    drive("wide_staggered", precision, opts, dict(kind="streaming1" if variant else "mixed", packs=4))


# ---------------------------------------------------------------- whole iterations in one launch, alone and as a batch
FUSED = [("assignment8", "assignment8", BOTH, dict(), dict(kind="resident2", fused=True)),
         ("cover_small", "cover_small", BOTH, dict(), dict(kind="resident2", fused=True, packs=2)),
         ("cover_small4", "cover_small4", BOTH, dict(), dict(kind="resident2", fused=True, packs=3))]


@pytest.mark.parametrize("shape,precision,opts,path", params(FUSED))
def test_fused_one_workgroup_kernel(shape, precision, opts, path):
    drive(shape, precision, opts, path)            # iteration(): launches of one
    drive_straight(shape, precision, opts, path)   # iterations(n): one launch of n


@pytest.mark.parametrize("precision", BOTH)
def test_batch_of_three_one_workgroup_members(precision):
    """one workgroup per member in one launch: every member bit-equal to ITS reference after every iteration and after iterations(n)"""
    shapes = ("assignment8", "cover_small", "cover_small4")
    n = min(n_iterations(shape, precision) for shape in shapes)
    for step in (1, n):
        members = [solver(shape, precision, dict(), dict(kind="resident2", fused=True)) for shape in shapes]
        assert len({s.nr_packs() for s, _ in members}) == 3, [s.nr_packs() for s, _ in members]
        batch = bdd_hip_batch([s for s, _ in members])
        for done in range(step, n + 1, step):
            batch.iterations(step)
            for shape, (s, perm) in zip(shapes, members):
                check_state(s, perm, reference(shape, n)[done - 1], precision, f"batch member {shape} {precision}, {done} iterations in launches of {step}")
        lbs = batch.lower_bounds()
        for i, (shape, (s, perm)) in enumerate(zip(shapes, members)):
            assert lbs[i] == s.lower_bound()
            check_min_marginals(s, perm, reference(shape, n)[n - 1], f"batch member {shape} {precision}")
        batch.close()
        for s, _ in members:
            s.close()


# ---------------------------------------------------------------- exchange forms (rows of 2-10 / 2-6, counts {1, 2, 4}: sums of one, two and four terms)
# (the first three: the options of test_random_cover_vs_oracle; exchange_by_variable: 1 is the binned order, 2 the (variable, bdd) order)
EXCHANGE = [("atomics-256_threads", "rows2_10", BOTH, dict(pack_width=128, waves_per_block=4, vars_per_bin=64), dict(kind="resident1", packs=9)),
            ("atomics-512_threads", "rows2_6_large", BOTH, dict(pack_width=128, waves_per_block=2, vars_per_bin=2048, pack_fill=64), dict(kind="resident1", packs=9)),
            ("atomics-1024_threads", "rows2_6_large", BOTH, dict(pack_width=128, waves_per_block=1, vars_per_bin=8192), dict(kind="resident1", packs=9)),
            ("atomics-default_bins", "rows2_6_large", BOTH, dict(), dict(kind="resident2", packs=9)),
            ("deterministic", "rows2_10", BOTH, dict(deterministic=True), dict(kind="resident2", packs=9)),
            ("deterministic-1024_threads", "rows2_6_large", BOTH, dict(deterministic=True, vars_per_bin=8192), dict(kind="resident2", packs=9)),
            ("binned_order", "rows2_10", BOTH, dict(exchange_by_variable=1), dict(kind="resident2", packs=9)),
            ("by_variable", "rows2_10", BOTH, dict(exchange_by_variable=2), dict(kind="resident2", packs=9)),
            ("by_variable-large", "rows2_6_large", BOTH, dict(exchange_by_variable=2), dict(kind="resident2", packs=9))]


@pytest.mark.parametrize("shape,precision,opts,path", params(EXCHANGE))
def test_exchange_forms(shape, precision, opts, path):
    drive(shape, precision, opts, path)
