"""CPU tests that pin the yardstick of tests/test_gpu_gradient_ties.py: on the fixtures of tests/exact_fixtures.py the restatements of the
gradient operators are exact — float32, float64 and longdouble give the same bits —, every value stays 4 bits under float32's mantissa,
a sizeable share of the deciding minima are exact ties, and the device's slot order inside a layer is the restatement's node order, so
that "lowest slot first" (include/bdd_mma.h) and "lowest node first" (the restatements) name the same node.  Each case prints its grid
step, headroom and tie shares (pytest -s)."""
import numpy as np
import pytest

from exact_fixtures import (HEADROOM, ITERATION_CASES, ITERATION_SEEDS, STATES, certificate, iterations_reference, model_of, recorded_values,
                            single_shot_reference, tie_share, tracked_mm)
from test_gpu_sum_marginals import CHAINED, FAMILIES, LAYOUT_OPTIONS, assert_chained_layout
from test_layout import Layout

TYPES = (np.float32, np.float64, np.longdouble)
GRADS = ("grad_lo", "grad_hi", "grad_mm", "grad_dist_weights", "grad_omega")
MIN_TIE_SHARE, MIN_MM_ZERO_SHARE = 0.05, 0.10


def _same_bits(a, b, what):
    """a (narrow type) and b (longdouble) hold the same numbers, infinities and NaNs included"""
    np.testing.assert_array_equal(np.asarray(a).astype(np.longdouble), np.asarray(b), err_msg=what)


def test_certificate():
    q, h = certificate([np.array([0.0, 3.0, -0.75, np.inf]), np.array([10.5])])
    assert (q, h) == (0.25, 42.0)
    assert certificate([np.zeros(3)]) == (1.0, 0.0)
    assert certificate([np.array([2.0 ** 30, 2.0 ** 31])]) == (2.0 ** 30, 2.0)
    assert certificate([np.array([1.0 + 2.0 ** -23])], np.float32) == (2.0 ** -23, 2.0 ** 23 + 1)
    assert certificate([np.array([1.0 + 2.0 ** -40])], np.float32) == (1.0, 1.0)   # taken in float32: the value it holds


@pytest.mark.parametrize("state", STATES)
@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_single_shot_fixture(family, state):
    refs = [single_shot_reference(family, state, dt) for dt in TYPES]
    wide = refs[-1]
    # (a) exact: every type gives the bits of longdouble
    for r, dt in zip(refs[:-1], TYPES):
        for k in ("mm_diff", "grad_lo", "grad_hi"):
            assert r[k].dtype == dt
            _same_bits(r[k], wide[k], f"{family} {state} {k} in {np.dtype(dt).name}")
    # (b) headroom: outputs and inputs on a grid q with |value| <= 2^20 q
    q, head = certificate([wide[k] for k in ("lo", "hi", "g", "mm_diff", "grad_lo", "grad_hi")])
    # (c) ties decide a sizeable share of the minima
    ties, decided = tie_share(wide["gaps"])
    print(f"{family} {state}: grid {q:g}, headroom {head:g} of {HEADROOM:g}; exact ties {ties} of {decided} deciding minima ({ties / max(decided, 1):.1%})")
    assert head <= HEADROOM
    assert decided > 0 and ties >= MIN_TIE_SHARE * decided
    if state == "zero_costs":
        assert ties == decided   # all costs zero: every finite minimum with a second candidate is a tie
    assert np.any(wide["grad_lo"] != 0) and np.any(wide["grad_hi"] != 0)


def test_every_family_has_iteration_seeds():
    assert set(ITERATION_SEEDS) == set(FAMILIES)
    assert [(f, ov) for f in sorted(FAMILIES) for ov in (False, True) if (f, ov) not in ITERATION_CASES] == [("chained_general", True)]


@pytest.mark.parametrize("family,omega_vec", ITERATION_CASES, ids=[f"{f}-{'omega_vec' if ov else 'omega'}" for f, ov in ITERATION_CASES])
def test_iterations_fixture(family, omega_vec):
    refs = [iterations_reference(family, omega_vec, dt) for dt in TYPES]
    wide = refs[-1]
    # (a) exact: the outputs, the start, the end and the trajectory after each tracked iteration
    for r, dt in zip(refs[:-1], TYPES):
        what = f"{family} {'omega_vec' if omega_vec else 'omega'} in {np.dtype(dt).name}"
        for i, nm in enumerate(GRADS):
            assert r["grads"][i].dtype == dt
            _same_bits(r["grads"][i], wide["grads"][i], f"{what}: {nm}")
        for i, nm in enumerate(("lo", "hi", "d")):
            _same_bits(r["start"][i], wide["start"][i], f"{what}: start {nm}")
            _same_bits(r["end"][i], wide["end"][i], f"{what}: end {nm}")
        for t, ((f, b), (fw, bw)) in enumerate(zip(r["records"], wide["records"])):
            for nm, x, y in (("lo", b["post"][0], bw["post"][0]), ("hi", b["post"][1], bw["post"][1]), ("mm", b["mm"], bw["mm"]),
                             ("forward pass mm", f["mm"], fw["mm"])):
                _same_bits(x, y, f"{what}: {nm} after tracked iteration {t}")
    # (b) headroom: all outputs (the scalar omega's sum too) and everything the reverse reads
    outputs = list(wide["grads"]) + ([] if omega_vec else [np.array([wide["grads"][4].sum()])])
    q, head = certificate(outputs + recorded_values(wide) + list(wide["end"]))
    # (c) ties decide a sizeable share of the trajectory's minima; mm = 0 in a sizeable share of the tracked layer-passes, both signs occur
    ties, decided = tie_share(wide["gaps"])
    mm = tracked_mm(wide)
    zero = int(np.sum(mm == 0))
    print(f"{family} {'omega_vec' if omega_vec else 'omega'}: grid {q:g}, headroom {head:g} of {HEADROOM:g}; exact ties {ties} of {decided} deciding "
          f"minima and signs ({ties / max(decided, 1):.1%}); mm == 0 in {zero} of {mm.size} tracked layer-passes ({zero / mm.size:.1%}), "
          f"mm > 0 in {int(np.sum(mm > 0))}, mm < 0 in {int(np.sum(mm < 0))}; largest |output| {max(float(np.abs(o).max()) for o in outputs):g}")
    assert head <= HEADROOM
    assert decided > 0 and ties >= MIN_TIE_SHARE * decided
    assert zero >= MIN_MM_ZERO_SHARE * mm.size and np.any(mm > 0) and np.any(mm < 0)
    assert all(np.any(g != 0) for g in wide["grads"])


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_the_two_restatements_agree_at_ties(family):
    """The reduction of tests/test_grad_iterations_restatement.py::test_reduction_to_the_single_shot_operator on a tied exact state, with
    equality instead of a rounding allowance: a pass that moves no cost (omega = 0, weights 0) reads the plain potentials of (lo, hi);
    reversed with multiplier 1/2 and grad_mm the only input, what reaches the costs is Gradients.grad_mm_diff applied to 1/2 of the gradient
    that reached each mm — the same seeds at the same tied arg-mins, routed by the same rule."""
    _, m = model_of(family)
    ref = iterations_reference(family, False)
    lo, hi, d = ref["start"]
    R = np.float64
    m._setup(R)
    zero, om0, om = np.zeros(m.n_layers), np.zeros(m.n_layers), np.full(m.n_layers, 0.5)
    f = m.forward_pass_rec(lo, hi, d, zero, om0, R)
    b = m.backward_pass_rec(f["post"][0], f["post"][1], f["mm"], f["F"], zero, om0, R)
    np.testing.assert_array_equal(b["post"][0], lo)
    np.testing.assert_array_equal(b["post"][1], hi)
    gaps = []
    o_lo, o_hi, gd, gF, _, _ = m.reverse_backward_pass(b, zero, zero, ref["x"]["g_mm"], np.zeros(m.n_nodes), zero, om, R, gaps)
    dmm = m.last_dmm.copy()
    o_lo, o_hi, _, gT, _, _ = m.reverse_forward_pass(f, o_lo, o_hi, zero, gF, zero, om0, R, gaps)
    assert not gT.any() and not gd.any()
    m.lo, m.hi = lo.copy(), hi.copy()
    s_lo, s_hi = m.grad_mm_diff(0.5 * dmm, R)
    ties, decided = tie_share(gaps)
    print(f"{family}: exact ties {ties} of {decided} deciding minima and signs")
    assert ties >= MIN_TIE_SHARE * decided
    np.testing.assert_array_equal(o_lo, s_lo)
    np.testing.assert_array_equal(o_hi, s_hi)


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_slot_order_is_node_order(family):
    """the slots of a layer hold increasing instruction indices, in the layout the family's options give: the lowest slot of a tie is the
    restatement's lowest node, and a node's parents by slot are its parents by node"""
    col, _ = model_of(family)
    lay = Layout(col, **{k: v for k, v in FAMILIES[family][1].items() if k in LAYOUT_OPTIONS})
    by_layer = {}
    for slot, (_, _, layer, _, _) in lay.decode().items():
        by_layer.setdefault(layer, []).append(slot)
    assert len(by_layer) == lay.n_layers
    widest = 0
    for layer, slots in by_layer.items():
        slots.sort()
        instr = lay.slot_to_instr[slots].astype(np.int64)
        assert np.all(np.diff(instr) > 0), (family, layer, instr[:8])
        widest = max(widest, len(slots))
    print(f"{family}: {lay.n_layers} layers, widest {widest} slots ({-(-widest // 16)} runs of 16), packs narrow / wide / huge {lay.np_n} / {lay.np_w} / {lay.np_h}")


@pytest.mark.parametrize("family", sorted(CHAINED))
def test_chained_families_are_chained(family):
    """the families that stand for chained packs get them from the layout: the recorded hops of every pack, a pack with more hops than the
    longest BDD has layers (a BDD starts below its first hop) and, with wide packs, fewer of them than wide BDDs; side by side without
    pack_stagger.  The GPU tests assert the same, and the kind of the solve sweeps, on the solvers they build (assert_chained)."""
    col, _ = model_of(family)
    opts = {k: v for k, v in FAMILIES[family][1].items() if k in LAYOUT_OPTIONS}
    assert opts.get("pack_stagger", 0) >= 2
    assert_chained_layout(family, col, Layout(col, **opts))
    with pytest.raises(AssertionError):
        assert_chained_layout(family, col, Layout(col, **dict(opts, pack_stagger=0)))
