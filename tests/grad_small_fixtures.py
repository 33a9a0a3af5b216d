"""The shapes and exact fixtures of the batch backward of the learned iterations (bddmma_grad_learned_iterations_batch), for
tests/test_grad_small_fixtures.py (CPU) and tests/test_gpu_grad_small.py (GPU).

Shapes: those of tests/test_gpu_small_learned.py — 1, 2, 4, 7 and 10 packs, the 81 variables of assign9 on one wave — and `mixed3x9`: 70
covering rows of 3 variables and 70 of 9 over 120 variables, which the layout packs into three packs of 9 hops and two of 3, so that the
waves of one workgroup run reverse sweeps of different lengths.  (A pack in which a BDD starts below the pack's first hop — a staggered
pack, PackDev::hop_root — is not admitted by the one-workgroup kernels at all: their resident headers exist only without staggered packs,
so there is no such shape to add.)

Exact fixtures: tests/exact_fixtures.py's inputs (integer costs, weights and gradients, omega 1 or an omega_vec from {1/2, 1}) on these
shapes, with the restatement tests/grad_iterations_restatement.py as the reference, computed once per (shape, form of omega, counts, type).
EXACT_SEEDS holds per shape the first seed from 1 on for which the restatement alone meets the conditions that
tests/test_grad_small_fixtures.py asserts.  Test helper only."""
import numpy as np

from bdd_amd.bdd_collection import BddCollection
from exact_fixtures import HEADROOM, certificate, exact_iteration_inputs, recorded_values, tie_share, tracked_mm
from grad_iterations_restatement import grad_iterations_of
from test_gpu_small_learned import ASSIGN9, SHAPES as LEARNED_SHAPES, instance as learned_instance

MIXED = "mixed3x9"
# (name, packs, precisions it is fused in)
SHAPES = [(name, packs, fused_in) for name, packs, fused_in, _ in LEARNED_SHAPES + [ASSIGN9]] + [(MIXED, 5, ("float", "double"))]
PACKS = {name: packs for name, packs, _ in SHAPES}
MIN_TIE_SHARE = 0.20
# exact_iteration_inputs seeds, (scalar omega, omega_vec), for 1 untracked + 2 tracked iterations
EXACT_SEEDS = {"assign3": (1, 1), "assign8": (3, 1), "assign9": (1, 1), "cover40x60": (1, 1), "cover67x100": (1, 1), "cover147x220": (1, 2),
               "cover200x300": (1, 2), MIXED: (1, 4)}
# 2 untracked + 5 tracked, scalar omega: the covers leave the headroom (they reach 2^31 grid steps)
EXACT_LONG = {"assign8": 3, "assign3": 1}
_COLS, _MODELS, _REFS = {}, {}, {}


def mixed_rows_cover(n_vars=120, n3=70, n9=70, seed=7):
    """covering rows of 3 and of 9 distinct variables; costs U(1, 10)"""
    rng = np.random.Generator(np.random.PCG64(seed))
    col = BddCollection()
    for cnt, k in ((n3, 3), (n9, 9)):
        rows = np.sort(rng.integers(0, n_vars, size=(cnt, k), dtype=np.int64), axis=1)
        while True:
            dup = (rows[:, 1:] == rows[:, :-1]).any(axis=1)
            if not dup.any():
                break
            rows[dup] = np.sort(rng.integers(0, n_vars, size=(int(dup.sum()), k), dtype=np.int64), axis=1)
        col.add_covering(rows.astype(np.uint64))
    return col, rng.uniform(1.0, 10.0, size=n_vars)


def instance(name, seed=1):
    """(collection, costs of `seed`), as tests/test_gpu_small_learned.py::instance"""
    if name != MIXED:
        return learned_instance(name, seed if name != "assign9" else 0)
    if name not in _COLS:
        _COLS[name] = mixed_rows_cover()
    col, costs = _COLS[name]
    return col, costs * np.random.default_rng(1000 + seed).uniform(0.5, 1.5, size=costs.shape)


def pack_hops(col):
    """hops of every narrow pack of the collection's default layout (the Python mirror of the layout builder)"""
    from test_layout import Layout
    return [int(h) for h in np.asarray(Layout(col).pack_hdr).reshape(-1, 8)[:, 5] & 0xFFFF]


def model_of(name):
    if name not in _MODELS:
        _MODELS[name] = grad_iterations_of(instance(name)[0], "double")
    return _MODELS[name]


def exact_reference(name, seed, omega_vec, untracked=1, tracked=2, dtype=np.float64):
    """dict(x: the inputs; start / end: (lo, hi, d) before / after the tracked iterations; records; grads: the five outputs; gaps), BDD-major, in
    `dtype`: exact_fixtures.iterations_of with the counts as arguments"""
    key = (name, seed, bool(omega_vec), untracked, tracked, np.dtype(dtype))
    if key not in _REFS:
        m = model_of(name)
        x = exact_iteration_inputs(m, seed, omega_vec)
        omega = x["omega_vec"] if omega_vec else x["omega"]
        start = m.iterate(x["lo"], x["hi"], np.zeros(m.n_layers), x["alpha"], omega, untracked, dtype)
        records, gaps = [], []
        end = m.iterate(*start, x["alpha"], omega, tracked, dtype, records)
        grads = m.grad_iterations(*start, x["alpha"], omega, tracked, x["g_lo"], x["g_hi"], x["g_mm"], dtype, gaps)
        _REFS[key] = dict(x=x, start=start, records=records, end=end, grads=grads, gaps=gaps)
    return _REFS[key]


def fixture_figures(name, seed, omega_vec, untracked=1, tracked=2):
    """dict(exact: float32 gives longdouble's bits on the five outputs and the end state; q, headroom: exact_fixtures.certificate of the
    per-layer outputs, everything the reverse reads and the end state; omega_sum: |the scalar omega's sum| in grid steps; ties, decided; pos,
    neg: tracked mm of each sign)"""
    wide = exact_reference(name, seed, omega_vec, untracked, tracked, np.longdouble)
    low = exact_reference(name, seed, omega_vec, untracked, tracked, np.float32)
    exact = all(np.array_equal(np.asarray(a).astype(np.longdouble), np.asarray(b)) for a, b in zip(list(low["grads"]) + list(low["end"]), list(wide["grads"]) + list(wide["end"])))
    q, head = certificate(list(wide["grads"]) + recorded_values(wide) + list(wide["end"]))
    ties, decided = tie_share(wide["gaps"])
    mm = tracked_mm(wide)
    omega_sum = 0.0 if omega_vec else float(abs(wide["grads"][4].sum()) / q)
    return dict(exact=exact, q=q, headroom=head, omega_sum=omega_sum, ties=ties, decided=decided, pos=int(np.sum(mm > 0)), neg=int(np.sum(mm < 0)))


def meets_conditions(f):
    """exact in float32; at most HEADROOM grid steps; the scalar omega's sum — formed in double on the device, rounded once — within float32's
    2^24; at least MIN_TIE_SHARE of the deciding minima exact ties; both signs of mm"""
    return (f["exact"] and f["headroom"] <= HEADROOM and f["omega_sum"] <= 2.0 ** 24 and f["decided"] > 0 and f["ties"] >= MIN_TIE_SHARE * f["decided"]
            and f["pos"] > 0 and f["neg"] > 0)
