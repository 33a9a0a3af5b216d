"""Fixtures on which the arithmetic of the gradient operators is exact, for tests/test_exact_fixtures.py (CPU) and
tests/test_gpu_gradient_ties.py (GPU).

Small integer arc costs, integer incoming gradients, integer distribution weights and omega in {1, 1/2}: every potential, path value,
difference and gradient is then a dyadic rational far below 2^24 grid steps, which float32 holds exactly, and every sum is exact in any
order.  Two implementations of the operators then agree bit for bit, in float and in double, if and only if they take the same arg-mins —
and with integer costs a large share of the deciding minima are exact ties, so the published tie rule (include/bdd_mma.h: lowest slot
first among a layer's nodes, first in parent table order among a node's parents, lo before hi, `>= 0` takes the hi side) decides them.

The references are the NumPy restatements tests/grad_restatement.py and tests/grad_iterations_restatement.py; they are computed once per
(instance, state, type) and shared by every test that needs them (the three cover10 families are one instance).  Test helper only."""
import numpy as np

from grad_iterations_restatement import grad_iterations_of
from test_gpu_sum_marginals import FAMILIES

COST_RANGE, GRAD_RANGE, WEIGHT_RANGE = 2, 3, 2   # lo / hi in [-2, 2], incoming gradients in [-3, 3], weights in {0, 1, 2}
GRAD_RANGE_OMEGA_VEC, HALF_SHARE = 1, 0.25       # with omega_vec: incoming gradients in [-1, 1], omega_vec = 1/2 on a quarter of the layers
UNTRACKED, TRACKED = 1, 2                        # the learned iterations: one untracked, then two tracked, from d = 0
HEADROOM = 2.0 ** 20                             # largest allowed |value| / grid step: 4 bits under float32's 2^24
STATE_SEEDS = (1, 2)                             # exact_state seeds of the single-shot comparison
# exact_iteration_inputs seeds per family, (scalar omega, omega_vec): the first seed from 1 on for which the restatement alone meets the
# conditions of tests/test_exact_fixtures.py::test_iterations_fixture (exact in float32, headroom, tie share, mm = 0 share, both signs of mm)
ITERATION_SEEDS = {"assignment8": (3, 1), "cover10_w64": (2, 2), "cover10_w128": (2, 2), "cover10_w256": (2, 2), "huge": (1, 1), "knapsack_w64": (1, 1),
                   "mixed": (1, 2), "split_bdds": (1, 1), "staggered_rows": (1, 1), "wide2": (1, 2),
                   # the chained families: the instance, and so the seeds, of staggered_rows, knapsack_w64 and mixed.  chained_general with omega_vec:
                   # no seed in 1..32 keeps the headroom (the closest, seed 6, exceeds it 1.5 times, the others 1.9 to 325 times): that form is left out (None)
                   "chained_rows": (1, 1), "chained_knapsack": (1, 1), "chained_wide": (1, 2), "chained_wide2": (1, 2), "chained_general": (1, None)}
ITERATION_CASES = [(f, ov) for f in sorted(ITERATION_SEEDS) for ov in (False, True) if ITERATION_SEEDS[f][ov] is not None]
STATES = tuple(f"seed{s}" for s in STATE_SEEDS) + ("zero_costs",)


def exact_state(m, seed):
    """(lo, hi, g) for a model with m.n_layers layers (BDD-major): integers in [-2, 2], [-2, 2] and [-3, 3], as float64"""
    rng = np.random.Generator(np.random.PCG64(seed))
    lo, hi = (rng.integers(-COST_RANGE, COST_RANGE + 1, m.n_layers).astype(np.float64) for _ in range(2))
    g = rng.integers(-GRAD_RANGE, GRAD_RANGE + 1, m.n_layers).astype(np.float64)
    return lo, hi, g


def zero_cost_state(m, seed=9):
    """(lo, hi, g): all-zero costs — every finite minimum is a tie, the result is decided by the rule alone — and a Gaussian g rounded to
    multiples of 2^-8"""
    rng = np.random.Generator(np.random.PCG64(seed))
    z = np.zeros(m.n_layers)
    return z, z.copy(), np.round(rng.normal(0, 1, m.n_layers) * 256.0) / 256.0


def exact_iteration_inputs(m, seed, omega_vec):
    """dict(lo, hi, alpha, omega, omega_vec, g_lo, g_hi, g_mm) in float64, BDD-major: integer costs, weights and incoming gradients; omega = 1
    and omega_vec None, or (omega_vec true) one omega per layer from {0.5, 1} and omega None.
    Every factor 1/2 a value passes halves its grid step — once per pass for the costs, once per layer of a BDD for what the reverse hands
    down through the potentials — and grad_omega and grad_dist_weights are products of two such values.  So that everything stays within
    HEADROOM grid steps, a quarter of the layers get 1/2 and the incoming gradients are narrowed to [-1, 1] with omega_vec (with 1/2 on half
    of the layers and gradients in [-3, 3] the split BDDs reach 2^27 grid steps, the covering rows 2^21)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    L = m.n_layers
    gr = GRAD_RANGE_OMEGA_VEC if omega_vec else GRAD_RANGE
    lo, hi = (rng.integers(-COST_RANGE, COST_RANGE + 1, L).astype(np.float64) for _ in range(2))
    g_lo, g_hi, g_mm = (rng.integers(-gr, gr + 1, L).astype(np.float64) for _ in range(3))
    alpha = rng.integers(0, WEIGHT_RANGE + 1, L).astype(np.float64)
    ov = np.where(rng.random(L) < HALF_SHARE, 0.5, 1.0)
    return dict(lo=lo, hi=hi, alpha=alpha, omega=None if omega_vec else 1.0, omega_vec=ov if omega_vec else None, g_lo=g_lo, g_hi=g_hi, g_mm=g_mm)


def grid_step(values):
    """the largest power of two that divides every finite non-zero value (1 when there is none)"""
    x = np.abs(np.asarray(values, np.longdouble).ravel())
    x = x[np.isfinite(x) & (x > 0)]
    if not x.size:
        return 1.0
    mant, exp = np.frexp(x)                       # x = mant * 2^exp, mant in [0.5, 1)
    n = np.ldexp(mant, 64).astype(np.uint64)      # a 64-bit integer mantissa holds every type up to the x87 long double
    low = n & (~n + np.uint64(1))                 # its lowest set bit
    tz = np.log2(low.astype(np.longdouble)).astype(np.int64)
    return float(np.ldexp(1.0, int(np.min(exp.astype(np.int64) - 64 + tz))))


def certificate(arrays, dt=np.longdouble):
    """(q, headroom) of the values of `arrays` taken in type dt: q the grid step (the largest power of two that divides every finite value)
    and headroom = the largest finite |value| / q.  headroom <= 2^24 means float32 holds every value, and every partial sum of values
    whose magnitudes add up to that bound, exactly."""
    x = np.concatenate([np.asarray(a).astype(dt).ravel().astype(np.longdouble) for a in arrays]) if len(arrays) else np.zeros(0, np.longdouble)
    x = x[np.isfinite(x)]
    q = grid_step(x)
    return q, float(np.abs(x).max(initial=0.0) / q)


def on_grid(value, q):
    v = float(value)
    return bool(np.isfinite(v) and v / q == np.floor(v / q))


# ---- models and references, computed once
_MODELS, _SINGLE, _ITER = {}, {}, {}


def model_of(family):
    """(collection, restatement model) of the family's instance; the three cover10 families share one"""
    make = FAMILIES[family][0]
    if make not in _MODELS:
        col, _ = make()
        _MODELS[make] = (col, grad_iterations_of(col, "double"))
    return _MODELS[make]


def state_of(m, state):
    return zero_cost_state(m) if state == "zero_costs" else exact_state(m, int(state[4:]))


def single_shot_reference(family, state, dtype=np.float64):
    """dict(lo, hi, g: the state; mm_diff, grad_lo, grad_hi: the restatement in `dtype`; gaps: its decision records), BDD-major"""
    key = (FAMILIES[family][0], state, np.dtype(dtype))
    if key not in _SINGLE:
        _, m = model_of(family)
        lo, hi, g = state_of(m, state)
        m.lo, m.hi = lo.copy(), hi.copy()
        gaps = []
        mm = m.mm_diff(dtype)
        g_lo, g_hi = m.grad_mm_diff(g, dtype, gaps)
        _SINGLE[key] = dict(lo=lo, hi=hi, g=g, mm_diff=mm, grad_lo=g_lo, grad_hi=g_hi, gaps=gaps[m.n_bdds:])   # (the first n_bdds records are magnitudes)
    return _SINGLE[key]


def iterations_reference(family, omega_vec, dtype=np.float64):
    """dict(x: the inputs; start: (lo, hi, d) after the untracked iteration; records: (forward pass, backward pass) per tracked iteration;
    end: (lo, hi, d) after all iterations; grads: the five outputs of grad_iterations from `start`; gaps: its decision records), in `dtype`"""
    key = (FAMILIES[family][0], bool(omega_vec), np.dtype(dtype))
    if key not in _ITER:
        _ITER[key] = iterations_of(model_of(family)[1], ITERATION_SEEDS[family][bool(omega_vec)], omega_vec, dtype)
    return _ITER[key]


def iterations_of(m, seed, omega_vec, dtype):
    x = exact_iteration_inputs(m, seed, omega_vec)
    omega = x["omega_vec"] if omega_vec else x["omega"]
    start = m.iterate(x["lo"], x["hi"], np.zeros(m.n_layers), x["alpha"], omega, UNTRACKED, dtype)
    records, gaps = [], []
    end = m.iterate(*start, x["alpha"], omega, TRACKED, dtype, records)
    grads = m.grad_iterations(*start, x["alpha"], omega, TRACKED, x["g_lo"], x["g_hi"], x["g_mm"], dtype, gaps)
    return dict(x=x, start=start, records=records, end=end, grads=grads, gaps=gaps)


def tie_share(gaps):
    """(exact ties, deciding minima) of decision records (bdd, gap, magnitude): a record decides something when a second candidate exists
    (finite gap); it is a tie when the gap is 0"""
    gap = np.array([g for _, g, _ in gaps], np.float64)
    return int(np.sum(gap == 0)), int(np.sum(np.isfinite(gap)))


def recorded_values(ref):
    """every array the reverse of the tracked iterations reads: pre, post, F, T, mm, S of each recorded pass"""
    out = []
    for passes in ref["records"]:
        for p in passes:
            out += [p["pre"][0], p["pre"][1], p["post"][0], p["post"][1], p["F"], p["T"], p["mm"], p["S"]]
    return out


def tracked_mm(ref):
    return np.concatenate([p["mm"] for passes in ref["records"] for p in passes])
