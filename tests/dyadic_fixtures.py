"""Fixtures on which the arithmetic of the forward solver is exact, for tests/test_dyadic_fixtures.py (CPU) and
tests/test_gpu_dyadic_parity.py (GPU).

Integer costs in [-2, 2], omega = 1/2 and every variable in exactly 1, 2 or 4 BDDs: the initial arc costs are multiples of 1/4, a
min-marginal difference halves the grid step once per layer it passes, the average over a variable's BDDs divides by 1, 2 or 4 — every
cost, potential, difference and delta of an MMA iteration is a dyadic rational.  The forward solver only uses minima (no arg-min decides
anything), so while the largest |value| / grid step stays two bits under the mantissa every operation is exact in float32 and in float64
and every order of a sum gives the same bits: the double `Oracle` is then THE result, and a kernel of either precision has to reproduce it
bit for bit.  How many iterations that holds is measured per shape (largest_n), never chosen.

An instance: for occurrence r = 0, 1, 2, 3 the variables that sit in more than r BDDs are permuted and the permutation is cut into rows,
so that no variable repeats in a row and variable v sits in exactly counts[v % len(counts)] BDDs.  Test helper only."""
import zlib

import numpy as np

from bdd_amd import BddCollection
from exact_fixtures import certificate
from oracle.oracle import Oracle

COST_RANGE = 2
HEADROOM = {"float": 2.0 ** 22, "double": 2.0 ** 51}   # largest |value| / grid step: two bits under the mantissa — a sum of up to four terms
MAX_ITERATIONS = 16                                    # where the search for the largest n stops (no shape gets there)


def _uniform(lo, hi):
    """rows of lo ... hi variables that use up the permutation exactly"""
    def cut(n, rng):
        m = min(max(int(round(2 * n / (lo + hi))), -(-n // hi)), n // lo)   # rows: about n / the mean length, and such that m rows can hold n
        assert m >= 1 and m * lo <= n <= m * hi, (n, lo, hi)
        out, rem = [], n
        for left in range(m - 1, -1, -1):   # `left` rows follow this one: leave them lo ... hi variables each
            k = int(rng.integers(max(lo, rem - left * hi), min(hi, rem - left * lo) + 1))
            out.append(k)
            rem -= k
        assert rem == 0
        return out
    return cut


def _blocks(a, b, run):
    """`run` rows of a, `run` rows of b, ...: different hop counts in one workgroup"""
    def cut(n, rng):
        out, rem = [], n
        while rem:
            k = a if (len(out) // run) % 2 == 0 else b
            assert rem >= k, (n, a, b, rem)
            out.append(k)
            rem -= k
        return out
    return cut


# row builders, as the existing tests of each family build theirs.  The coefficients shape the BDD only; the arithmetic is in the costs.
def _covering(col, vs, rng):
    col.add_covering(vs)


def _simplex(col, vs, rng):
    col.add_simplex(vs)


def _either(col, vs, rng):
    (col.add_covering if rng.random() < 0.5 else col.add_simplex)(vs)


def _linear(top, sense, div):
    def add(col, vs, rng):
        co = rng.integers(1, top, size=len(vs))
        col.add_linear(co, sense, int(co.sum() // div), vs)
    return add


# shape: (variables, counts, [(row builder, cut) of occurrence r; the last one serves the further occurrences])
SHAPES = {
    # ---- short rows: what the on-chip, the streaming and the resident sweeps and the exchange forms serve
    "rows10": (2000, (2, 4), [(_either, _uniform(10, 10))]),              # 600 BDDs: ten 128-slot packs, the last partly filled
    "rows2_10": (2000, (1, 2, 4), [(_either, _uniform(2, 10))]),          # BDDs that end at different hops
    "rows11": (1320, (2, 4), [(_either, _uniform(11, 11))]),              # the lower edge of the 16-hop capacity
    "rows16": (2400, (2,), [(_either, _uniform(16, 16))]),
    "rows10_16": (1664, (2,), [(_either, _blocks(16, 10, 64))]),
    "rows17": (3400, (1, 2), [(_either, _uniform(17, 17))]),              # beyond the on-chip kernels' capacity
    # packs shorter than any look-ahead.  (No rows of one variable: such a row forces its variable, the min-marginal of the other side is
    # +inf, and there the GPU rule and the `Oracle` part ways on purpose — INTEGRATION.md, tests/test_gpu_cuda_rule.py.)
    "rows2": (240, (1, 2, 4), [(_covering, _uniform(2, 2))]),
    # more than 8 192 variables: full bins of the 512- / 1024-thread exchange.  (Rows of 2-10 at this size reach 2^23 grid steps after two
    # iterations with every seed tried — more values, a larger maximum —, rows of 2-6 stay within 2^22.)
    "rows2_6_large": (20000, (1, 2, 4), [(_either, _uniform(2, 6))]),
    # ---- one-workgroup instances: 1, 2 and 4 packs of 64 slots
    "assignment8": None,                                                  # every variable in a row and a column BDD
    "cover_small": (60, (1, 2, 4), [(_covering, _uniform(2, 6))]),
    "cover_small4": (180, (1, 2, 4), [(_either, _uniform(2, 6))]),
    # ---- long, wide and huge
    # 70-150 hops (several stage groups per pack, hop-window refills); the second occurrence of half the variables is in short rows: with long
    # rows in both, the grid refines by 25-35 bits in ONE iteration (a bit per layer passed) and not even one float iteration is exact
    "long": (16500, (1, 2), [(_either, _uniform(70, 150)), (_either, _uniform(2, 10))]),
    "rows17_60": (6000, (1, 2), [(_either, _uniform(17, 60)), (_either, _uniform(2, 10))]),   # resident packs of more than 16 hops
    "wide": (120, (2, 4), [(_linear(40, "<=", 2), _uniform(16, 21)), (_covering, _uniform(5, 5))]),
    "wide_staggered": (240, (2, 4), [(_linear(40, "<=", 2), _uniform(15, 19)), (_covering, _uniform(5, 5))]),
    "huge": (28, (2, 4), [(_linear(5000, "<=", 2), _uniform(28, 28)), (_linear(40, ">=", 3), _uniform(28, 28)), (_covering, _uniform(3, 9))]),
    "knapsack": (24, (2,), [(_linear(9, "<=", 2), _uniform(9, 14))]),
    "rows3_16": (600, (2, 4), [(_covering, _uniform(3, 16))]),            # packs of different lengths; chained with pack_stagger
}
LONG = ("long", "rows17_60", "wide", "wide_staggered", "huge")   # BDDs of more than 17 layers: the lower floors of tests/test_dyadic_fixtures.py
# shape: seed, where it is not 1 — the first seed from 1 on with which the reference alone meets every condition of
# tests/test_dyadic_fixtures.py (the floors of the headroom in most cases, a bound that rises in every iteration in the small ones)
SEEDS = {"rows10": 2, "rows11": 3, "rows10_16": 2, "rows2_6_large": 9, "cover_small": 6, "huge": 5, "knapsack": 3}

# (n_float, n_double) per shape: the largest n for which the reference alone — every array `reference` records, iterations 1 ... n —
# stays within HEADROOM.  Found by largest_n() below; tests/test_dyadic_fixtures.py::test_headroom recomputes every entry and compares.
ITERATIONS = {
    "rows10": (2, 5), "rows2_10": (2, 5), "rows11": (2, 5), "rows16": (2, 7), "rows10_16": (2, 6), "rows17": (2, 7), "rows2": (2, 7),
    "rows2_6_large": (2, 5), "assignment8": (4, 10), "cover_small": (2, 7), "cover_small4": (2, 7), "long": (2, 5), "wide": (1, 4),
    "wide_staggered": (2, 5), "huge": (1, 4), "knapsack": (4, 12), "rows3_16": (2, 7), "rows17_60": (2, 7),
}


def _assignment8(rng):
    col = BddCollection()
    n = 8
    for r in range(n):
        col.add_simplex(np.arange(r * n, (r + 1) * n))
    for c in range(n):
        col.add_simplex(np.arange(c, n * n, n))
    return col


def dyadic_rows(shape, seed=None):
    """(BddCollection, integer costs in [-2, 2] as float64) of the shape"""
    seed = SEEDS.get(shape, 1) if seed is None else seed
    rng = np.random.Generator(np.random.PCG64([seed, zlib.crc32(shape.encode())]))
    if SHAPES[shape] is None:
        col = _assignment8(rng)
    else:
        V, counts, occ = SHAPES[shape]
        count = np.asarray(counts)[np.arange(V) % len(counts)]
        col = BddCollection()
        for r in range(max(counts)):
            add, cut = occ[min(r, len(occ) - 1)]
            perm = rng.permutation(np.flatnonzero(count > r))
            at = 0
            for k in cut(len(perm), rng):
                add(col, np.sort(perm[at:at + k]), rng)
                at += k
            assert at == len(perm)
    costs = rng.integers(-COST_RANGE, COST_RANGE + 1, col.nr_variables()).astype(np.float64)
    return col, costs


# what `reference` records, by the oracle that computed it.  A grid step is a property of one computation's values: the oracle driven by
# iteration() and the one driven by explicit half-steps (whose delta is never divided, so its costs grow) share no value, and each gets
# its own certificate; the headroom of a shape is the larger of the two.  lb_per_bdd and min_marginals are path sums: with them inside,
# the certificate also covers the potentials the sweeps add up on the way.
ITERATION_ARRAYS = ("lo", "hi", "delta_in", "mm_last", "lb_per_bdd", "min_marginals")
HALF_STEP_ARRAYS = ("forward_delta", "backward_delta", "half_lo", "half_hi", "half_lb_per_bdd")
ARRAYS = ITERATION_ARRAYS + HALF_STEP_ARRAYS
_ROWS, _TRAJ = {}, {}


def rows(shape):
    if shape not in _ROWS:
        _ROWS[shape] = dyadic_rows(shape)
    return _ROWS[shape]


class _Trajectory:
    """the oracle's records per iteration, extended on demand and kept"""

    def __init__(self, shape, precision):
        col, costs = rows(shape)
        self.dtype = np.float64 if precision == "double" else np.float32
        self.o, self.marg, self.half = (Oracle(col, costs, precision) for _ in range(3))
        self.d = np.zeros(2 * self.o.nr_variables(), self.dtype)
        self.records = []
        self.initial = dict(lb_per_bdd=self.o.lower_bound_per_bdd(), bound=self.o.lower_bound())

    def upto(self, n):
        while len(self.records) < n:
            o, marg, half = self.o, self.marg, self.half
            o.iteration()
            lo, hi = o.get_costs()
            rec = dict(lo=lo, hi=hi, delta_in=o.delta_in(), mm_last=o.mm_last(), bound=o.lower_bound(), lb_per_bdd=o.lower_bound_per_bdd())
            marg.iteration()   # (a second oracle: min_marginals() runs a forward sweep over its potentials)
            rec["min_marginals"] = marg.min_marginals()
            half.forward_mm(0.5, self.d)
            rec["forward_delta"] = self.d.copy()
            half.backward_mm(0.5, self.d)
            rec["backward_delta"] = self.d.copy()
            rec["half_lo"], rec["half_hi"] = half.get_costs()
            rec["half_lb_per_bdd"] = half.lower_bound_per_bdd()
            self.records.append(rec)
        return self.records[:n]


def trajectory(shape, precision="double"):
    if (shape, precision) not in _TRAJ:
        _TRAJ[shape, precision] = _Trajectory(shape, precision)
    return _TRAJ[shape, precision]


def reference(shape, n, precision="double"):
    """the `Oracle`'s trajectory over n iterations: a list of n records dict(lo, hi, delta_in, mm_last, lb_per_bdd: the state after the
    iteration, BDD-major; bound; min_marginals: (n_layers, 2) from that state; forward_delta, backward_delta: the delta vectors of the
    explicit forward_mm(0.5, d) / backward_mm(0.5, d) of a second oracle driven by half-steps from d = 0; half_lo, half_hi,
    half_lb_per_bdd: that oracle's state after the two).  Computed once per shape."""
    return trajectory(shape, precision).upto(n)


def headrooms(shape, n):
    """[largest |value| / grid step over every recorded array of iterations 1 ... k] for k = 1 ... n"""
    q, top, out = [np.inf, np.inf], [0.0, 0.0], []
    for rec in reference(shape, n):
        if "certificate" not in rec:
            rec["certificate"] = [certificate([rec[k] for k in group]) for group in (ITERATION_ARRAYS, HALF_STEP_ARRAYS)]
        for g, (qi, hi) in enumerate(rec["certificate"]):
            q[g], top[g] = min(q[g], qi), max(top[g], hi * qi)
        out.append(max(top[0] / q[0], top[1] / q[1]))
    return out


def largest_n(shape):
    """(n_float, n_double): the largest n whose headroom is within HEADROOM, and the headrooms measured on the way"""
    seen = []
    n = {"float": 0, "double": 0}
    for k in range(1, MAX_ITERATIONS + 1):
        seen = headrooms(shape, k)
        for p in n:
            if seen[-1] <= HEADROOM[p]:
                n[p] = k
        if seen[-1] > HEADROOM["double"]:
            break
    return (n["float"], n["double"]), seen
