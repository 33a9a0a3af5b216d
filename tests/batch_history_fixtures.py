"""What tests/test_gpu_batch_history.py (GPU) and tests/test_batch_history_fixtures.py (CPU) share: the members of the history batches, their
inputs, and the decision margin that makes the double comparison of sol_avg on the set covers meaningful.

sol_avg averages 0 / 1 decisions.  In double, on a cover* member, the batch kernel's exchange adds a variable's terms in another order than the
per-member call's (tier 1: 1e-12 relative), so a decision could differ where the two path costs of an on-path node tie to within that
rounding.  The cost seeds used are therefore those — from 1 upwards — for which every on-path node of every tracked iteration decides with
a margin of at least REF_TOL["double"] (1e-9) times the larger of 1 and the largest cost magnitude: three orders above tier 1.  The margins
are computed with the NumPy restatement alone (tests/learned_mma_restatement.py); the CPU test asserts the table below.

Inputs are generated in BDD-major layer order (the restatement's) from the member's shape and cost seed, so that both tests see the same values; a
solver's public order maps to it through bdd_major_order()."""
import zlib

import numpy as np

from learned_mma_restatement import LearnedMma

NUM_ITR = 10
HISTORIES = (1, 2, 3, 10)
BETA = 0.7
OMEGA = 0.5
MARGIN = 1e-9   # REF_TOL["double"] of tests/test_gpu_small_learned.py

# cost seeds per shape (tests/test_gpu_small_learned.py: SHAPES gives the packs and the precisions).  assign*: every variable sits in two
# BDDs, both paths are bit-equal, any seed does.  cover*: the first seeds from 1 upwards that meet the margin in every tracked iteration of
# both input sets (scalar omega, omega_vec); REJECTED lists the ones that do not, with the iteration and margin that failed.
SEEDS = {"assign3": (1, 2), "assign8": (1, 2), "cover40x60": (1, 2), "cover67x100": (1, 2), "cover147x220": (1, 2), "cover200x300": (1, 2)}
REJECTED = {}


class LearnedMmaOv(LearnedMma):
    """the restatement with an omega per layer (BDD-major order) where omega is an array"""

    def _layer_mm(self, l, omega):
        return super()._layer_mm(l, omega[l] if np.ndim(omega) else omega)


def major_inputs(layer_var, name, seed, dtype):
    """(dist_weights, omega_vec) in BDD-major order for the member of shape `name` and cost seed `seed`: Dirichlet weights per variable,
    omega in [0.1, 0.9)"""
    rng = np.random.default_rng([31, zlib.crc32(name.encode()), seed])
    layer_var = np.asarray(layer_var)
    w = np.zeros(layer_var.size)
    for v in np.unique(layer_var):
        idx = np.flatnonzero(layer_var == v)
        w[idx] = rng.dirichlet(np.ones(idx.size))
    return w.astype(dtype), rng.uniform(0.1, 0.9, layer_var.size).astype(dtype)


def member_keys(precision, shapes):
    """[(name, packs, seed)] of the history batch: the shapes interleaved, so that no launch group is contiguous in the caller's
    order (as member_set of tests/test_gpu_small_learned.py)"""
    out = []
    for k in range(max(len(s) for s in SEEDS.values())):
        for name, packs, fused_in, _ in shapes:
            if precision in fused_in and k < len(SEEDS[name]):
                out.append((name, packs, SEEDS[name][k]))
    return out


def decision_margins(col, costs, w, omega, num_itr=NUM_ITR):
    """per iteration: (the smallest |hi_path - lo_path| over the on-path nodes of every BDD's arg-min path, the largest finite arc-cost
    magnitude), in double, with the restatement"""
    m = LearnedMmaOv(col.instr, col.delims, "double")
    m.update_costs_hi(np.asarray(costs, np.float64))
    out = []
    for _ in range(num_itr):
        m.learned_iteration(w, omega)
        m.forward_run()
        margin = np.inf
        for b in range(m.n_bdds):
            l0, l1 = m.bdd_layer_ptr[b], m.bdd_layer_ptr[b + 1]
            u = m.layer_node_ptr[l0] if l0 < l1 else None
            for l in range(l0, l1):
                if u is None:
                    break
                assert m.layer_node_ptr[l] <= u < m.layer_node_ptr[l + 1]
                hi_path = m.F[u] + (m._Tc(m.hi_child[u]) + m.hi[l])
                lo_path = m.F[u] + (m._Tc(m.lo_child[u]) + m.lo[l])
                if np.isfinite(hi_path) and np.isfinite(lo_path):
                    margin = min(margin, abs(hi_path - lo_path))
                c = m.lo_child[u] if (hi_path - lo_path) > 0 else m.hi_child[u]
                u = c if c >= 0 else None
        finite = np.concatenate([m.lo[np.isfinite(m.lo)], m.hi[np.isfinite(m.hi)]])
        out.append((float(margin), float(np.abs(finite).max()) if finite.size else 0.0))
    return out
