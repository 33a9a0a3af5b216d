"""NumPy restatement of sum-marginals (bdd_cuda_base<REAL>::sum_marginals_cuda, src/bdd_solver/bdd_cuda_base.cu:788-1025 of the reference)
and the smooth solution (:1027-1064) for the tests, hop-free: per BDD in topological order, in the log domain, in any NumPy float type
(float32 / float64 / longdouble).  Layers are in BDD-major order as in learned_mma_restatement.py, whose parsing of a bdd_collection it
reuses; a solver's public layer order maps to it through bdd_hip_parallel_mma.bdd_major_order().

    sm_lo[l] = log sum over the root -> top paths of the layer's BDD that take a lo arc in layer l of exp(-cost(path))     (sm_hi: hi arc)

Also here: brute-force enumeration of all assignments of a BDD (the yardstick's yardstick) and the path counts through each arc.
Test helper only: Python loops over nodes."""
import numpy as np

from learned_mma_restatement import BOT, TOP, LearnedMma


class SumMarginals(LearnedMma):
    def log_sum_marginals(self, dtype=None):
        """(sm_lo, sm_hi) per layer, BDD-major, computed in `dtype` (default: the model's precision) from self.lo / self.hi"""
        R = np.dtype(dtype or self.dt).type
        ninf = R(-np.inf)
        lo, hi = self.lo.astype(R), self.hi.astype(R)
        F = np.full(self.n_nodes, ninf, R)
        T = np.full(self.n_nodes, ninf, R)
        for b in range(self.n_bdds):
            if self.bdd_layer_ptr[b] < self.bdd_layer_ptr[b + 1]:
                F[self.layer_node_ptr[self.bdd_layer_ptr[b]]] = R(0)
        with np.errstate(invalid="ignore"):
            for l in range(self.n_layers):
                for u in range(self.layer_node_ptr[l], self.layer_node_ptr[l + 1]):
                    for c, cost in ((self.lo_child[u], lo[l]), (self.hi_child[u], hi[l])):
                        if c >= 0:
                            F[c] = np.logaddexp(F[c], F[u] - cost)

            def Tc(c):
                return R(0) if c == TOP else ninf if c == BOT else T[c]

            sm_lo = np.full(self.n_layers, ninf, R)
            sm_hi = np.full(self.n_layers, ninf, R)
            for l in range(self.n_layers - 1, -1, -1):
                for u in range(self.layer_node_ptr[l], self.layer_node_ptr[l + 1]):
                    a, b = Tc(self.lo_child[u]) - lo[l], Tc(self.hi_child[u]) - hi[l]
                    T[u] = np.logaddexp(a, b)
                    sm_lo[l] = np.logaddexp(sm_lo[l], F[u] + a)
                    sm_hi[l] = np.logaddexp(sm_hi[l], F[u] + b)
        return sm_lo, sm_hi

    @staticmethod
    def smooth_solution(sm_lo, sm_hi):
        """ComputeSmoothSolution (:1027-1048) of log sum-marginals, in their type; 0.5 where both are -inf"""
        sm_lo, sm_hi = np.asarray(sm_lo), np.asarray(sm_hi)
        c = np.maximum(sm_lo, sm_hi)
        fin = np.isfinite(c)
        cs = np.where(fin, c, 0)
        e_lo, e_hi = np.exp(sm_lo - cs), np.exp(sm_hi - cs)
        with np.errstate(invalid="ignore"):
            return np.where(fin, e_hi / (e_lo + e_hi), sm_lo.dtype.type(0.5))

    # ---- brute force and path counts (float64)
    def brute_force(self, b):
        """probabilities (not logs) (p_lo, p_hi) of the layers of BDD b by enumeration of all 2^k assignments of its k layers: every assignment
        is walked from the root; it counts if it ends in the top sink.  Requires that no arc skips a layer (the collections here are
        quasi-reduced), so that assignments and root -> top paths are the same thing."""
        l0, l1 = self.bdd_layer_ptr[b], self.bdd_layer_ptr[b + 1]
        k = l1 - l0
        assert 0 < k <= 19
        N = 1 << k
        x = (np.arange(N)[:, None] >> np.arange(k)[None, :]) & 1   # assignment i takes arc x[i, j] in layer l0 + j
        node = np.full(N, self.layer_node_ptr[l0], np.int64)
        cost = np.zeros(N)
        lo_child, hi_child = np.asarray(self.lo_child, np.int64), np.asarray(self.hi_child, np.int64)
        for j in range(k):
            l = l0 + j
            alive = node >= 0
            assert np.all((node[alive] >= self.layer_node_ptr[l]) & (node[alive] < self.layer_node_ptr[l + 1])), "an arc skips a layer"
            take_hi = x[:, j] == 1
            cost = cost + np.where(take_hi, float(self.hi[l]), float(self.lo[l]))
            nxt = np.where(take_hi, hi_child[np.maximum(node, 0)], lo_child[np.maximum(node, 0)])
            assert not np.any(alive & (nxt == TOP)) or j == k - 1, "a path reaches the top sink early"
            node = np.where(alive, nxt, BOT)
        w = np.where(node == TOP, np.exp(-cost), 0.0)
        p_lo = np.array([w[x[:, j] == 0].sum() for j in range(k)])
        p_hi = np.array([w[x[:, j] == 1].sum() for j in range(k)])
        return p_lo, p_hi

    def path_counts(self):
        """number of root -> top paths through the lo / hi arcs of every layer (what the sum-marginal probabilities are at cost 0)"""
        F = np.zeros(self.n_nodes)
        T = np.zeros(self.n_nodes)
        for b in range(self.n_bdds):
            if self.bdd_layer_ptr[b] < self.bdd_layer_ptr[b + 1]:
                F[self.layer_node_ptr[self.bdd_layer_ptr[b]]] = 1
        for u in range(self.n_nodes):
            for c in (self.lo_child[u], self.hi_child[u]):
                if c >= 0:
                    F[c] += F[u]
        n_lo, n_hi = np.zeros(self.n_layers), np.zeros(self.n_layers)
        for l in range(self.n_layers - 1, -1, -1):
            for u in range(self.layer_node_ptr[l], self.layer_node_ptr[l + 1]):
                a = 1.0 if self.lo_child[u] == TOP else 0.0 if self.lo_child[u] == BOT else T[self.lo_child[u]]
                b = 1.0 if self.hi_child[u] == TOP else 0.0 if self.hi_child[u] == BOT else T[self.hi_child[u]]
                T[u] = a + b
                n_lo[l] += F[u] * a
                n_hi[l] += F[u] * b
        return n_lo, n_hi

    def layer_bdd(self):
        out = np.zeros(self.n_layers, np.int64)
        for b in range(self.n_bdds):
            out[self.bdd_layer_ptr[b]:self.bdd_layer_ptr[b + 1]] = b
        return out


# ---- instances of the sum-marginal tests (CPU and GPU)
def cover10(seed=5, V=500, rows=1500):
    from bdd_amd import BddCollection
    rng = np.random.Generator(np.random.PCG64(seed))
    col = BddCollection()
    for _ in range(rows):
        col.add_covering(np.sort(rng.choice(V, size=10, replace=False)))
    return col, rng.normal(0, 3, col.nr_variables()).round(3)


def assignment8():
    from bdd_amd import to_bdd_collection
    from bdd_amd.instances import assignment_ilp
    ilp = assignment_ilp(8, None)
    return to_bdd_collection(ilp), np.asarray(ilp.objective, np.float64)


def knapsack_rows(seed=3):
    """general linear rows whose BDDs have layers wider than two nodes, <= 14 variables each"""
    from bdd_amd import BddCollection
    rng = np.random.Generator(np.random.PCG64(seed))
    col = BddCollection()
    V = 24
    for k in (9, 12, 14, 11):
        vs = np.sort(rng.choice(V, size=k, replace=False))
        co = rng.integers(1, 9, size=k)
        col.add_linear(co, "<=", int(co.sum() // 2), vs)
    assert max(max(col.layer_widths(b)) for b in range(col.nr_bdds())) > 2
    return col, rng.normal(0, 2, col.nr_variables()).round(3)


def wide_rows(seed=21):
    """six knapsack rows of 16-21 variables (wide packs) and 30 covering rows (narrow packs)"""
    from bdd_amd import BddCollection
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


def general_rows(seed=77):
    """the instance of tests/test_layout.py::test_roundtrip_chained_packs: 14 knapsack rows of 15-19 variables (layers of 59-135 nodes: wide
    packs at pack width 64), 30 of 8-12 variables (layers of up to ~40 nodes: narrow packs) and 40 covering rows of 5 — with pack_stagger
    several chained packs of both kinds"""
    from bdd_amd import BddCollection
    rng = np.random.Generator(np.random.PCG64(seed))
    col = BddCollection()
    V = 60
    for lo_k, hi_k, top, n in ((15, 20, 40, 14), (8, 13, 12, 30)):
        for _ in range(n):
            k = int(rng.integers(lo_k, hi_k))
            co = rng.integers(1, top, size=k)
            col.add_linear(co, "<=", int(co.sum() // 2), np.sort(rng.choice(V, size=k, replace=False)))
    for _ in range(40):
        col.add_covering(np.sort(rng.choice(V, size=5, replace=False)))
    return col, rng.normal(0, 3, col.nr_variables()).round(3)


def huge_rows():
    """a knapsack row of 28 variables with a layer wider than 2048 nodes (a huge pack), covering rows and a second long row"""
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


def two_simplex():
    from bdd_amd import native
    col = native.lp_to_bdd_collection(TWO_SIMPLEX_LP)
    return col, np.asarray(native.parse_lp(TWO_SIMPLEX_LP).objective, np.float64)


def restatement_of(col, costs, precision="double"):
    m = SumMarginals(col.instr, col.delims, precision)
    m.update_costs_hi(np.asarray(costs, np.float64))
    return m


TWO_SIMPLEX_LP = """Minimize
2 x_1 + 3 x_2 + 4 x_3
+1 x_4 + 2 x_5 - 1 x_6
Subject To
x_1 + x_2 + x_3 = 2
x_4 + x_5 + x_6 = 1
End"""
E = np.exp
# test/test_bdd_cuda_sum_marginals.cpp of the reference, two_simplex_problem: (lo, hi) probabilities of variables 0..5
TWO_SIMPLEX_CLOSED_FORMS = [
    (E(-3 - 4), E(-2 - 3) + E(-2 - 4)), (E(-2 - 4), E(-3 - 2) + E(-3 - 4)), (E(-2 - 3), E(-4 - 2) + E(-4 - 3)),
    (E(-2) + E(1), E(-1.0)), (E(-1) + E(+1), E(-2.0)), (E(-1) + E(-2), E(1.0)),
]
