"""NumPy restatement of the single-shot backward operators of the learned solver (bdd_cuda_learned_mma<REAL>: grad_mm_diff_all_hops,
grad_lower_bound_per_bdd, grad_distribute_delta, grad_cost_perturbation; src/bdd_solver/bdd_cuda_learned_mma.cu:387-416, 623-1187 of the
reference) for the tests, hop-free, on top of sum_marginals_restatement.SumMarginals: layers in BDD-major order, any NumPy float type; a
solver's public layer order maps to it through bdd_hip_parallel_mma.bdd_major_order().

The backward of the min-marginal differences mm_diff[l] = m_hi[l] - m_lo[l], m_a[l] = min over the nodes u of l of F[u] + c_a[l] +
T[child_a(u)] (F: cost from the root, T: cost to the terminal), with g the incoming gradient:
    seeds      per layer l and arc a at the arg-min node u* (s = +1 for hi, -1 for lo): dc_a[l] += s g[l], dF[u*] += s g[l],
               dT[child_a(u*)] += s g[l]; sinks take nothing, an arc no finite path takes seeds nothing
    through T  root -> terminal: a node sends its whole dT along its arg-min arc to that child and adds it to that arc's dc of its layer
    through F  terminal -> root: a node sends its whole dF to its arg-min (parent, arc) and adds it to that arc's dc of the parent's layer
Ties: lowest node first among a layer's nodes, first among the parents in (node, lo before hi) order, lo before hi.

Test helper only: Python loops over nodes."""
import numpy as np

from sum_marginals_restatement import BOT, TOP, SumMarginals


class Gradients(SumMarginals):
    # ---- plain potentials in any type
    def potentials(self, dtype=None):
        R = np.dtype(dtype or self.dt).type
        lo, hi = self.lo.astype(R), self.hi.astype(R)
        inf = R(np.inf)
        F = np.full(self.n_nodes, inf, R)
        T = np.full(self.n_nodes, inf, R)
        for b in range(self.n_bdds):
            if self.bdd_layer_ptr[b] < self.bdd_layer_ptr[b + 1]:
                F[self.layer_node_ptr[self.bdd_layer_ptr[b]]] = R(0)
        for l in range(self.n_layers):
            for u in range(self.layer_node_ptr[l], self.layer_node_ptr[l + 1]):
                for c, cost in ((self.lo_child[u], lo[l]), (self.hi_child[u], hi[l])):
                    if c >= 0 and F[u] + cost < F[c]:
                        F[c] = F[u] + cost
        for l in range(self.n_layers - 1, -1, -1):
            for u in range(self.layer_node_ptr[l], self.layer_node_ptr[l + 1]):
                T[u] = min(lo[l] + self._t(T, self.lo_child[u], R), hi[l] + self._t(T, self.hi_child[u], R))
        return F, T

    @staticmethod
    def _t(T, c, R):
        return R(0) if c == TOP else R(np.inf) if c == BOT else T[c]

    def _path_values(self, F, T, R):
        """(P_lo, P_hi, A, B) per node: F + (c + T[child]) through each arc, and c + T[child]"""
        lo, hi = self.lo.astype(R), self.hi.astype(R)
        A = np.empty(self.n_nodes, R)
        B = np.empty(self.n_nodes, R)
        for l in range(self.n_layers):
            for u in range(self.layer_node_ptr[l], self.layer_node_ptr[l + 1]):
                A[u] = lo[l] + self._t(T, self.lo_child[u], R)
                B[u] = hi[l] + self._t(T, self.hi_child[u], R)
        return F + A, F + B, A, B

    def mm_diff(self, dtype=None):
        R = np.dtype(dtype or self.dt).type
        F, T = self.potentials(R)
        P0, P1, _, _ = self._path_values(F, T, R)
        out = np.empty(self.n_layers, R)
        for l in range(self.n_layers):
            s = slice(self.layer_node_ptr[l], self.layer_node_ptr[l + 1])
            out[l] = P1[s].min() - P0[s].min()
        return out

    def node_layer(self):
        out = np.zeros(self.n_nodes, np.int64)
        for l in range(self.n_layers):
            out[self.layer_node_ptr[l]:self.layer_node_ptr[l + 1]] = l
        return out

    def parents(self):
        """per node: its (parent, arc) pairs by parent, lo arc before hi arc"""
        par = [[] for _ in range(self.n_nodes)]
        for u in range(self.n_nodes):
            for arc, c in enumerate((self.lo_child[u], self.hi_child[u])):
                if c >= 0:
                    par[c].append((u, arc))
        return par

    # ---- the backward of the min-marginal differences
    def grad_mm_diff(self, g, dtype=None, gaps=None):
        """(grad_lo, grad_hi) per layer in `dtype`.  gaps (a list, optional) receives one (bdd, gap, |value|) per minimum that carried a
        non-zero gradient: best-to-second-best distance (inf when there is no second candidate) and the magnitude of the best value."""
        R = np.dtype(dtype or self.dt).type
        g = np.asarray(g).astype(R)
        lo, hi = self.lo.astype(R), self.hi.astype(R)
        F, T = self.potentials(R)
        P0, P1, A, B = self._path_values(F, T, R)
        nl, bdd_of, par = self.node_layer(), self.layer_bdd(), self.parents()
        dT, dF = np.zeros(self.n_nodes, R), np.zeros(self.n_nodes, R)
        dc = [np.zeros(self.n_layers, R), np.zeros(self.n_layers, R)]
        inf = R(np.inf)
        if gaps is not None:   # the largest |path cost| of every BDD
            for b in range(self.n_bdds):
                n0, n1 = self.layer_node_ptr[self.bdd_layer_ptr[b]], self.layer_node_ptr[self.bdd_layer_ptr[b + 1]]
                v = np.concatenate([P0[n0:n1], P1[n0:n1]])
                gaps.append((b, np.inf, float(np.abs(v[np.isfinite(v)]).max(initial=0.0))))

        def note(l, vals, i):
            if gaps is not None:
                rest = np.delete(vals, i)
                gaps.append((int(bdd_of[l]), float(rest.min() - vals[i]) if rest.size else np.inf, float(abs(vals[i]))))

        for l in range(self.n_layers):   # seeds
            u0 = self.layer_node_ptr[l]
            for arc, (P, child, s) in enumerate(((P0, self.lo_child, R(-1)), (P1, self.hi_child, R(1)))):
                vals = P[u0:self.layer_node_ptr[l + 1]]
                i = int(np.argmin(vals))   # the first minimum
                if not vals[i] < inf:
                    continue
                if g[l] != 0:
                    note(l, vals, i)
                dc[arc][l] += s * g[l]
                dF[u0 + i] += s * g[l]
                if child[u0 + i] >= 0:
                    dT[child[u0 + i]] += s * g[l]
        for u in range(self.n_nodes):    # through T: parents come before their children
            if dT[u] == 0:
                continue
            l = nl[u]
            arc = 0 if A[u] <= B[u] else 1
            if gaps is not None:
                gaps.append((int(bdd_of[l]), float(abs(A[u] - B[u])), float(abs(F[u] + min(A[u], B[u])))))
            dc[arc][l] += dT[u]
            c = (self.lo_child, self.hi_child)[arc][u]
            if c >= 0:
                dT[c] += dT[u]
        for c in range(self.n_nodes - 1, -1, -1):   # through F
            if dF[c] == 0 or not par[c]:
                continue
            vals = np.array([F[p] + (lo[nl[p]], hi[nl[p]])[arc] for p, arc in par[c]], R)
            i = int(np.argmin(vals))
            if not vals[i] < inf:
                continue
            note(nl[c], vals, i)
            p, arc = par[c][i]
            dF[p] += dF[c]
            dc[arc][nl[p]] += dF[c]
        return dc[0], dc[1]

    def decision_gap(self, g, dtype=np.longdouble):
        """per BDD: (the smallest best-to-second-best distance over the minima that decide where a non-zero gradient goes — per layer and arc
        over its nodes, per node over its two arcs, per node over its parents —, the largest finite |F + c + T| over the BDD's nodes and arcs)"""
        gaps = []
        self.grad_mm_diff(g, dtype, gaps)
        gap = np.full(self.n_bdds, np.inf)
        mag = np.zeros(self.n_bdds)
        for b, d, v in gaps:
            gap[b] = min(gap[b], d)
            mag[b] = max(mag[b], v)
        return gap, mag

    def _enumerate(self, b):
        """(x [N, k], cost [N] with inf for the assignments that do not end in the top sink) of BDD b, as SumMarginals.brute_force"""
        l0, l1 = self.bdd_layer_ptr[b], self.bdd_layer_ptr[b + 1]
        k = l1 - l0
        assert 0 < k <= 19
        N = 1 << k
        x = (np.arange(N)[:, None] >> np.arange(k)[None, :]) & 1
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
            node = np.where(alive, nxt, BOT)
        return x, np.where(node == TOP, cost, np.inf)

    def brute_force_grad(self, b, g):
        """sum over the layers l of BDD b of g[l] (chi(P_hi(l)) - chi(P_lo(l))) by enumeration of all assignments: (grad_lo, grad_hi) of its layers"""
        l0 = self.bdd_layer_ptr[b]
        x, cost = self._enumerate(b)
        k = x.shape[1]
        out = [np.zeros(k), np.zeros(k)]
        for j in range(k):
            for arc, s in ((0, -1.0), (1, 1.0)):
                c = np.where(x[:, j] == arc, cost, np.inf)
                i = int(np.argmin(c))
                if not np.isfinite(c[i]):
                    continue
                for j2 in range(k):
                    out[x[i, j2]][j2] += s * float(g[l0 + j])
        return out[0], out[1]

    def brute_force_solution(self, b):
        """(the arg-min assignment of BDD b as 0 / 1 per layer, its cost)"""
        x, cost = self._enumerate(b)
        i = int(np.argmin(cost))
        return x[i].astype(np.float64), float(cost[i])

    # ---- the three elementwise operators
    def grad_lower_bound(self, glb, x):
        gb = np.asarray(glb)[self.layer_bdd()]
        return (1 - x) * gb, x * gb

    @staticmethod
    def grad_distribute_delta(grad_lo, grad_hi, mm):
        return np.where(np.asarray(mm) > 0, grad_hi, -np.asarray(grad_lo))

    def grad_cost_perturbation(self, grad_lo, grad_hi):
        out_lo, out_hi = np.zeros(self.n_vars, np.asarray(grad_lo).dtype), np.zeros(self.n_vars, np.asarray(grad_hi).dtype)
        for l in range(self.n_layers):
            out_lo[self.layer_var[l]] += grad_lo[l]
            out_hi[self.layer_var[l]] += grad_hi[l]
        n = np.maximum(self.nbdds, 1)
        return out_lo / n, out_hi / n


def gradients_of(col, precision="double"):
    return Gradients(col.instr, col.delims, precision)


def tie_free_state(m, seed):
    """seeded Gaussian lo / hi costs and incoming gradient for a model with m.n_layers layers (BDD-major): (lo, hi, g) in float64, rounded to
    float32 values so that a float solver holds exactly the same numbers"""
    rng = np.random.Generator(np.random.PCG64(seed))
    lo, hi, g = (rng.normal(0, 1, m.n_layers).astype(np.float32).astype(np.float64) for _ in range(3))
    return lo, hi, g


GAP_FACTOR = 2.0 ** 10


def tie_free(m, g, dt):
    """the condition of the GPU comparison: every BDD's decision gap, in the type wider than dt, is at least 2^10 eps(dt) times its largest
    |path cost|.  Returns (holds, the smallest ratio gap / (eps * magnitude) over the BDDs)."""
    wider = np.float64 if np.dtype(dt) == np.float32 else np.longdouble
    gap, mag = m.decision_gap(g, wider)
    ratio = gap / (np.finfo(dt).eps * np.maximum(mag, np.finfo(np.float64).tiny))
    return bool(np.all(ratio >= GAP_FACTOR)), float(ratio.min())
