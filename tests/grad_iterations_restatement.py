"""NumPy restatement of the backward of the learned MMA iterations (bdd_cuda_learned_mma<REAL>::grad_iterations,
src/bdd_solver/bdd_cuda_learned_mma.cu:308-385 with :418-621 of the reference) for the tests, hop-free, on grad_restatement.Gradients (and
through it learned_mma_restatement.LearnedMma): layers in BDD-major order, any NumPy float type.

One learned iteration is LearnedMma.learned_iteration: T = T(lo, hi); a forward pass (root -> terminal) that reads that T and writes new
costs, mm and F; a backward pass (terminal -> root) that reads that F, writes new costs and mm and rebuilds T from them.  Each pass adds
alpha[l] * S_a[v(l)] to the arc costs, S the per-variable sums of the deferred differences d it consumed (the other pass's mm).

A pass is recorded as what its reverse reads: the costs before and after it, the potentials F and T its min-marginals were taken with, its
mm, the differences it consumed and their sums.  The reverse is taken at the arg-mins the pass took, with the potentials the pass used (the
reference replays the pass and then takes its arg-mins against the potentials of the UPDATED costs, :542-545 and :592-595; that is not
restated here).  Ties: lowest node first among a layer's nodes, first among the parents in (node, lo before hi) order, lo before hi; the
dual update's sign rule at mm = 0 and d = 0 is the reference's (>= 0: the hi side, :439-442 and :512-516).

Test helper only: Python loops over nodes."""
import numpy as np

from grad_restatement import Gradients


class GradIterations(Gradients):
    # ---- the passes, recorded
    def _setup(self, R):
        self._nl, self._par, self._bdd_of = self.node_layer(), self.parents(), self.layer_bdd()
        self._roots = [self.layer_node_ptr[self.bdd_layer_ptr[b]] for b in range(self.n_bdds) if self.bdd_layer_ptr[b] < self.bdd_layer_ptr[b + 1]]

    def _T_of(self, lo, hi, R):
        T = np.full(self.n_nodes, R(np.inf), R)
        for l in range(self.n_layers - 1, -1, -1):
            for u in range(self.layer_node_ptr[l], self.layer_node_ptr[l + 1]):
                T[u] = min(hi[l] + self._t(T, self.hi_child[u], R), lo[l] + self._t(T, self.lo_child[u], R))
        return T

    def _sums(self, d, R):
        S = np.zeros((self.n_vars, 2), R)
        for l in range(self.n_layers):
            if d[l] > 0:
                S[self.layer_var[l], 1] += d[l]
            elif d[l] < 0:
                S[self.layer_var[l], 0] += -d[l]
        return S

    def _layer_paths(self, l, lo, hi, F, T, R):
        u0, u1 = self.layer_node_ptr[l], self.layer_node_ptr[l + 1]
        P0 = np.array([(F[u] + lo) + self._t(T, self.lo_child[u], R) for u in range(u0, u1)], R)
        P1 = np.array([(F[u] + hi) + self._t(T, self.hi_child[u], R) for u in range(u0, u1)], R)
        return P0, P1

    def _update(self, l, lo, hi, P0, P1, om, alpha, S, R):
        m0, m1 = P0.min(), P1.min()
        mm = om[l] * (m1 - m0) if (np.isfinite(m0) and np.isfinite(m1)) else R(0)
        v = self.layer_var[l]
        return mm, (lo + min(mm, R(0))) + alpha[l] * S[v, 0], (hi + min(-mm, R(0))) + alpha[l] * S[v, 1]

    def forward_pass_rec(self, lo, hi, d, alpha, om, R):
        T = self._T_of(lo, hi, R)
        S = self._sums(d, R)
        F = np.full(self.n_nodes, R(np.inf), R)
        F[self._roots] = R(0)
        lo2, hi2, mm = lo.copy(), hi.copy(), np.zeros(self.n_layers, R)
        for l in range(self.n_layers):
            P0, P1 = self._layer_paths(l, lo[l], hi[l], F, T, R)
            mm[l], lo2[l], hi2[l] = self._update(l, lo[l], hi[l], P0, P1, om, alpha, S, R)
            for u in range(self.layer_node_ptr[l], self.layer_node_ptr[l + 1]):
                for c, cost in ((self.lo_child[u], lo2[l]), (self.hi_child[u], hi2[l])):
                    if c >= 0 and F[u] + cost < F[c]:
                        F[c] = F[u] + cost
        return dict(pre=(lo, hi), post=(lo2, hi2), F=F, T=T, mm=mm, d=d, S=S)

    def backward_pass_rec(self, lo, hi, d, F, alpha, om, R):
        S = self._sums(d, R)
        T = np.full(self.n_nodes, R(np.inf), R)
        lo2, hi2, mm = lo.copy(), hi.copy(), np.zeros(self.n_layers, R)
        for l in range(self.n_layers - 1, -1, -1):
            P0, P1 = self._layer_paths(l, lo[l], hi[l], F, T, R)
            mm[l], lo2[l], hi2[l] = self._update(l, lo[l], hi[l], P0, P1, om, alpha, S, R)
            for u in range(self.layer_node_ptr[l], self.layer_node_ptr[l + 1]):
                T[u] = min(hi2[l] + self._t(T, self.hi_child[u], R), lo2[l] + self._t(T, self.lo_child[u], R))
        return dict(pre=(lo, hi), post=(lo2, hi2), F=F, T=T, mm=mm, d=d, S=S)

    def iterate(self, lo, hi, d, alpha, omega, n, dtype=None, records=None):
        """n learned iterations from (lo, hi, d) in `dtype`: (lo, hi, mm) after them.  omega: a scalar or one value per layer.  records (a list)
        receives (forward pass, backward pass) per iteration."""
        R = np.dtype(dtype or self.dt).type
        self._setup(R)
        lo, hi, d, alpha = (np.asarray(x).astype(R) for x in (lo, hi, d, alpha))
        om = np.broadcast_to(np.asarray(omega), (self.n_layers,)).astype(R)
        for _ in range(n):
            f = self.forward_pass_rec(lo, hi, d, alpha, om, R)
            b = self.backward_pass_rec(f["post"][0], f["post"][1], f["mm"], f["F"], alpha, om, R)
            if records is not None:
                records.append((f, b))
            lo, hi, d = b["post"][0], b["post"][1], b["mm"]
        return lo, hi, d

    # ---- the reverse of a pass
    def _note(self, gaps, l, gap, mag):
        if gaps is not None:
            gaps.append((int(self._bdd_of[l]), float(gap), float(mag)))

    def _note_min(self, gaps, l, vals, i):
        if gaps is not None:
            rest = np.delete(vals, i)
            self._note(gaps, l, rest.min() - vals[i] if rest.size else np.inf, abs(vals[i]))

    def _dual_and_seeds(self, rec, l, dc0, dc1, g_lo, g_hi, g_mm, alpha, om, R, out, gaps):
        """steps 3 and 4 of a layer: dc = what arrived at the layer's post-pass costs through the potentials.  Returns (g_lo, g_hi of the
        pre-pass costs, the seeds [(node, arc, value)])"""
        u0 = self.layer_node_ptr[l]
        v = self.layer_var[l]
        ga, gb = dc0 + g_lo[l], dc1 + g_hi[l]
        mm = rec["mm"][l]
        dmm = g_mm[l] + (-gb if mm >= 0 else ga)
        out["dmm"][l] = dmm
        if ga != 0 or gb != 0:
            self._note(gaps, l, abs(mm), 0.0)
        out["gS"][l, 0], out["gS"][l, 1] = alpha[l] * ga, alpha[l] * gb
        out["galpha"][l] += rec["S"][v, 0] * ga + rec["S"][v, 1] * gb
        P0, P1 = self._layer_paths(l, rec["pre"][0][l], rec["pre"][1][l], rec["F"], rec["T"], R)
        fin = np.concatenate([P0[np.isfinite(P0)], P1[np.isfinite(P1)]])
        self._note(gaps, l, np.inf, np.abs(fin).max(initial=0.0))
        i0, i1 = int(np.argmin(P0)), int(np.argmin(P1))
        seeds = []
        if np.isfinite(P0[i0]) and np.isfinite(P1[i1]):
            out["gomega"][l] += dmm * (P1[i1] - P0[i0])
            t = om[l] * dmm
            if t != 0:
                self._note_min(gaps, l, P0, i0)
                self._note_min(gaps, l, P1, i1)
            seeds = [(u0 + i0, 0, -t), (u0 + i1, 1, t)]
            ga, gb = ga - t, gb + t
        return ga, gb, seeds

    def reverse_backward_pass(self, rec, g_lo, g_hi, g_mm, gT, alpha, om, R, gaps=None):
        """(g_lo, g_hi of the costs before the pass, gd of the differences it consumed, gF, galpha [L], gomega [L])"""
        lo2, hi2 = rec["post"]
        T = rec["T"]
        out = dict(gS=np.zeros((self.n_layers, 2), R), galpha=np.zeros(self.n_layers, R), gomega=np.zeros(self.n_layers, R), dmm=np.zeros(self.n_layers, R))
        self.last_dmm = out["dmm"]   # the gradient that reached each layer's mm: incoming plus the dual update's feedback
        dT = np.array(gT, R)
        gF = np.zeros(self.n_nodes, R)
        o_lo, o_hi = np.zeros(self.n_layers, R), np.zeros(self.n_layers, R)
        for l in range(self.n_layers):
            dc = [R(0), R(0)]
            sends = []
            for u in range(self.layer_node_ptr[l], self.layer_node_ptr[l + 1]):
                A, B = lo2[l] + self._t(T, self.lo_child[u], R), hi2[l] + self._t(T, self.hi_child[u], R)
                arc = 0 if A <= B else 1
                if dT[u] != 0:
                    self._note(gaps, l, abs(A - B), abs(min(A, B)))
                dc[arc] += dT[u]
                sends.append((u, arc, dT[u]))
            o_lo[l], o_hi[l], seeds = self._dual_and_seeds(rec, l, dc[0], dc[1], g_lo, g_hi, g_mm, alpha, om, R, out, gaps)
            for u, arc, x in seeds:
                gF[u] += x
            for u, arc, x in sends + seeds:
                c = (self.lo_child, self.hi_child)[arc][u]
                if c >= 0:
                    dT[c] += x
        return o_lo, o_hi, self._gd(rec, out["gS"], R, gaps), gF, out["galpha"], out["gomega"]

    def reverse_forward_pass(self, rec, g_lo, g_hi, g_mm, gF, alpha, om, R, gaps=None):
        """(g_lo, g_hi of the costs before the pass, gd, gT of the T the pass read, galpha [L], gomega [L])"""
        lo2, hi2 = rec["post"]
        F = rec["F"]
        out = dict(gS=np.zeros((self.n_layers, 2), R), galpha=np.zeros(self.n_layers, R), gomega=np.zeros(self.n_layers, R), dmm=np.zeros(self.n_layers, R))
        self.last_dmm = out["dmm"]   # the gradient that reached each layer's mm: incoming plus the dual update's feedback
        dF = np.array(gF, R)
        gT = np.zeros(self.n_nodes, R)
        o_lo, o_hi = np.zeros(self.n_layers, R), np.zeros(self.n_layers, R)
        inf = R(np.inf)
        for l in range(self.n_layers - 1, -1, -1):
            dc = [R(0), R(0)]
            took = {}
            for u in range(self.layer_node_ptr[l], self.layer_node_ptr[l + 1]):   # the children are done
                for arc, c in enumerate((self.lo_child[u], self.hi_child[u])):
                    if c < 0 or dF[c] == 0:
                        continue
                    vals = np.array([F[p] + (lo2, hi2)[a][self._nl[p]] for p, a in self._par[c]], R)
                    i = int(np.argmin(vals))
                    if vals[i] < inf and self._par[c][i] == (u, arc):
                        self._note_min(gaps, l, vals, i)
                        dc[arc] += dF[c]
                        took[u] = took.get(u, R(0)) + dF[c]
            o_lo[l], o_hi[l], seeds = self._dual_and_seeds(rec, l, dc[0], dc[1], g_lo, g_hi, g_mm, alpha, om, R, out, gaps)
            for u, x in took.items():
                dF[u] += x
            for u, arc, x in seeds:
                dF[u] += x
                c = (self.lo_child, self.hi_child)[arc][u]
                if c >= 0:
                    gT[c] += x
        return o_lo, o_hi, self._gd(rec, out["gS"], R, gaps), gT, out["galpha"], out["gomega"]

    def _gd(self, rec, gS, R, gaps):
        gSv = np.zeros((self.n_vars, 2), R)
        for l in range(self.n_layers):
            gSv[self.layer_var[l]] += gS[l]
        gd = np.zeros(self.n_layers, R)
        for l in range(self.n_layers):
            v = self.layer_var[l]
            gd[l] = gSv[v, 1] if rec["d"][l] >= 0 else -gSv[v, 0]
            if gSv[v, 0] != 0 or gSv[v, 1] != 0:
                self._note(gaps, l, abs(rec["d"][l]), 0.0)
        return gd

    def through_T(self, lo, hi, gT, R, gaps=None):
        """gT pushed through T(lo, hi): (grad_lo, grad_hi); the through-T step of Gradients.grad_mm_diff without seeds"""
        T = self._T_of(lo, hi, R)
        dT = np.array(gT, R)
        o = [np.zeros(self.n_layers, R), np.zeros(self.n_layers, R)]
        for u in range(self.n_nodes):
            if dT[u] == 0:
                continue
            l = self._nl[u]
            A, B = lo[l] + self._t(T, self.lo_child[u], R), hi[l] + self._t(T, self.hi_child[u], R)
            arc = 0 if A <= B else 1
            self._note(gaps, l, abs(A - B), abs(min(A, B)))
            o[arc][l] += dT[u]
            c = (self.lo_child, self.hi_child)[arc][u]
            if c >= 0:
                dT[c] += dT[u]
        return o[0], o[1]

    # ---- the entry point
    def grad_iterations(self, lo, hi, d, alpha, omega, n, g_lo, g_hi, g_mm, dtype=None, gaps=None):
        """The transpose-Jacobian product of n learned iterations from (lo, hi, d): (g_lo, g_hi, g_d, g_alpha [L], g_omega [L]) in `dtype`;
        the gradient of a scalar omega is the sum of g_omega.  gaps (a list, optional) receives (bdd, gap, magnitude) records: per arg-min
        that routed a non-zero gradient its best-to-second-best distance, per sign decision |mm| resp. |d|, and the magnitudes of the path
        costs of every layer (with gap inf)."""
        R = np.dtype(dtype or self.dt).type
        recs = []
        self.iterate(lo, hi, d, alpha, omega, n, R, recs)
        alpha = np.asarray(alpha).astype(R)
        om = np.broadcast_to(np.asarray(omega), (self.n_layers,)).astype(R)
        g_lo, g_hi, g_mm = (np.asarray(x).astype(R) for x in (g_lo, g_hi, g_mm))
        g_alpha, g_omega = np.zeros(self.n_layers, R), np.zeros(self.n_layers, R)
        gT = np.zeros(self.n_nodes, R)
        for f, b in reversed(recs):
            g_lo, g_hi, g_mm, gF, ga, go = self.reverse_backward_pass(b, g_lo, g_hi, g_mm, gT, alpha, om, R, gaps)
            g_alpha, g_omega = g_alpha + ga, g_omega + go
            g_lo, g_hi, g_mm, gT, ga, go = self.reverse_forward_pass(f, g_lo, g_hi, g_mm, gF, alpha, om, R, gaps)
            g_alpha, g_omega = g_alpha + ga, g_omega + go
        if recs:
            t_lo, t_hi = self.through_T(recs[0][0]["pre"][0], recs[0][0]["pre"][1], gT, R, gaps)
            g_lo, g_hi = g_lo + t_lo, g_hi + t_hi
        return g_lo, g_hi, g_mm, g_alpha, g_omega

    def trajectory_gap(self, lo, hi, d, alpha, omega, n, g_lo, g_hi, g_mm, dtype=np.longdouble):
        """per BDD: (the smallest decision gap of the trajectory, the largest finite |F + c + T| any of its passes saw)"""
        gaps = []
        self.grad_iterations(lo, hi, d, alpha, omega, n, g_lo, g_hi, g_mm, dtype, gaps)
        gap, mag = np.full(self.n_bdds, np.inf), np.zeros(self.n_bdds)
        for b, x, v in gaps:
            gap[b] = min(gap[b], x)
            mag[b] = max(mag[b], v)
        return gap, mag


def grad_iterations_of(col, precision="double"):
    return GradIterations(col.instr, col.delims, precision)


def seeded_inputs(m, seed):
    """the fixtures of the tests for a model m (BDD-major): costs and the three incoming gradients seeded Gaussian and rounded to float32
    values, weights seeded uniform in [0.2, 1] and normalised per variable, omega_vec seeded in [0.3, 0.7] — all float64 holding float32 values"""
    rng = np.random.Generator(np.random.PCG64(seed))
    f32 = lambda x: x.astype(np.float32).astype(np.float64)
    lo, hi, a, b, c = (f32(rng.normal(0, 1, m.n_layers)) for _ in range(5))
    w = rng.uniform(0.2, 1.0, m.n_layers)
    w = f32(w / np.bincount(m.layer_var, weights=w, minlength=m.n_vars)[m.layer_var])
    omega_vec = f32(rng.uniform(0.3, 0.7, m.n_layers))
    return dict(lo=lo, hi=hi, g_lo=a, g_hi=b, g_mm=c, alpha=w, omega_vec=omega_vec)


GAP_FACTOR = 2.0 ** 10


def trajectory_tie_free(m, x, omega, dt, untracked=1, tracked=2):
    """the condition of the GPU comparison: after `untracked` iterations from (x.lo, x.hi, 0), every BDD's decision gap over `tracked`
    reversed iterations, in the type wider than dt, is at least 2^10 eps(dt) times its largest |path cost|.  (holds, smallest ratio)"""
    wider = np.float64 if np.dtype(dt) == np.float32 else np.longdouble
    lo, hi, d = m.iterate(x["lo"], x["hi"], np.zeros(m.n_layers), x["alpha"], omega, untracked, wider)
    gap, mag = m.trajectory_gap(lo, hi, d, x["alpha"], omega, tracked, x["g_lo"], x["g_hi"], x["g_mm"], wider)
    ratio = gap / (np.finfo(dt).eps * np.maximum(mag, np.finfo(np.float64).tiny))
    return bool(np.all(ratio >= GAP_FACTOR)), float(ratio.min())
