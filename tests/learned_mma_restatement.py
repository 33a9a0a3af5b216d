"""NumPy restatement of the learned MMA iterations (bdd_cuda_learned_mma<REAL>::iterations, src/bdd_solver/bdd_cuda_learned_mma.cu:9-262
of the reference) for the tests: the per-pass arithmetic of SURVEY.md §8 a' with the isotropic split delta[v] / n[v] replaced by a weight per
layer, alpha[l] * S[v], and the history rules of :211-266.  Layers are in BDD-major order (bdd ascending, then top to bottom), as in the
C restatements under oracle/; a solver's public layer order maps to it through bdd_hip_parallel_mma.bdd_major_order().

Test helper only: slow (Python loops over nodes), meant for instances of a few thousand nodes."""
import numpy as np

TOPSINK, BOTSINK = 2**64 - 1, 2**64 - 2   # bdd_collection's sink indices of a flat instruction
TOP, BOT = -1, -2


class LearnedMma:
    def __init__(self, instr, delims, precision="double"):
        self.dt = np.float64 if precision == "double" else np.float32
        R = self.dt
        instr = np.asarray(instr, np.uint64)
        delims = np.asarray(delims, np.uint64)
        self.n_bdds = len(delims) - 1
        lo_child, hi_child, layer_node_ptr, layer_var, bdd_layer_ptr = [], [], [], [], []
        for b in range(self.n_bdds):
            d0, d1 = int(delims[b]), int(delims[b + 1])
            idx = [int(instr[i, 2]) for i in range(d0, d1)]
            node_of, k = {}, len(lo_child)
            for j, x in enumerate(idx):
                node_of[j] = TOP if x == TOPSINK else BOT if x == BOTSINK else None
                if node_of[j] is None:
                    node_of[j] = k
                    k += 1
            bdd_layer_ptr.append(len(layer_var))
            prev = None
            for j, x in enumerate(idx):
                if x in (TOPSINK, BOTSINK):
                    continue
                if x != prev:
                    layer_node_ptr.append(len(lo_child))
                    layer_var.append(x)
                    prev = x
                lo_child.append(node_of[int(instr[d0 + j, 0]) - d0])
                hi_child.append(node_of[int(instr[d0 + j, 1]) - d0])
        bdd_layer_ptr.append(len(layer_var))
        layer_node_ptr.append(len(lo_child))
        self.lo_child, self.hi_child = lo_child, hi_child
        self.layer_node_ptr, self.bdd_layer_ptr = layer_node_ptr, bdd_layer_ptr
        self.layer_var = np.array(layer_var, np.int64)
        self.n_layers, self.n_nodes = len(layer_var), len(lo_child)
        self.n_vars = int(self.layer_var.max()) + 1 if self.n_layers else 0
        self.nbdds = np.bincount(self.layer_var, minlength=self.n_vars)
        self.lo = np.zeros(self.n_layers, R)
        self.hi = np.zeros(self.n_layers, R)
        self.mm = np.zeros(self.n_layers, R)
        self.F = np.zeros(self.n_nodes, R)
        self.T = np.zeros(self.n_nodes, R)
        self.initial_lb_change = np.inf

    # ---- costs, plain sweeps (cuda_rule oracle: cr_update_costs, cr_backward_run, cr_forward_run, cr_lower_bound)
    def update_costs_hi(self, costs):
        c = np.zeros(self.n_vars)
        c[: min(len(costs), self.n_vars)] = costs[: self.n_vars]
        for l in range(self.n_layers):
            v = self.layer_var[l]
            self.hi[l] = self.dt(float(self.hi[l]) + c[v] / float(self.nbdds[v]))

    def _Tc(self, c):
        return self.dt(0) if c == TOP else self.dt(np.inf) if c == BOT else self.T[c]

    def backward_run(self):
        for l in range(self.n_layers - 1, -1, -1):
            for u in range(self.layer_node_ptr[l], self.layer_node_ptr[l + 1]):
                self.T[u] = min(self._Tc(self.hi_child[u]) + self.hi[l], self._Tc(self.lo_child[u]) + self.lo[l])

    def _flush_F(self):
        self.F[:] = np.inf
        for b in range(self.n_bdds):
            if self.bdd_layer_ptr[b] < self.bdd_layer_ptr[b + 1]:
                self.F[self.layer_node_ptr[self.bdd_layer_ptr[b]]] = 0

    def forward_run(self):
        self._flush_F()
        for l in range(self.n_layers):
            for u in range(self.layer_node_ptr[l], self.layer_node_ptr[l + 1]):
                for c, cost in ((self.lo_child[u], self.lo[l]), (self.hi_child[u], self.hi[l])):
                    if c >= 0:
                        self.F[c] = min(self.F[c], self.F[u] + cost)

    def lower_bound_per_bdd(self):
        out = np.zeros(self.n_bdds, self.dt)
        for b in range(self.n_bdds):
            if self.bdd_layer_ptr[b] < self.bdd_layer_ptr[b + 1]:
                out[b] = self.T[self.layer_node_ptr[self.bdd_layer_ptr[b]]]
        return out

    def lower_bound(self):
        """backward_run + the roots' costs from terminal summed in double (after a backward pass backward_run gives the same T)"""
        self.backward_run()
        return float(sum(float(x) for x in self.lower_bound_per_bdd()))

    def bdds_solution(self):
        """argmin path per BDD (compute_bdd_sol_func with the `< 0` rule: lo unless hi_path - lo_path <= 0), REAL 0 / 1 per layer"""
        self.forward_run()
        sol = np.zeros(self.n_layers, self.dt)
        for b in range(self.n_bdds):
            l0, l1 = self.bdd_layer_ptr[b], self.bdd_layer_ptr[b + 1]
            if l0 == l1:
                continue
            u = self.layer_node_ptr[l0]
            for l in range(l0, l1):
                if u is None or not (self.layer_node_ptr[l] <= u < self.layer_node_ptr[l + 1]):
                    continue
                hi_path = self.F[u] + (self._Tc(self.hi_child[u]) + self.hi[l])
                lo_path = self.F[u] + (self._Tc(self.lo_child[u]) + self.lo[l])
                take_lo = (hi_path - lo_path) > 0
                sol[l] = 0 if take_lo else 1
                c = self.lo_child[u] if take_lo else self.hi_child[u]
                u = c if c >= 0 else None
        return sol

    # ---- one pass
    def sums(self):
        """compute_delta of the deferred differences, in REAL and layer order: S[v] = {sum of -mm over mm < 0, sum of mm over mm > 0}"""
        S = np.zeros((self.n_vars, 2), self.dt)
        for l in range(self.n_layers):
            m = self.mm[l]
            if m > 0:
                S[self.layer_var[l], 1] += m
            elif m < 0:
                S[self.layer_var[l], 0] += -m
        return S

    def weighted_delta(self, alpha):
        """{lo, hi} added to layer l in the next pass: alpha[l] * S[v(l)], one product in REAL"""
        S = self.sums()
        a = np.asarray(alpha, self.dt)
        return a * S[self.layer_var, 0], a * S[self.layer_var, 1]

    def _layer_mm(self, l, omega):
        m0 = m1 = self.dt(np.inf)
        for u in range(self.layer_node_ptr[l], self.layer_node_ptr[l + 1]):
            m0 = min(m0, (self.F[u] + self.lo[l]) + self._Tc(self.lo_child[u]))
            m1 = min(m1, (self.F[u] + self.hi[l]) + self._Tc(self.hi_child[u]))
        if not (np.isfinite(m0) and np.isfinite(m1)):
            return self.dt(0)
        return self.dt(omega) * (m1 - m0)

    def forward_pass(self, omega, dlo, dhi):
        self._flush_F()
        for l in range(self.n_layers):
            mm = self._layer_mm(l, omega)
            self.mm[l] = mm
            lo = (self.lo[l] + min(mm, self.dt(0))) + dlo[l]
            hi = (self.hi[l] + min(-mm, self.dt(0))) + dhi[l]
            for u in range(self.layer_node_ptr[l], self.layer_node_ptr[l + 1]):
                if self.lo_child[u] >= 0:
                    self.F[self.lo_child[u]] = min(self.F[self.lo_child[u]], self.F[u] + lo)
                if self.hi_child[u] >= 0:
                    self.F[self.hi_child[u]] = min(self.F[self.hi_child[u]], self.F[u] + hi)
            self.lo[l], self.hi[l] = lo, hi

    def backward_pass(self, omega, dlo, dhi):
        for l in range(self.n_layers - 1, -1, -1):
            mm = self._layer_mm(l, omega)
            self.mm[l] = mm
            hi = (self.hi[l] + min(-mm, self.dt(0))) + dhi[l]
            lo = (self.lo[l] + min(mm, self.dt(0))) + dlo[l]
            for u in range(self.layer_node_ptr[l], self.layer_node_ptr[l + 1]):
                self.T[u] = min(hi + self._Tc(self.hi_child[u]), lo + self._Tc(self.lo_child[u]))
            self.lo[l], self.hi[l] = lo, hi

    def learned_iteration(self, alpha, omega=0.5):
        """forward_iteration_learned_mm_dist + backward_iteration_learned_mm_dist (:52-93, :125-165)"""
        self.backward_run()
        self.forward_pass(omega, *self.weighted_delta(alpha))
        self.backward_pass(omega, *self.weighted_delta(alpha))

    def isotropic_alpha(self):
        return (self.dt(1) / self.nbdds[self.layer_var].astype(self.dt)).astype(self.dt)

    # ---- iterations(...) with its stopping rule and history (:184-270)
    def iterations(self, alpha, num_itr, omega=0.5, improvement_slope=1e-6, sol_avg=None, lb_first_diff_avg=None, lb_second_diff_avg=None,
                   compute_history_for_itr=0, history_avg_beta=0.9, lb_trajectory=None):
        """returns the number of iterations run; the averages are updated in place; lb_trajectory (a list) receives the bound after
        every iteration"""
        R = self.dt
        beta = R(history_avg_beta)
        lb_initial = self.lower_bound() if num_itr > 0 else 0.0
        lb_post = lb_initial
        hist = History(beta) if compute_history_for_itr > 0 else None
        converged = False
        ran = 0
        for itr in range(num_itr):
            self.learned_iteration(alpha, omega)
            ran += 1
            if hist is not None and (compute_history_for_itr >= num_itr - itr or converged):
                hist.step(self.bdds_solution(), self.lower_bound_per_bdd(), sol_avg, lb_first_diff_avg, lb_second_diff_avg)
            lb_prev, lb_post = lb_post, self.lower_bound()
            if lb_trajectory is not None:
                lb_trajectory.append(lb_post)
            if itr == 0 and not np.isfinite(self.initial_lb_change):
                self.initial_lb_change = abs(lb_initial - lb_post)
            if improvement_slope > 0:
                if not converged and abs(lb_prev - lb_post) < improvement_slope * self.initial_lb_change:
                    converged = True
                if converged and (hist.tracked if hist else 0) == compute_history_for_itr:
                    break
        return ran


def ema(avg, cur, beta):
    """compute_exp_moving_avg (:171-180): beta * avg in REAL, the rest in double (1.0 is a double literal), rounded to REAL once"""
    R = avg.dtype.type
    return ((beta * avg).astype(np.float64) + (1.0 - np.float64(beta)) * cur.astype(np.float64)).astype(R)


class History:
    """The history rules of :211-254: sol_avg is an EMA of the solutions (the first one copied), lb_first_diff_avg an EMA of the change
    of the per-BDD bounds (from the second tracked iteration, the first change copied), lb_second_diff_avg an EMA of the second difference
    (from the third, the first copied)."""

    def __init__(self, beta):
        self.beta = beta
        self.tracked = 0
        self.last = self.second = self.third = None

    def step(self, sol, lb, sol_avg, lb1, lb2):
        if self.tracked == 0:
            sol_avg[:] = sol
        else:
            sol_avg[:] = ema(sol_avg, sol, self.beta)
            chg = lb - self.second
            if self.tracked == 1:
                lb1[:] = chg
            else:
                lb1[:] = ema(lb1, chg, self.beta)
                sec = chg - (self.second - self.third)
                if self.tracked == 2:
                    lb2[:] = sec
                else:
                    lb2[:] = ema(lb2, sec, self.beta)
        self.third, self.second = self.second, lb.copy()
        self.tracked += 1
