"""Host-side mirror of the reference solver classes for the `cuda parallel mma` path.

`bdd_hip_parallel_mma` has the public surface of `LPMP::bdd_cuda_parallel_mma<REAL>` +
`bdd_cuda_base<REAL>` (reference: include/bdd_solver/bdd_cuda_parallel_mma.h:7-52,
include/bdd_solver/bdd_cuda_base.h:58-229) — same method names, argument meaning and error
behaviour — so the parity tests read like test/test_cuda_parallel_mma.cu and
test/test_bdd_cuda_*.cpp.  All compute happens in the HIP library behind the C-ABI.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import capi
from .bdd_collection import BddCollection


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _is_dev(x):
    """a device buffer: anything with data_ptr() living on a GPU (torch CUDA tensors) — the thrust::device_vector
    overloads of the reference.  Passed through the C-ABI as a raw pointer with on_device = 1."""
    return hasattr(x, "data_ptr") and bool(getattr(x, "is_cuda", False))


def _dev_ptr(x, n, dtype):
    """raw pointer of a contiguous device buffer holding >= n elements of `dtype`"""
    assert x.is_contiguous() and x.numel() >= n, "device buffer too small or not contiguous"
    assert x.element_size() == np.dtype(dtype).itemsize, "device buffer has the wrong element type"
    return C.c_void_p(x.data_ptr())


class bdd_hip_parallel_mma:
    """Drop-in for bdd_cuda_parallel_mma<REAL> (value_type = float | double)."""

    def __init__(self, bdd_col: BddCollection, costs_hi=None, precision: str = "double", device: int = 0,
                 pack_width: int = 0, wide_pack_width: int = 0, deterministic: bool = False,
                 vars_per_bin: int = 0, stage_cap: int = 0, waves_per_block: int = 0, keep_bdd_order: bool = False,
                 resident_sweeps: int = 0, exchange_by_variable: int = 0, variant_flags: int = 0, pack_fill: int = 0, pack_stagger: int = 0, _handle=None):
        self._L = capi.lib()
        self.value_type = {"double": np.float64, "float": np.float32, "single": np.float32}[precision]
        self._prec = capi.F64 if self.value_type == np.float64 else capi.F32
        if _handle is not None:
            self._h = _handle
            return
        instr = np.ascontiguousarray(bdd_col.instr, dtype=np.uint64)
        delims = np.ascontiguousarray(bdd_col.delims, dtype=np.uint64)
        opts = capi.Options(pack_width, wide_pack_width, 1 if deterministic else 0, vars_per_bin, stage_cap, waves_per_block)
        opts.keep_bdd_order = int(keep_bdd_order)   # 0 (default): BDDs of equal shape are packed together; 1: input order; 2: include/bdd_mma.h
        opts.resident_sweeps = int(resident_sweeps)         # 0 automatic, 1 off, 2 on
        opts.exchange_by_variable = int(exchange_by_variable)             # 2: entries by (variable, bdd)
        opts.pack_fill = int(pack_fill)
        opts.pack_stagger = int(pack_stagger)
        opts.variant_flags = int(variant_flags)             # bit 0 / 1: backward / forward narrow + wide sweeps as two launches
        h = C.c_void_p()
        costs = None if costs_hi is None else np.ascontiguousarray(costs_hi, dtype=np.float64)
        rc = self._L.bddmma_create(C.byref(h), self._prec, device, _ptr(instr), _ptr(delims), bdd_col.nr_bdds(),
                                   _ptr(costs), 0 if costs is None else costs.size, C.byref(opts))
        capi.check(rc, None)
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            self._L.bddmma_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, rc):
        capi.check(rc, self._h)

    # ---- sizes (bdd_cuda_base.h:98-116)
    def nr_variables(self): return int(self._L.bddmma_nr_variables(self._h))
    def nr_layers(self): return int(self._L.bddmma_nr_layers(self._h))
    def nr_bdd_nodes(self): return int(self._L.bddmma_nr_bdd_nodes(self._h))
    def nr_hops(self): return int(self._L.bddmma_nr_hops(self._h))
    def nr_packs(self): return int(self._L.bddmma_nr_packs(self._h))

    SWEEP_KINDS = ("none", "mixed", "streaming1", "streaming2", "streaming3", "resident1", "resident2")

    def solve_sweep_kind(self) -> str:
        """which kernels run the narrow packs' solve sweeps (include/bdd_mma.h: BDDMMA_SWEEPS_*)"""
        return self.SWEEP_KINDS[int(self._L.bddmma_solve_sweep_kind(self._h))]
    def fused_small(self) -> bool:
        """whole iterations run inside one launch (the instance fits one workgroup; csrc/kernels/small.hpp)"""
        return bool(self._L.bddmma_fused_small(self._h))
    def fused_small_learned(self) -> bool:
        """True when learned_iterations() runs whole learned iterations inside one launch too (with improvement_slope <= 0; batches of
        such solvers: bdd_hip_batch.learned_iterations)"""
        return bool(self._L.bddmma_fused_small_learned(self._h))
    def fused_small_history(self) -> bool:
        """True when bdd_hip_batch.learned_iterations_history can run this solver's history steps (compute_history_for_itr > 0) inside
        its workgroup as well"""
        return bool(self._L.bddmma_fused_small_history(self._h))
    def fused_small_stop(self) -> bool:
        """True when a bdd_hip_batch runs this solver's stopping rule (improvement_slope > 0) inside its workgroup too
        (bddmma_fused_small_stop; bdd_hip_batch.learned_iterations_stopping)."""
        return bool(self._L.bddmma_fused_small_stop(self._h))

    def nontemporal_loads(self) -> bool:
        """the solve sweeps run in the instantiation that loads potentials and staging tables non-temporally (footprint beyond the caches' reach)"""
        return bool(self._L.bddmma_nontemporal_loads(self._h))

    def potentials_on_chip(self) -> bool:
        """the solve sweeps of iteration() / iterations() / run_solver rebuild F and T on chip instead of storing and reloading them"""
        return bool(self._L.bddmma_potentials_on_chip(self._h))

    def onchip_hops(self) -> int:
        """hop capacity of the kernels behind potentials_on_chip(): 0 (off), 10 or 12 (F and T on chip), 16 (F on chip, T through memory)"""
        return int(self._L.bddmma_onchip_hops(self._h))
    def lane_sweeps(self) -> bool:
        """those sweeps keep a BDD's potentials in one lane and walk the hops in registers (csrc/kernels/narrow5.hpp; variant_flags bit 24: off)"""
        return bool(self._L.bddmma_lane_sweeps(self._h))
    def device(self) -> int:
        """index of the GPU the solver lives on"""
        return int(self._L.bddmma_device(self._h))
    def device_bytes(self): return int(self._L.bddmma_device_bytes(self._h))
    def device_allocated_bytes(self): return int(self._L.bddmma_device_allocated_bytes(self._h))

    def nr_bdds(self, var=None):
        if var is None:
            return int(self._L.bddmma_nr_bdds(self._h))
        return int(self.get_num_bdds_per_var()[var])

    def get_num_bdds_per_var(self):
        out = np.zeros(self.nr_variables(), np.int32)
        self._ck(self._L.bddmma_num_bdds_per_var(self._h, _ptr(out)))
        return out

    def get_primal_variable_index(self):
        out = np.zeros(self.nr_layers(), np.int32)
        self._ck(self._L.bddmma_layer_variables(self._h, _ptr(out)))
        return out

    def get_bdd_index(self):
        out = np.zeros(self.nr_layers(), np.int32)
        self._ck(self._L.bddmma_layer_bdds(self._h, _ptr(out)))
        return out

    def nodes_per_hop(self):
        out = np.zeros(self.nr_hops(), np.uint64)
        self._ck(self._L.bddmma_nodes_per_hop(self._h, _ptr(out)))
        return out

    def layers_per_hop(self):
        out = np.zeros(self.nr_hops(), np.uint64)
        self._ck(self._L.bddmma_layers_per_hop(self._h, _ptr(out)))
        return out

    def bdd_major_order(self):
        """Permutation taking internal layer order to BDD-major order (bdd ascending, hop ascending):
        the layer order of the reference CPU solver (bdd_parallel_mma_base.cpp:75-170)."""
        return np.argsort(self.get_bdd_index(), kind="stable")

    # ---- costs
    def update_costs(self, cost_delta_0, cost_delta_1):
        if _is_dev(cost_delta_0) or _is_dev(cost_delta_1):   # update_costs(device_vector<REAL>, device_vector<REAL>), bdd_cuda_base.cu:476-500
            n0 = cost_delta_0.numel() if cost_delta_0 is not None else 0
            n1 = cost_delta_1.numel() if cost_delta_1 is not None else 0
            self._ck(self._L.bddmma_update_costs(self._h, _dev_ptr(cost_delta_0, n0, self.value_type) if n0 else None, n0,
                                                 _dev_ptr(cost_delta_1, n1, self.value_type) if n1 else None, n1, self._prec, 1))
            return
        lo = np.ascontiguousarray(cost_delta_0, dtype=np.float64)
        hi = np.ascontiguousarray(cost_delta_1, dtype=np.float64)
        self._ck(self._L.bddmma_update_costs(self._h, _ptr(lo), lo.size, _ptr(hi), hi.size, capi.F64, 0))

    def set_cost(self, c, var):
        self._ck(self._L.bddmma_set_cost(self._h, float(c), int(var)))

    def get_solver_costs(self, out=None):
        n = self.nr_layers()
        if out is not None:   # three device buffers
            self._ck(self._L.bddmma_get_solver_costs(self._h, *(_dev_ptr(x, n, self.value_type) for x in out), 1))
            return out
        lo, hi, mm = (np.zeros(n, self.value_type) for _ in range(3))
        self._ck(self._L.bddmma_get_solver_costs(self._h, _ptr(lo), _ptr(hi), _ptr(mm), 0))
        return lo, hi, mm

    def set_solver_costs(self, lo, hi, mm):
        if _is_dev(lo):
            n = self.nr_layers()
            self._ck(self._L.bddmma_set_solver_costs(self._h, *(_dev_ptr(x, n, self.value_type) for x in (lo, hi, mm)), 1))
            return
        lo, hi, mm = (np.ascontiguousarray(x, dtype=self.value_type) for x in (lo, hi, mm))
        self._ck(self._L.bddmma_set_solver_costs(self._h, _ptr(lo), _ptr(hi), _ptr(mm), 0))

    def get_primal_objective_vector(self, out):
        """compute_primal_objective_vec into a device buffer (bdd_cuda_base.cu:1352-1362)"""
        self._ck(self._L.bddmma_primal_objective_vec(self._h, _dev_ptr(out, self.nr_variables(), self.value_type), 1))
        return out

    def get_primal_objective_vector_host(self):
        out = np.zeros(self.nr_variables(), self.value_type)
        self._ck(self._L.bddmma_primal_objective_vec(self._h, _ptr(out), 0))
        return out

    # ---- sweeps
    def forward_run(self): self._ck(self._L.bddmma_forward_run(self._h))
    def backward_run(self): self._ck(self._L.bddmma_backward_run(self._h))

    def lower_bound(self) -> float:
        lb = C.c_double()
        self._ck(self._L.bddmma_lower_bound(self._h, C.byref(lb)))
        return lb.value

    def lower_bound_per_bdd(self, out=None):
        if out is not None:
            self._ck(self._L.bddmma_lower_bound_per_bdd(self._h, _dev_ptr(out, self.nr_bdds(), self.value_type), 1))
            return out
        out = np.zeros(self.nr_bdds(), self.value_type)
        self._ck(self._L.bddmma_lower_bound_per_bdd(self._h, _ptr(out), 0))
        return out

    # ---- parallel mma
    def iteration(self, omega=0.5):
        self._ck(self._L.bddmma_iteration(self._h, float(omega)))

    def iterations(self, n, omega=0.5):
        self._ck(self._L.bddmma_iterations(self._h, float(omega), int(n)))

    def forward_mm(self, omega, delta_lo_hi):
        if _is_dev(delta_lo_hi):   # forward_mm(omega, device_vector<REAL>&), bdd_cuda_parallel_mma.cu:207-257
            self._ck(self._L.bddmma_forward_mm(self._h, float(omega), _dev_ptr(delta_lo_hi, 2 * self.nr_variables(), self.value_type), 1))
            return
        assert delta_lo_hi.dtype == self.value_type and delta_lo_hi.size == 2 * self.nr_variables()
        self._ck(self._L.bddmma_forward_mm(self._h, float(omega), _ptr(delta_lo_hi), 0))

    def backward_mm(self, omega, delta_lo_hi):
        if _is_dev(delta_lo_hi):
            self._ck(self._L.bddmma_backward_mm(self._h, float(omega), _dev_ptr(delta_lo_hi, 2 * self.nr_variables(), self.value_type), 1))
            return
        assert delta_lo_hi.dtype == self.value_type and delta_lo_hi.size == 2 * self.nr_variables()
        self._ck(self._L.bddmma_backward_mm(self._h, float(omega), _ptr(delta_lo_hi), 0))

    def normalize_delta(self, delta_lo_hi):
        if _is_dev(delta_lo_hi):
            self._ck(self._L.bddmma_normalize_delta(self._h, _dev_ptr(delta_lo_hi, 2 * self.nr_variables(), self.value_type), 1))
            return
        self._ck(self._L.bddmma_normalize_delta(self._h, _ptr(delta_lo_hi), 0))

    def distribute_delta(self):
        self._ck(self._L.bddmma_distribute_delta(self._h))

    # ---- learned iterations (bdd_cuda_learned_mma<REAL>::iterations; Python binding bdd_cuda_learned_mma_py.cu:580-600)
    def _learned_buf(self, x, n, what):
        """(pointer, on_device) of a REAL[n] argument: a torch device tensor or a numpy array of the solver's precision"""
        if _is_dev(x):
            if x.numel() != n:
                raise capi.BddMmaError(f"bdd_mma error {capi.ERR_INVALID_ARGUMENT}: {what} has {x.numel()} values, the solver needs {n}")
            if not x.is_contiguous():
                raise capi.BddMmaError(f"bdd_mma error {capi.ERR_INVALID_ARGUMENT}: {what} must be contiguous")
            if x.element_size() != np.dtype(self.value_type).itemsize or not x.is_floating_point():
                raise capi.BddMmaError(f"bdd_mma error {capi.ERR_INVALID_ARGUMENT}: {what} is {x.dtype}, the solver's values are "
                                       f"{np.dtype(self.value_type).name}")
            return _dev_ptr(x, n, self.value_type), 1
        if not isinstance(x, np.ndarray):
            raise capi.BddMmaError(f"bdd_mma error {capi.ERR_INVALID_ARGUMENT}: {what} must be a numpy array or a device tensor")
        if x.dtype != self.value_type:
            raise capi.BddMmaError(f"bdd_mma error {capi.ERR_INVALID_ARGUMENT}: {what} is {x.dtype}, the solver's values are "
                                   f"{np.dtype(self.value_type).name}")
        if x.size != n:
            raise capi.BddMmaError(f"bdd_mma error {capi.ERR_INVALID_ARGUMENT}: {what} has {x.size} values, the solver needs {n}")
        if not x.flags.c_contiguous:
            raise capi.BddMmaError(f"bdd_mma error {capi.ERR_INVALID_ARGUMENT}: {what} must be contiguous")
        return _ptr(x), 0

    def learned_iterations(self, dist_weights, num_itr, omega=0.5, improvement_slope=1e-6, sol_avg=None, lb_first_diff_avg=None,
                           lb_second_diff_avg=None, compute_history_for_itr=0, history_avg_beta=0.9, omega_vec=None) -> int:
        """iterations(dist_weights, ...) of the learned solver: MMA passes that add dist_weights[l] * (sum of the deferred differences
        of the layer's variable) instead of the sum / nr_bdds; returns the number of iterations run.  dist_weights: REAL[nr_layers] in
        the order of get_solver_costs.  With compute_history_for_itr > 0, sol_avg (REAL[nr_layers]), lb_first_diff_avg and
        lb_second_diff_avg (REAL[nr_bdds]) are updated in place (all three on the host or all three on the device).
        omega_vec: REAL[nr_layers] in the same order (numpy array or device tensor), one omega per layer; when given, omega is ignored.
        State contract and error codes: include/bdd_mma.h, bddmma_learned_iterations(_omega_vec)."""
        w, w_dev = self._learned_buf(dist_weights, self.nr_layers(), "dist_weights")
        if omega_vec is not None:
            ov, ov_dev = self._learned_buf(omega_vec, self.nr_layers(), "omega_vec")
        outs = [None, None, None]
        out_dev = 0
        if int(compute_history_for_itr) > 0:
            bufs = (sol_avg, lb_first_diff_avg, lb_second_diff_avg)
            if any(b is None for b in bufs):
                raise capi.BddMmaError(f"bdd_mma error {capi.ERR_INVALID_ARGUMENT}: compute_history_for_itr > 0 needs sol_avg, "
                                       "lb_first_diff_avg and lb_second_diff_avg")
            devs = [_is_dev(b) for b in bufs]
            if len(set(devs)) != 1:
                raise capi.BddMmaError(f"bdd_mma error {capi.ERR_INVALID_ARGUMENT}: the history outputs must all be on the host or all on the device")
            sizes = (self.nr_layers(), self.nr_bdds(), self.nr_bdds())
            names = ("sol_avg", "lb_first_diff_avg", "lb_second_diff_avg")
            outs = [self._learned_buf(b, n, nm)[0] for b, n, nm in zip(bufs, sizes, names)]
            out_dev = 1 if devs[0] else 0
        done = C.c_uint64()
        if omega_vec is not None:
            self._ck(self._L.bddmma_learned_iterations_omega_vec(self._h, w, w_dev, int(num_itr), ov, ov_dev, float(improvement_slope), outs[0],
                                                                  outs[1], outs[2], int(compute_history_for_itr), float(history_avg_beta),
                                                                  out_dev, C.byref(done)))
            return int(done.value)
        self._ck(self._L.bddmma_learned_iterations(self._h, w, w_dev, int(num_itr), float(omega), float(improvement_slope), outs[0], outs[1],
                                                    outs[2], int(compute_history_for_itr), float(history_avg_beta), out_dev, C.byref(done)))
        return int(done.value)

    def get_isotropic_dist_weights(self, out=None):
        """1 / nr_bdds(variable) per layer (get_solver_costs order): the weights with which learned_iterations is iterations"""
        if out is not None:
            self._ck(self._L.bddmma_isotropic_dist_weights(self._h, _dev_ptr(out, self.nr_layers(), self.value_type), 1))
            return out
        out = np.zeros(self.nr_layers(), self.value_type)
        self._ck(self._L.bddmma_isotropic_dist_weights(self._h, _ptr(out), 0))
        return out

    def set_delta(self, delta_lo_hi):
        if _is_dev(delta_lo_hi):
            self._ck(self._L.bddmma_set_delta(self._h, _dev_ptr(delta_lo_hi, 2 * self.nr_variables(), self.value_type), 1))
            return
        d = np.ascontiguousarray(delta_lo_hi, dtype=self.value_type)
        self._ck(self._L.bddmma_set_delta(self._h, _ptr(d), 0))

    def get_delta(self, out=None):
        if out is not None:
            self._ck(self._L.bddmma_get_delta(self._h, _dev_ptr(out, 2 * self.nr_variables(), self.value_type), 1))
            return out
        out = np.zeros(2 * self.nr_variables(), self.value_type)
        self._ck(self._L.bddmma_get_delta(self._h, _ptr(out), 0))
        return out

    # ---- min-marginals / solutions
    def min_marginals_cuda(self, get_sorted=True, out=None):
        n = self.nr_layers()
        if out is not None:   # (int32 var, REAL mm0, REAL mm1) device buffers, as min_marginals_cuda returns them (bdd_cuda_base.cu:716-749)
            v, m0, m1 = out
            self._ck(self._L.bddmma_min_marginals(self._h, 1 if get_sorted else 0, _dev_ptr(v, n, np.int32), _dev_ptr(m0, n, self.value_type),
                                                  _dev_ptr(m1, n, self.value_type), 1))
            return out
        var = np.zeros(n, np.int32)
        mm0, mm1 = np.zeros(n, self.value_type), np.zeros(n, self.value_type)
        self._ck(self._L.bddmma_min_marginals(self._h, 1 if get_sorted else 0, _ptr(var), _ptr(mm0), _ptr(mm1), 0))
        return var, mm0, mm1

    def min_marginals(self):
        """two_dim_variable_array<array<double,2>>[var][bdd] (bdd_cuda_base.cu:751-786) as a list of (k,2) arrays."""
        var, mm0, mm1 = self.min_marginals_cuda(True)
        nb = self.get_num_bdds_per_var()
        ptr = np.concatenate([[0], np.cumsum(nb)])
        return [np.stack([mm0[ptr[v]:ptr[v + 1]], mm1[ptr[v]:ptr[v + 1]]], axis=1).astype(np.float64)
                for v in range(self.nr_variables())]

    # ---- sum-marginals / smooth solution (bdd_cuda_base.cu:788-1100; state contract: include/bdd_mma.h, bddmma_sum_marginals)
    def sum_marginals_cuda(self, get_sorted=True, get_log_probs=True, out=None):
        """(var, sm_lo, sm_hi) per layer: log of the summed exp(-cost) over the root-to-top paths through the layer's lo / hi arcs
        (get_log_probs=False: the sums themselves); -inf / 0 where no path takes that side.  `out`: (int32, REAL, REAL) device buffers."""
        n = self.nr_layers()
        flags = (1 if get_sorted else 0, 1 if get_log_probs else 0)
        if out is not None:
            v, m0, m1 = out
            self._ck(self._L.bddmma_sum_marginals(self._h, *flags, _dev_ptr(v, n, np.int32), _dev_ptr(m0, n, self.value_type),
                                                  _dev_ptr(m1, n, self.value_type), 1))
            return out
        var = np.zeros(n, np.int32)
        sm0, sm1 = np.zeros(n, self.value_type), np.zeros(n, self.value_type)
        self._ck(self._L.bddmma_sum_marginals(self._h, *flags, _ptr(var), _ptr(sm0), _ptr(sm1), 0))
        return var, sm0, sm1

    def sum_marginals(self, get_log_probs=True):
        """[var][bdd] -> (sm_lo, sm_hi) as a list of (k,2) arrays, like min_marginals() (bdd_cuda_base.cu:1066-1100)."""
        var, sm0, sm1 = self.sum_marginals_cuda(True, get_log_probs)
        nb = self.get_num_bdds_per_var()
        ptr = np.concatenate([[0], np.cumsum(nb)])
        return [np.stack([sm0[ptr[v]:ptr[v + 1]], sm1[ptr[v]:ptr[v + 1]]], axis=1).astype(np.float64)
                for v in range(self.nr_variables())]

    def smooth_solution_per_bdd(self, out=None):
        """exp(sm_hi) / (exp(sm_lo) + exp(sm_hi)) per layer, internal layer order (smooth_solution_cuda, bdd_cuda_base.cu:1050-1064); `out`: device buffer"""
        if out is not None:
            self._ck(self._L.bddmma_smooth_solution(self._h, _dev_ptr(out, self.nr_layers(), self.value_type), 1))
            return out
        res = np.zeros(self.nr_layers(), self.value_type)
        self._ck(self._L.bddmma_smooth_solution(self._h, _ptr(res), 0))
        return res

    def min_marginal_diff(self, out=None):
        """mm1 - mm0 per layer (compute_and_set_min_marginal_diff, bdd_cuda_parallel_mma_py.cu:56-72); `out`: device buffer"""
        if out is not None:
            self._ck(self._L.bddmma_min_marginal_diff(self._h, _dev_ptr(out, self.nr_layers(), self.value_type), 1))
            return out
        res = np.zeros(self.nr_layers(), self.value_type)
        self._ck(self._L.bddmma_min_marginal_diff(self._h, _ptr(res), 0))
        return res

    # ---- single-shot backward operators (bdd_cuda_learned_mma.h:82-110; state contracts: include/bdd_mma.h, bddmma_grad_*).  Inputs are NumPy
    # arrays (results come back as NumPy arrays) or device buffers (then `out` must hold the device buffers the results go to).
    def _grad_call(self, fn, ins, in_sizes, out, out_sizes, *flags):
        if _is_dev(ins[0]):
            assert out is not None and len(out) == len(out_sizes), "device inputs need device output buffers (out=...)"
            args = [_dev_ptr(x, n, self.value_type) for x, n in zip(list(ins) + list(out), list(in_sizes) + list(out_sizes))]
            self._ck(fn(self._h, *args, *flags, 1))
            return out[0] if len(out) == 1 else tuple(out)
        ins = [np.ascontiguousarray(x, dtype=self.value_type) for x in ins]
        for x, n in zip(ins, in_sizes):
            assert x.size == n, f"expected {n} values, got {x.size}"
        res = [np.zeros(n, self.value_type) for n in out_sizes]
        self._ck(fn(self._h, *(_ptr(x) for x in ins + res), *flags, 0))
        return res[0] if len(res) == 1 else tuple(res)

    def grad_all_min_marginal_differences(self, grad_mm, out=None):
        """(grad_lo, grad_hi): the transpose-Jacobian product of min_marginal_diff() with respect to the arc costs, per layer
        (grad_mm_diff_all_hops, bdd_cuda_learned_mma.cu:623-1023); `out`: (grad_lo, grad_hi) device buffers"""
        n = self.nr_layers()
        return self._grad_call(self._L.bddmma_grad_min_marginal_diff, (grad_mm,), (n,), out, (n, n))

    def grad_lower_bound_per_bdd(self, grad_lb_per_bdd, out=None):
        """(grad_lo, grad_hi) of the per-BDD lower bounds weighted by grad_lb_per_bdd [nr_bdds] (bdd_cuda_learned_mma.cu:387-416)"""
        n = self.nr_layers()
        return self._grad_call(self._L.bddmma_grad_lower_bound_per_bdd, (grad_lb_per_bdd,), (self.nr_bdds(),), out, (n, n), 0)

    def grad_smooth_lower_bound_per_bdd(self, grad_lb_per_bdd, out=None):
        """the same for the smooth lower bound -log sum over paths of exp(-cost) per BDD: x is smooth_solution_per_bdd()"""
        n = self.nr_layers()
        return self._grad_call(self._L.bddmma_grad_lower_bound_per_bdd, (grad_lb_per_bdd,), (self.nr_bdds(),), out, (n, n), 1)

    def grad_distribute_delta(self, grad_lo, grad_hi, out=None):
        """gradient with respect to the deferred differences the last distribute_delta() applied (bdd_cuda_learned_mma.cu:1025-1065);
        `out`: a device buffer (a 1-tuple of it is accepted too)"""
        n = self.nr_layers()
        if out is not None and not isinstance(out, (tuple, list)):
            out = (out,)
        return self._grad_call(self._L.bddmma_grad_distribute_delta, (grad_lo, grad_hi), (n, n), out, (n,))

    def grad_cost_perturbation(self, grad_lo, grad_hi, out=None):
        """(grad_lo_pert, grad_hi_pert) per variable: the backward of update_costs (bdd_cuda_learned_mma.cu:1067-1187)"""
        n, v = self.nr_layers(), self.nr_variables()
        return self._grad_call(self._L.bddmma_grad_cost_perturbation, (grad_lo, grad_hi), (n, n), out, (v, v))

    def grad_iterations(self, dist_weights, grad_lo, grad_hi, grad_mm, omega=0.5, track_grad_after_itr=0, track_grad_for_num_itr=1, num_caches=1,
                        omega_vec=None, out=None):
        """The backward of learned_iterations (grad_iterations, bdd_cuda_learned_mma.cu:308-385): the loss gradient with respect to the arc
        costs and deferred differences after track_grad_for_num_itr iterations (run after track_grad_after_itr untracked ones) -> the
        gradient with respect to those before them, the distribution weights and omega.  Returns (grad_lo, grad_hi, grad_mm,
        grad_dist_weights, grad_omega); grad_omega has one entry, nr_layers with omega_vec.  NumPy inputs give new NumPy arrays; with
        device tensors grad_lo / grad_hi / grad_mm are updated in place and `out` = (grad_dist_weights, grad_omega) device buffers.
        State contract and error codes: include/bdd_mma.h, bddmma_grad_learned_iterations."""
        n = self.nr_layers()
        n_om = n if omega_vec is not None else 1
        w, w_dev = self._learned_buf(dist_weights, n, "dist_weights")
        ov, ov_dev = self._learned_buf(omega_vec, n, "omega_vec") if omega_vec is not None else (None, 0)
        tail = (int(track_grad_after_itr), int(track_grad_for_num_itr), int(num_caches))
        if _is_dev(grad_lo):
            assert out is not None and len(out) == 2, "device gradients need device output buffers: out=(grad_dist_weights, grad_omega)"
            ptrs = [_dev_ptr(x, k, self.value_type) for x, k in zip((grad_lo, grad_hi, grad_mm, out[0], out[1]), (n, n, n, n, n_om))]
            self._ck(self._L.bddmma_grad_learned_iterations(self._h, w, w_dev, float(omega), ov, ov_dev, *ptrs, *tail, 1))
            return grad_lo, grad_hi, grad_mm, out[0], out[1]
        g = [np.array(x, dtype=self.value_type, order="C") for x in (grad_lo, grad_hi, grad_mm)]
        for x in g:
            assert x.size == n, f"expected {n} values, got {x.size}"
        res = [np.zeros(n, self.value_type), np.zeros(n_om, self.value_type)]
        self._ck(self._L.bddmma_grad_learned_iterations(self._h, w, w_dev, float(omega), ov, ov_dev, *(_ptr(x) for x in g + res), *tail, 0))
        return g[0], g[1], g[2], res[0], res[1]

    def bdds_solution_vec(self, out=None):
        if out is not None:   # device_vector<char> (bdd_cuda_base.cu:1138-1145)
            self._ck(self._L.bddmma_bdds_solution(self._h, 0, _dev_ptr(out, self.nr_layers(), np.int8), 1))
            return out
        out = np.zeros(self.nr_layers(), np.int8)
        self._ck(self._L.bddmma_bdds_solution(self._h, 0, _ptr(out), 0))
        return out

    def bdds_solution(self):
        out = np.zeros(self.nr_layers(), np.int8)
        self._ck(self._L.bddmma_bdds_solution(self._h, 1, _ptr(out), 0))
        nb = self.get_num_bdds_per_var()
        ptr = np.concatenate([[0], np.cumsum(nb)])
        return [out[ptr[v]:ptr[v + 1]].astype(np.float64) for v in range(self.nr_variables())]

    # ---- L-BFGS support
    def net_solver_costs(self, out=None):
        if out is not None:
            self._ck(self._L.bddmma_net_solver_costs(self._h, _dev_ptr(out, self.nr_layers(), self.value_type), 1))
            return out
        out = np.zeros(self.nr_layers(), self.value_type)
        self._ck(self._L.bddmma_net_solver_costs(self._h, _ptr(out), 0))
        return out

    def make_dual_feasible(self, d):
        if _is_dev(d):
            self._ck(self._L.bddmma_make_dual_feasible(self._h, _dev_ptr(d, self.nr_layers(), self.value_type), 1))
            return
        assert d.dtype == self.value_type and d.size == self.nr_layers()
        self._ck(self._L.bddmma_make_dual_feasible(self._h, _ptr(d), 0))

    def gradient_step(self, g, step_size):
        if _is_dev(g):
            self._ck(self._L.bddmma_gradient_step(self._h, _dev_ptr(g, self.nr_layers(), self.value_type), float(step_size), 1))
            return
        g = np.ascontiguousarray(g, dtype=self.value_type)
        self._ck(self._L.bddmma_gradient_step(self._h, _ptr(g), float(step_size), 0))

    # ---- primal rounding
    def perturb_primal_costs(self, cur_delta, round_index=0, seed=0, lbfgs=None):
        """one round of perturb_primal_costs (incremental_mm_agreement_rounding_cuda.cu:262-331)
        -> dict(counts = (#one, #zero, #equal, #inconsistent), sol, cost_delta_0, cost_delta_1)"""
        n = self.nr_variables()
        counts = (C.c_uint32 * 4)()
        sol = np.zeros(n, np.int8)
        c0, c1 = np.zeros(n, self.value_type), np.zeros(n, self.value_type)
        self._ck(self._L.bddmma_perturb_primal_costs(self._h, lbfgs._h if lbfgs is not None else None, float(cur_delta), int(round_index),
                                                     int(seed), counts, _ptr(sol), _ptr(c0), _ptr(c1)))
        return dict(counts=tuple(int(c) for c in counts), sol=sol, cost_delta_0=c0, cost_delta_1=c1)

    def primal_rounding_incremental(self, init_delta, delta_growth_rate, num_itr_lb, verbose=False, num_rounds=500, seed=0):
        """incremental_mm_agreement_rounding_cuda on this solver (primal_rounding_incremental of the reference's Python module,
        bdd_cuda_learned_mma_py.cu:433-440): the solution as a list of 0.0 / 1.0 per variable, empty when none was found.  The costs
        stay perturbed."""
        sol = np.zeros(self.nr_variables(), np.int8)
        found = C.c_int(0)
        self._ck(self._L.bddmma_incremental_mm_agreement_rounding(self._h, None, float(init_delta), float(delta_growth_rate), int(num_itr_lb),
                                                                  int(num_rounds), int(seed), 1 if verbose else 0, _ptr(sol), C.byref(found)))
        return [float(x) for x in sol] if found.value else []

    # ---- checkpoint (bdd_cuda_base.cu:1486-1550; pickle in bdd_cuda_parallel_mma_py.cu:15-38)
    def save(self, path: str):
        self._ck(self._L.bddmma_save(self._h, path.encode()))

    @classmethod
    def load(cls, path: str, device: int = 0):
        L = capi.lib()
        h = C.c_void_p()
        capi.check(L.bddmma_load(C.byref(h), device, path.encode()), None)
        prec = "double" if L.bddmma_precision(h) == capi.F64 else "float"
        return cls(None, precision=prec, _handle=h)

    # ---- ordering against other streams (include/bdd_mma.h: bddmma_stream_wait / bddmma_stream_signal)
    def stream_wait(self, hip_stream=0):
        """what is queued on the solver's stream from now on starts after everything queued so far on `hip_stream` (a raw hipStream_t as an
        integer, e.g. torch.cuda.current_stream().cuda_stream; 0 / None: the default stream).  The host does not wait."""
        self._ck(self._L.bddmma_stream_wait(self._h, C.c_void_p(int(hip_stream or 0))))

    def stream_signal(self, hip_stream=0):
        """the reverse: what is queued on `hip_stream` from now on starts after everything queued so far on the solver's stream"""
        self._ck(self._L.bddmma_stream_signal(self._h, C.c_void_p(int(hip_stream or 0))))

    # ---- measurement
    def synchronize(self): self._ck(self._L.bddmma_synchronize(self._h))
    def set_profiling(self, on, stride: int = 1):
        """record hipEvent pairs around the launches of every `stride`-th iteration (0/False: off)"""
        self._ck(self._L.bddmma_set_profiling(self._h, int(stride) if on else 0))

    def get_profile(self):
        p = capi.Profile()
        self._ck(self._L.bddmma_get_profile(self._h, C.byref(p)))
        return {"launches": list(p.launches), "total_ms": list(p.total_ms)}

    def time_kernel(self, kind: int, reps: int) -> float:
        """average ms per launch of one kernel class (see bddmma_time_kernel)"""
        ms = C.c_double()
        self._ck(self._L.bddmma_time_kernel(self._h, int(kind), int(reps), C.byref(ms)))
        return ms.value / reps

    def time_iterations(self, n, omega=0.5) -> float:
        ms = C.c_double()
        self._ck(self._L.bddmma_time_iterations(self._h, float(omega), int(n), C.byref(ms)))
        return ms.value


class bdd_hip_lbfgs:
    """lbfgs<bdd_cuda_parallel_mma<REAL>, ...> (include/bdd_solver/lbfgs.h:35-111) over a HIP solver."""

    def __init__(self, solver: bdd_hip_parallel_mma, history_size=5, init_step_size=1e-6, req_rel_lb_increase=1e-6,
                 step_size_decrease_factor=0.8, step_size_increase_factor=1.1):
        self.solver = solver
        self._L = capi.lib()
        p = capi.LbfgsParams(history_size, init_step_size, req_rel_lb_increase, step_size_decrease_factor,
                             step_size_increase_factor)
        h = C.c_void_p()
        capi.check(self._L.bddmma_lbfgs_create(C.byref(h), solver._h, C.byref(p)), solver._h)
        self._h = h

    def close(self):
        """release the history buffers; call before closing the wrapped solver"""
        if getattr(self, "_h", None):
            self._L.bddmma_lbfgs_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def iteration(self):
        capi.check(self._L.bddmma_lbfgs_iteration(self._h), self.solver._h)

    def lower_bound(self):
        return self.solver.lower_bound()

    def flush(self):
        capi.check(self._L.bddmma_lbfgs_flush(self._h), self.solver._h)

    def state(self):
        st = capi.LbfgsState()
        capi.check(self._L.bddmma_lbfgs_get_state(self._h, C.byref(st)), self.solver._h)
        return {k: getattr(st, k) for k, _ in capi.LbfgsState._fields_}

    def update_costs(self, lo, hi):
        lo = np.ascontiguousarray(lo, dtype=np.float64)
        hi = np.ascontiguousarray(hi, dtype=np.float64)
        capi.check(self._L.bddmma_lbfgs_update_costs(self._h, _ptr(lo), lo.size, _ptr(hi), hi.size, capi.F64, 0),
                   self.solver._h)


class bdd_hip_batch:
    """Solvers whose instances fit one workgroup each (fused_small()), run together: one workgroup per member in one launch instead of
    one launch per solver (include/bdd_mma.h: bddmma_batch_*).  The solvers are borrowed — the batch keeps them alive, and they stay
    usable on their own between its calls; a call behaves as if it had been made on each member in turn."""

    def __init__(self, solvers):
        self.solvers = list(solvers)
        self._L = capi.lib()
        n = len(self.solvers)
        arr = (C.c_void_p * max(n, 1))(*[s._h for s in self.solvers])
        h = C.c_void_p()
        self._check(self._L.bddmma_batch_create(C.byref(h), arr if n else None, n), None)
        self._h = h

    def _check(self, rc, h):
        if rc != capi.OK:
            msg = self._L.bddmma_batch_last_error(h)
            raise capi.BddMmaError(f"bdd_mma error {rc}: {msg.decode() if msg else ''}")

    def close(self):
        """release the batch (never its members); call before closing a member"""
        if getattr(self, "_h", None):
            self._L.bddmma_batch_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __len__(self):
        return int(self._L.bddmma_batch_size(self._h))

    def iterations(self, n, omega=0.5):
        self._check(self._L.bddmma_batch_iterations(self._h, float(omega), int(n)), self._h)

    def learned_iterations(self, dist_weights, num_itr, omega=0.5, omega_vec=None):
        """learned_iterations(w_i, num_itr, omega, improvement_slope=0.0) — with omega_vec its omega_vec form — of every member i, one
        workgroup per member.  dist_weights / omega_vec: the members' REAL[nr_layers] one behind the other in the members' order (numpy
        arrays or device tensors, both of one kind).  Every member must be fused_small_learned().  include/bdd_mma.h:
        bddmma_learned_iterations_batch.  (With a history: learned_iterations_history.)"""
        self.learned_iterations_history(dist_weights, num_itr, omega=omega, omega_vec=omega_vec)

    def learned_iterations_history(self, dist_weights, num_itr, omega=0.5, omega_vec=None, compute_history_for_itr=0, history_avg_beta=0.9,
                                   sol_avg=None, lb_first_diff_avg=None, lb_second_diff_avg=None):
        """learned_iterations with the history of the per-solver method: the last min(num_itr, compute_history_for_itr) iterations also
        update, in place, sol_avg (the members' REAL[nr_layers] one behind the other) and lb_first_diff_avg / lb_second_diff_avg (the
        members' REAL[nr_bdds] one behind the other), inside the members' workgroups; all arrays of the call on the host or all on the
        device.  Every member must be fused_small_history().  compute_history_for_itr == 0 is learned_iterations.  include/bdd_mma.h:
        bddmma_learned_iterations_history_batch."""
        s0 = self.solvers[0]
        n = sum(s.nr_layers() for s in self.solvers)
        w, w_dev = s0._learned_buf(dist_weights, n, "dist_weights")
        ov = None
        if omega_vec is not None:
            ov, ov_dev = s0._learned_buf(omega_vec, n, "omega_vec")
            if ov_dev != w_dev:
                raise capi.BddMmaError(f"bdd_mma error {capi.ERR_INVALID_ARGUMENT}: dist_weights and omega_vec must both be on the host or "
                                       "both on the device")
        if int(compute_history_for_itr) == 0:
            self._check(self._L.bddmma_learned_iterations_batch(self._h, w, ov, float(omega), int(num_itr), w_dev), self._h)
            return
        outs = self._history_outs(n, w_dev, sol_avg, lb_first_diff_avg, lb_second_diff_avg)
        self._check(self._L.bddmma_learned_iterations_history_batch(self._h, w, ov, float(omega), int(num_itr), *outs, int(compute_history_for_itr),
                                                                     float(history_avg_beta), w_dev), self._h)

    def _history_outs(self, n, w_dev, sol_avg, lb_first_diff_avg, lb_second_diff_avg):
        s0 = self.solvers[0]
        nb = sum(s.nr_bdds() for s in self.solvers)
        outs = []
        for x, k, what in ((sol_avg, n, "sol_avg"), (lb_first_diff_avg, nb, "lb_first_diff_avg"), (lb_second_diff_avg, nb, "lb_second_diff_avg")):
            if x is None:   # (the library refuses it: BDDMMA_ERR_INVALID_ARGUMENT, nothing touched)
                outs.append(None)
                continue
            p, dev = s0._learned_buf(x, k, what)
            if dev != w_dev:
                raise capi.BddMmaError(f"bdd_mma error {capi.ERR_INVALID_ARGUMENT}: the arrays of a batch call must all be on the host or all "
                                       "on the device")
            outs.append(p)
        return outs

    def learned_iterations_stopping(self, dist_weights, num_itr, omega=0.5, improvement_slope=1e-6, omega_vec=None, compute_history_for_itr=0,
                                    history_avg_beta=0.9, sol_avg=None, lb_first_diff_avg=None, lb_second_diff_avg=None):
        """learned_iterations(w_i, num_itr, omega, improvement_slope, history...) of every member i — the per-solver method with its stopping
        rule — inside the members' workgroups; returns the members' counts of iterations run, as that method does for one.  Arrays as in
        learned_iterations_history (the history arrays are needed with compute_history_for_itr > 0 only).  With improvement_slope > 0 every
        member must be fused_small_stop(); improvement_slope <= 0 is learned_iterations_history and every count is num_itr.
        include/bdd_mma.h: bddmma_learned_iterations_stop_batch."""
        import ctypes
        s0 = self.solvers[0]
        n = sum(s.nr_layers() for s in self.solvers)
        w, w_dev = s0._learned_buf(dist_weights, n, "dist_weights")
        ov = None
        if omega_vec is not None:
            ov, ov_dev = s0._learned_buf(omega_vec, n, "omega_vec")
            if ov_dev != w_dev:
                raise capi.BddMmaError(f"bdd_mma error {capi.ERR_INVALID_ARGUMENT}: dist_weights and omega_vec must both be on the host or "
                                       "both on the device")
        outs = [None, None, None] if int(compute_history_for_itr) == 0 else self._history_outs(n, w_dev, sol_avg, lb_first_diff_avg, lb_second_diff_avg)
        done = (ctypes.c_uint64 * len(self.solvers))()
        self._check(self._L.bddmma_learned_iterations_stop_batch(self._h, w, ov, float(omega), int(num_itr), float(improvement_slope), *outs,
                                                                  int(compute_history_for_itr), float(history_avg_beta), w_dev, done), self._h)
        return [int(x) for x in done]

    def grad_iterations(self, dist_weights, grad_lo, grad_hi, grad_mm, omega=0.5, track_grad_after_itr=0, track_grad_for_num_itr=1, num_caches=1,
                        omega_vec=None, out=None):
        """grad_iterations(...) of every member i with its part of every array, one workgroup per member in one launch instead of a loop of
        per-solver calls.  Every layer array is the members' REAL[nr_layers] one behind the other in the members' order; both iteration
        counts are the same for all members.  Returns (grad_lo, grad_hi, grad_mm, grad_dist_weights, grad_omega); grad_omega has one entry per
        member (member i's own sum), the concatenated per-layer array with omega_vec.  NumPy inputs give new NumPy arrays; with device
        tensors grad_lo / grad_hi / grad_mm are updated in place and `out` = (grad_dist_weights, grad_omega) device buffers, as in the
        per-solver method.  Every member must be fused_small_learned().  State contract and error codes: include/bdd_mma.h,
        bddmma_grad_learned_iterations_batch."""
        s0 = self.solvers[0]
        n = sum(s.nr_layers() for s in self.solvers)
        n_om = n if omega_vec is not None else len(self.solvers)
        dev = _is_dev(grad_lo)
        w, w_dev = s0._learned_buf(dist_weights, n, "dist_weights")
        ov, ov_dev = s0._learned_buf(omega_vec, n, "omega_vec") if omega_vec is not None else (None, w_dev)
        if w_dev != int(dev) or ov_dev != int(dev):
            raise capi.BddMmaError(f"bdd_mma error {capi.ERR_INVALID_ARGUMENT}: the arrays of a batch call must all be on the host or all "
                                   "on the device")
        tail = (int(track_grad_after_itr), int(track_grad_for_num_itr), int(num_caches))
        call = self._L.bddmma_grad_learned_iterations_batch
        if dev:
            assert out is not None and len(out) == 2, "device gradients need device output buffers: out=(grad_dist_weights, grad_omega)"
            ptrs = [_dev_ptr(x, k, s0.value_type) for x, k in zip((grad_lo, grad_hi, grad_mm, out[0], out[1]), (n, n, n, n, n_om))]
            self._check(call(self._h, w, ov, float(omega), *ptrs, *tail, 1), self._h)
            return grad_lo, grad_hi, grad_mm, out[0], out[1]
        g = [np.array(x, dtype=s0.value_type, order="C") for x in (grad_lo, grad_hi, grad_mm)]
        for x in g:
            assert x.size == n, f"expected {n} values, got {x.size}"
        res = [np.zeros(n, s0.value_type), np.zeros(n_om, s0.value_type)]
        self._check(call(self._h, w, ov, float(omega), *(_ptr(x) for x in g + res), *tail, 0), self._h)
        return g[0], g[1], g[2], res[0], res[1]

    def grad_iterations_counts(self, dist_weights, grad_lo, grad_hi, grad_mm, track_grad_after_itr, track_grad_for_num_itr, omega=0.5, num_caches=1,
                               omega_vec=None, out=None):
        """grad_iterations with every member's own two counts: track_grad_after_itr / track_grad_for_num_itr are sequences of
        len(solvers) — what the backward of learned_iterations_stopping needs, whose members stop at different iterations.  Arrays, results
        and `out` as in grad_iterations.  A member whose tracked count is 0 is left untouched: its parts of grad_lo / grad_hi / grad_mm stay,
        its parts of the two outputs are zero.  include/bdd_mma.h: bddmma_grad_learned_iterations_counts_batch."""
        import ctypes
        s0 = self.solvers[0]
        k = len(self.solvers)
        assert len(track_grad_after_itr) == k and len(track_grad_for_num_itr) == k, f"expected {k} counts of each kind"
        n = sum(s.nr_layers() for s in self.solvers)
        n_om = n if omega_vec is not None else k
        dev = _is_dev(grad_lo)
        w, w_dev = s0._learned_buf(dist_weights, n, "dist_weights")
        ov, ov_dev = s0._learned_buf(omega_vec, n, "omega_vec") if omega_vec is not None else (None, w_dev)
        if w_dev != int(dev) or ov_dev != int(dev):
            raise capi.BddMmaError(f"bdd_mma error {capi.ERR_INVALID_ARGUMENT}: the arrays of a batch call must all be on the host or all "
                                   "on the device")
        tail = ((ctypes.c_uint64 * k)(*(int(x) for x in track_grad_after_itr)), (ctypes.c_uint64 * k)(*(int(x) for x in track_grad_for_num_itr)),
                int(num_caches))
        call = self._L.bddmma_grad_learned_iterations_counts_batch
        if dev:
            assert out is not None and len(out) == 2, "device gradients need device output buffers: out=(grad_dist_weights, grad_omega)"
            ptrs = [_dev_ptr(x, c, s0.value_type) for x, c in zip((grad_lo, grad_hi, grad_mm, out[0], out[1]), (n, n, n, n, n_om))]
            self._check(call(self._h, w, ov, float(omega), *ptrs, *tail, 1), self._h)
            return grad_lo, grad_hi, grad_mm, out[0], out[1]
        g = [np.array(x, dtype=s0.value_type, order="C") for x in (grad_lo, grad_hi, grad_mm)]
        for x in g:
            assert x.size == n, f"expected {n} values, got {x.size}"
        res = [np.zeros(n, s0.value_type), np.zeros(n_om, s0.value_type)]
        self._check(call(self._h, w, ov, float(omega), *(_ptr(x) for x in g + res), *tail, 0), self._h)
        return g[0], g[1], g[2], res[0], res[1]

    def _costs_args(self, arrays, what):
        """three per-layer arrays of a batch call (None: skipped) as pointers and the on_device flag; device tensors or NumPy, all of
        one kind"""
        s0 = self.solvers[0]
        n = sum(s.nr_layers() for s in self.solvers)
        given = [x for x in arrays if x is not None]
        dev = bool(given) and _is_dev(given[0])
        if any(_is_dev(x) != dev for x in given):
            raise capi.BddMmaError(f"bdd_mma error {capi.ERR_INVALID_ARGUMENT}: the arrays of a batch call must all be on the host or all "
                                   "on the device")
        if dev:
            return [None if x is None else _dev_ptr(x, n, s0.value_type) for x in arrays], 1
        for x in given:
            assert x.size == n, f"{what}: expected {n} values, got {x.size}"
        return [_ptr(x) for x in arrays], 0

    def set_solver_costs(self, lo, hi, mm):
        """set_solver_costs(lo_i, hi_i, mm_i) followed by backward_run() of every member i in one launch: the members' REAL[nr_layers]
        one behind the other in the members' order.  Device tensors take the device path (the host does not wait), NumPy arrays the
        host path; None leaves that part of every member's state as it is.  include/bdd_mma.h: bddmma_set_solver_costs_batch."""
        vt = self.solvers[0].value_type
        arrays = [x if x is None or _is_dev(x) else np.ascontiguousarray(x, dtype=vt) for x in (lo, hi, mm)]
        ptrs, dev = self._costs_args(arrays, "set_solver_costs")
        self._check(self._L.bddmma_set_solver_costs_batch(self._h, *ptrs, dev), self._h)

    def get_solver_costs(self, out=None):
        """get_solver_costs() of every member in one launch: (lo, hi, mm), the members' values one behind the other.  out: three device
        buffers, any of them None (skipped) — written in the batch stream's order, the host does not wait; without it three new NumPy
        arrays.  include/bdd_mma.h: bddmma_get_solver_costs_batch."""
        if out is not None:
            out = tuple(out)
            assert len(out) == 3 and all(x is None or _is_dev(x) for x in out), "out: three device buffers (or None)"
            ptrs, _ = self._costs_args(list(out), "get_solver_costs")
            self._check(self._L.bddmma_get_solver_costs_batch(self._h, *ptrs, 1), self._h)
            return out
        n = sum(s.nr_layers() for s in self.solvers)
        lo, hi, mm = (np.zeros(n, self.solvers[0].value_type) for _ in range(3))
        self._check(self._L.bddmma_get_solver_costs_batch(self._h, _ptr(lo), _ptr(hi), _ptr(mm), 0), self._h)
        return lo, hi, mm

    # ---- the tail of a training step's loss (include/bdd_mma.h: bddmma_lower_bound_per_bdd_batch and the two entries behind it)
    def lower_bound_per_bdd(self, out=None):
        """lower_bound_per_bdd() of every member in one launch: the members' REAL[nr_bdds] one behind the other in the members' order.
        out: a device buffer, written in the batch stream's order (the host does not wait); without it a new NumPy array."""
        nb = sum(s.nr_bdds() for s in self.solvers)
        vt = self.solvers[0].value_type
        if out is not None:
            assert _is_dev(out), "out: a device buffer"
            self._check(self._L.bddmma_lower_bound_per_bdd_batch(self._h, _dev_ptr(out, nb, vt), 1), self._h)
            return out
        out = np.zeros(nb, vt)
        self._check(self._L.bddmma_lower_bound_per_bdd_batch(self._h, _ptr(out), 0), self._h)
        return out

    def grad_lower_bound_per_bdd(self, grad_lb, out=None):
        """grad_lower_bound_per_bdd(grad_lb_i) of every member i, one workgroup per member: (grad_lo, grad_hi), the members' REAL[nr_layers]
        one behind the other; grad_lb: the members' REAL[nr_bdds] one behind the other.  A device tensor needs out = (grad_lo, grad_hi)
        device buffers, a NumPy array gives two new NumPy arrays."""
        n = sum(s.nr_layers() for s in self.solvers)
        nb = sum(s.nr_bdds() for s in self.solvers)
        vt = self.solvers[0].value_type
        call = self._L.bddmma_grad_lower_bound_per_bdd_batch
        if _is_dev(grad_lb):
            assert out is not None and len(out) == 2 and all(_is_dev(x) for x in out), "device gradients need device output buffers: out=(grad_lo, grad_hi)"
            self._check(call(self._h, _dev_ptr(grad_lb, nb, vt), _dev_ptr(out[0], n, vt), _dev_ptr(out[1], n, vt), 1), self._h)
            return out[0], out[1]
        g = np.ascontiguousarray(grad_lb, dtype=vt)
        assert g.size == nb, f"expected {nb} values, got {g.size}"
        lo, hi = np.zeros(n, vt), np.zeros(n, vt)
        self._check(call(self._h, _ptr(g), _ptr(lo), _ptr(hi), 0), self._h)
        return lo, hi

    def distribute_delta(self):
        """distribute_delta() of every member in one launch; a member's grad_distribute_delta() afterwards refers to it"""
        self._check(self._L.bddmma_distribute_delta_batch(self._h), self._h)

    # ---- the min-marginal differences and their gradient (include/bdd_mma.h: bddmma_min_marginal_diff_batch and the entry behind it)
    def min_marginal_diff(self, out=None):
        """min_marginal_diff() of every member, one workgroup per member: the members' REAL[nr_layers] one behind the other in the
        members' order.  out: a device buffer, written in the batch stream's order (the host does not wait); without it a new NumPy array."""
        n = sum(s.nr_layers() for s in self.solvers)
        vt = self.solvers[0].value_type
        if out is not None:
            assert _is_dev(out), "out: a device buffer"
            self._check(self._L.bddmma_min_marginal_diff_batch(self._h, _dev_ptr(out, n, vt), 1), self._h)
            return out
        out = np.zeros(n, vt)
        self._check(self._L.bddmma_min_marginal_diff_batch(self._h, _ptr(out), 0), self._h)
        return out

    def grad_all_min_marginal_differences(self, grad_mm, out=None):
        """grad_all_min_marginal_differences(grad_mm_i) of every member i, one workgroup per member: (grad_lo, grad_hi); all three are the
        members' REAL[nr_layers] one behind the other.  A device tensor needs out = (grad_lo, grad_hi) device buffers, a NumPy array gives
        two new NumPy arrays."""
        n = sum(s.nr_layers() for s in self.solvers)
        vt = self.solvers[0].value_type
        call = self._L.bddmma_grad_min_marginal_diff_batch
        if _is_dev(grad_mm):
            assert out is not None and len(out) == 2 and all(_is_dev(x) for x in out), "device gradients need device output buffers: out=(grad_lo, grad_hi)"
            self._check(call(self._h, _dev_ptr(grad_mm, n, vt), _dev_ptr(out[0], n, vt), _dev_ptr(out[1], n, vt), 1), self._h)
            return out[0], out[1]
        g = np.ascontiguousarray(grad_mm, dtype=vt)
        assert g.size == n, f"expected {n} values, got {g.size}"
        lo, hi = np.zeros(n, vt), np.zeros(n, vt)
        self._check(call(self._h, _ptr(g), _ptr(lo), _ptr(hi), 0), self._h)
        return lo, hi

    # ---- sum-marginals, smooth solutions and the smooth bound gradient (include/bdd_mma.h: bddmma_sum_marginals_batch and the two entries behind it)
    def sum_marginals_cuda(self, get_log_probs=True, out=None):
        """sum_marginals_cuda(get_sorted=False, get_log_probs) of every member, one workgroup per member: (sm_lo, sm_hi), the members'
        REAL[nr_layers] one behind the other in the members' order, each in the unsorted layer order (a member's
        get_primal_variable_index() names the variables).  out: (sm_lo, sm_hi) device buffers, written in the batch stream's order (the
        host does not wait); without it two new NumPy arrays."""
        n = sum(s.nr_layers() for s in self.solvers)
        vt = self.solvers[0].value_type
        call = self._L.bddmma_sum_marginals_batch
        if out is not None:
            assert len(out) == 2 and all(_is_dev(x) for x in out), "out: (sm_lo, sm_hi) device buffers"
            self._check(call(self._h, 1 if get_log_probs else 0, _dev_ptr(out[0], n, vt), _dev_ptr(out[1], n, vt), 1), self._h)
            return out[0], out[1]
        lo, hi = np.zeros(n, vt), np.zeros(n, vt)
        self._check(call(self._h, 1 if get_log_probs else 0, _ptr(lo), _ptr(hi), 0), self._h)
        return lo, hi

    def smooth_solution_per_bdd(self, out=None):
        """smooth_solution_per_bdd() of every member, one workgroup per member: the members' REAL[nr_layers] one behind the other.
        out: a device buffer, written in the batch stream's order (the host does not wait); without it a new NumPy array."""
        n = sum(s.nr_layers() for s in self.solvers)
        vt = self.solvers[0].value_type
        if out is not None:
            assert _is_dev(out), "out: a device buffer"
            self._check(self._L.bddmma_smooth_solution_batch(self._h, _dev_ptr(out, n, vt), 1), self._h)
            return out
        out = np.zeros(n, vt)
        self._check(self._L.bddmma_smooth_solution_batch(self._h, _ptr(out), 0), self._h)
        return out

    def grad_smooth_lower_bound_per_bdd(self, grad_lb, out=None):
        """grad_smooth_lower_bound_per_bdd(grad_lb_i) of every member i, one workgroup per member: (grad_lo, grad_hi), the members'
        REAL[nr_layers] one behind the other; grad_lb: the members' REAL[nr_bdds] one behind the other.  A device tensor needs
        out = (grad_lo, grad_hi) device buffers, a NumPy array gives two new NumPy arrays."""
        n = sum(s.nr_layers() for s in self.solvers)
        nb = sum(s.nr_bdds() for s in self.solvers)
        vt = self.solvers[0].value_type
        call = self._L.bddmma_grad_smooth_lower_bound_per_bdd_batch
        if _is_dev(grad_lb):
            assert out is not None and len(out) == 2 and all(_is_dev(x) for x in out), "device gradients need device output buffers: out=(grad_lo, grad_hi)"
            self._check(call(self._h, _dev_ptr(grad_lb, nb, vt), _dev_ptr(out[0], n, vt), _dev_ptr(out[1], n, vt), 1), self._h)
            return out[0], out[1]
        g = np.ascontiguousarray(grad_lb, dtype=vt)
        assert g.size == nb, f"expected {nb} values, got {g.size}"
        lo, hi = np.zeros(n, vt), np.zeros(n, vt)
        self._check(call(self._h, _ptr(g), _ptr(lo), _ptr(hi), 0), self._h)
        return lo, hi

    # ---- primal rounding (include/bdd_mma.h: bddmma_perturb_primal_costs_batch, bddmma_incremental_mm_agreement_rounding_batch)
    def perturb_primal_costs(self, delta, round_index=0, seed=0):
        """perturb_primal_costs(delta, round_index, seed) of every member, one workgroup per member in one launch per wave count
        present: a list of the per-member dicts of bdd_hip_parallel_mma.perturb_primal_costs (sol is zero where the member's
        min-marginals did not agree)"""
        nv = [s.nr_variables() for s in self.solvers]
        off = np.cumsum([0] + nv)
        vt = self.solvers[0].value_type
        counts = np.zeros(4 * len(nv), np.uint32)
        sol = np.zeros(int(off[-1]), np.int8)
        c0, c1 = np.zeros(int(off[-1]), vt), np.zeros(int(off[-1]), vt)
        self._check(self._L.bddmma_perturb_primal_costs_batch(self._h, float(delta), int(round_index), int(seed),
                                                              counts.ctypes.data_as(C.POINTER(C.c_uint32)), _ptr(sol), _ptr(c0), _ptr(c1)), self._h)
        return [dict(counts=tuple(int(c) for c in counts[4 * i:4 * i + 4]), sol=sol[off[i]:off[i + 1]].copy(),
                     cost_delta_0=c0[off[i]:off[i + 1]].copy(), cost_delta_1=c1[off[i]:off[i + 1]].copy()) for i in range(len(nv))]

    def primal_rounding_incremental(self, init_delta, delta_growth_rate, num_itr_lb, num_rounds=500, seed=0, return_rounds=False):
        """primal_rounding_incremental(...) of every member (not verbose), every round one launch per wave count present and the
        iterations in between those of run_solver on the members still looking: a list of per-member solutions, each a list of
        0.0 / 1.0 per variable, empty where none was found.  The costs stay perturbed.  return_rounds: also the round index in which
        each member's agreement was seen (num_rounds where none was)."""
        nv = [s.nr_variables() for s in self.solvers]
        off = np.cumsum([0] + nv)
        sol = np.zeros(int(off[-1]), np.int8)
        found = (C.c_int * len(nv))()
        rounds = (C.c_uint64 * len(nv))()
        self._check(self._L.bddmma_incremental_mm_agreement_rounding_batch(self._h, float(init_delta), float(delta_growth_rate), int(num_itr_lb),
                                                                           int(num_rounds), int(seed), _ptr(sol), found, rounds), self._h)
        sols = [[float(x) for x in sol[off[i]:off[i + 1]]] if found[i] else [] for i in range(len(nv))]
        return (sols, [int(r) for r in rounds]) if return_rounds else sols

    # ---- per-BDD solutions, cost updates and the gradient of a cost perturbation (include/bdd_mma.h: bddmma_bdds_solution_batch and the two
    # entries behind it)
    def bdds_solution_vec(self, out=None):
        """bdds_solution_vec() of every member, one workgroup per member: the arg-min path of every BDD as int8 0 / 1 per layer, the
        members' [nr_layers] one behind the other in the members' order.  out: an int8 device buffer, written in the batch stream's order
        (the host does not wait); without it a new NumPy int8 array."""
        n = sum(s.nr_layers() for s in self.solvers)
        if out is not None:
            assert _is_dev(out), "out: a device buffer"
            self._check(self._L.bddmma_bdds_solution_batch(self._h, _dev_ptr(out, n, np.int8), 1), self._h)
            return out
        out = np.zeros(n, np.int8)
        self._check(self._L.bddmma_bdds_solution_batch(self._h, _ptr(out), 0), self._h)
        return out

    def update_costs(self, cost_delta_0, cost_delta_1):
        """update_costs(cost_delta_0_i, cost_delta_1_i) of every member i in one launch: the members' [nr_variables] one behind the other in
        the members' order, every layer of a variable gets its value / nr_bdds(variable).  Device tensors of the members' precision take
        the device path (the host does not wait); host arrays are passed as float64, as the member method passes them.  None leaves
        that side of every member's costs as it is."""
        nv = sum(s.nr_variables() for s in self.solvers)
        given = [x for x in (cost_delta_0, cost_delta_1) if x is not None]
        dev = bool(given) and _is_dev(given[0])
        if any(_is_dev(x) != dev for x in given):
            raise capi.BddMmaError(f"bdd_mma error {capi.ERR_INVALID_ARGUMENT}: the arrays of a batch call must all be on the host or all "
                                   "on the device")
        s0 = self.solvers[0]
        if dev:
            ptrs = [None if x is None else _dev_ptr(x, nv, s0.value_type) for x in (cost_delta_0, cost_delta_1)]
            self._check(self._L.bddmma_update_costs_batch(self._h, *ptrs, s0._prec, 1), self._h)
            return
        arrays = [None if x is None else np.ascontiguousarray(x, dtype=np.float64) for x in (cost_delta_0, cost_delta_1)]
        for x in arrays:
            assert x is None or x.size == nv, f"update_costs: expected {nv} values, got {x.size}"
        self._check(self._L.bddmma_update_costs_batch(self._h, *(_ptr(x) for x in arrays), capi.F64, 0), self._h)

    def grad_cost_perturbation(self, grad_lo, grad_hi, out=None):
        """grad_cost_perturbation(grad_lo_i, grad_hi_i) of every member i in one launch: (grad_lo_pert, grad_hi_pert), the members'
        REAL[nr_variables] one behind the other; grad_lo / grad_hi: the members' REAL[nr_layers] one behind the other.  Device tensors
        need out = (lo_pert, hi_pert) device buffers, NumPy arrays give two new NumPy arrays."""
        n = sum(s.nr_layers() for s in self.solvers)
        nv = sum(s.nr_variables() for s in self.solvers)
        vt = self.solvers[0].value_type
        call = self._L.bddmma_grad_cost_perturbation_batch
        if _is_dev(grad_lo) or _is_dev(grad_hi):
            assert _is_dev(grad_lo) and _is_dev(grad_hi), "the arrays of a batch call must all be on the host or all on the device"
            assert out is not None and len(out) == 2 and all(_is_dev(x) for x in out), "device gradients need device output buffers: out=(lo_pert, hi_pert)"
            self._check(call(self._h, _dev_ptr(grad_lo, n, vt), _dev_ptr(grad_hi, n, vt), _dev_ptr(out[0], nv, vt), _dev_ptr(out[1], nv, vt), 1), self._h)
            return out[0], out[1]
        g = [np.ascontiguousarray(x, dtype=vt) for x in (grad_lo, grad_hi)]
        for x in g:
            assert x.size == n, f"expected {n} values, got {x.size}"
        lo, hi = np.zeros(nv, vt), np.zeros(nv, vt)
        self._check(call(self._h, _ptr(g[0]), _ptr(g[1]), _ptr(lo), _ptr(hi), 0), self._h)
        return lo, hi

    # ---- ordering against other streams (include/bdd_mma.h: bddmma_stream_wait_batch / bddmma_stream_signal_batch)
    def stream_wait(self, hip_stream=0):
        """what the batch's calls queue from now on starts after everything queued so far on `hip_stream` (a raw hipStream_t as an
        integer, e.g. torch.cuda.current_stream().cuda_stream; 0 / None: the default stream).  The host does not wait."""
        self._check(self._L.bddmma_stream_wait_batch(self._h, C.c_void_p(int(hip_stream or 0))), self._h)

    def stream_signal(self, hip_stream=0):
        """the reverse: what is queued on `hip_stream` from now on starts after everything the batch's calls have queued so far"""
        self._check(self._L.bddmma_stream_signal_batch(self._h, C.c_void_p(int(hip_stream or 0))), self._h)

    def time_iterations(self, n, omega=0.5) -> float:
        """iterations(n) between hipEvents on the batch's stream (first launch to last): elapsed device milliseconds"""
        ms = C.c_double()
        self._check(self._L.bddmma_batch_time_iterations(self._h, float(omega), int(n), C.byref(ms)), self._h)
        return ms.value

    def run_solver(self, max_iter=1000, tolerance=1e-6, improvement_slope=1e-9, time_limit=3600.0):
        """run_solver() of every member, each stopping on its own criterion: a list of dicts shaped like run_solver()'s; `seconds` is
        the batch's wall time, the time limit one clock for the whole batch"""
        res = (capi.RunResult * len(self.solvers))()
        self._check(self._L.bddmma_batch_run_solver(self._h, int(max_iter), float(tolerance), float(improvement_slope), float(time_limit), res),
                    self._h)
        return [dict(iterations=int(r.iterations), lb_initial=r.lb_initial, lb_final=r.lb_final, seconds=r.seconds,
                     stop_reason=int(r.stop_reason)) for r in res]

    def lower_bounds(self, out=None):
        """lower_bound() of every member in one launch per wave count present: float64[len(solvers)] in the members' order.  out: a
        device tensor of float64 — the bounds are written to it on the batch's stream, the host does not wait, and it is returned.
        include/bdd_mma.h: bddmma_lower_bound_batch."""
        n = len(self.solvers)
        if out is not None:
            if not _is_dev(out):
                raise capi.BddMmaError(f"bdd_mma error {capi.ERR_INVALID_ARGUMENT}: lower_bounds(out=...) takes a device tensor")
            self._check(self._L.bddmma_lower_bound_batch(self._h, C.cast(_dev_ptr(out, n, np.float64), C.POINTER(C.c_double)), 1), self._h)
            return out
        out = np.empty(n, dtype=np.float64)
        self._check(self._L.bddmma_batch_lower_bounds(self._h, out.ctypes.data_as(C.POINTER(C.c_double))), self._h)
        return out


def run_solver(solver, max_iter=1000, tolerance=1e-6, improvement_slope=1e-9, time_limit=3600.0, verbose=False,
               lbfgs: bdd_hip_lbfgs = None, host_loop: bool = False):
    """run_solver<SOLVER>() of include/run_solver_util.h:10-77 (executed inside the library).  host_loop: the reference's literal loop
    (a host round trip for the bound every iteration) instead of the device-resident one; same result."""
    L = capi.lib()
    res = capi.RunResult()
    base = solver.solver if isinstance(solver, bdd_hip_lbfgs) else solver
    lb = solver if isinstance(solver, bdd_hip_lbfgs) else lbfgs
    capi.check((L.bddmma_run_solver_host_loop if host_loop else L.bddmma_run_solver)(base._h, lb._h if lb else None, int(max_iter), float(tolerance),
                                   float(improvement_slope), float(time_limit), 1 if verbose else 0, C.byref(res)), base._h)
    return dict(iterations=int(res.iterations), lb_initial=res.lb_initial, lb_final=res.lb_final,
                seconds=res.seconds, stop_reason=int(res.stop_reason))
