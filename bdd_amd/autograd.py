"""torch autograd Functions over the learned solver's operators: the layer that trains through `bdd_hip_parallel_mma`.

Import it explicitly (`import bdd_amd.autograd`); `import bdd_amd` does not import torch.  The names, the argument order and the
semantics are those of the reference's torch layer (src/bdd_cuda_torch/bdd_cuda_torch.py; every function cites the lines it
mirrors); the differences are the ones include/bdd_mma.h has from the reference's solver classes and are listed here.

Conventions of every function
  solvers     a list of bdd_hip_parallel_mma of one precision on one device, or a bdd_hip_batch: its members in order.  (The chain of
              a training step's loss — DualIterations, DistributeDeferredDelta and ComputeLowerBoundperBDD, forward and backward —
              makes batch calls on a batch, with the results of the list form, and so do ComputeAllMinMarginalsDiff, GetSumMarginals,
              GetMarginalProbability, ComputePrimalSolution, ComputePerBDDSolutions and PerturbPrimalCosts; only the backward of
              ComputeLowerBoundperBDD with smooth_gradients_temp > 0 does with a batch what it does with the list of its members.)
  tensors     1-D, contiguous, on the solvers' device, of the solvers' precision (torch.float32 / torch.float64 — the reference asks for
              torch's default dtype instead).  A batch tensor is the concatenation over the solvers, in list order, of each solver's array:
                per layer     nr_layers() values in the public layer order (get_solver_costs, get_primal_variable_index) — there are
                              no terminal layers, unlike the reference;
                per BDD       nr_bdds() values in the order of lower_bound_per_bdd;
                per variable  nr_variables() values (the reference has one more per solver, for its terminal).
              batch_index(solvers) gives the offsets and the (variable, BDD) of every layer with the offsets applied.
  refusals    a tensor that breaks any of this raises ValueError naming the argument before any solver is touched.  What the library
              itself refuses (a NaN in an incoming gradient, a negative weight, a call while an L-BFGS wrapper is attached:
              BDDMMA_ERR_STATE) surfaces as bdd_amd.capi.BddMmaError with the library's message.
  state       the tensors are the truth and a solver is a workspace: every forward and every backward first sets the solver's costs
              from its (saved) input tensors, so Functions on the same solvers may be interleaved freely.  Each call leaves a solver in
              the state the C-ABI call it makes documents (include/bdd_mma.h); no Function relies on what another left there.
  streams     a handle runs on its own stream.  Every function makes each handle's stream wait for torch's current stream before its
              first call on the solver (stream_wait) and torch's current stream wait for the handle's afterwards (stream_signal), so
              that no caller has to synchronise: inputs written by kernels still queued on the current stream are read after them,
              outputs are read after they are written, and memory of an input that torch's caching allocator reuses later is not
              overwritten while a handle still reads it.  Use the same current stream for a Function's forward and for what consumes
              its outputs, as with any torch operator.  DualIterations' two batched paths make batch calls only, which run on the
              batch's own stream and order themselves against every member's: there the one pair is the batch's (bdd_hip_batch.stream_wait
              / stream_signal) instead of a pair per member.  The same holds for the batched forms of DistributeDeferredDelta,
              ComputeLowerBoundperBDD, ComputeAllMinMarginalsDiff, GetSumMarginals, GetMarginalProbability,
              ComputePerBDDSolutions and PerturbPrimalCosts.
Every backward is once_differentiable, takes a missing incoming gradient (None) as zeros and runs on the stream that is current
when autograd calls it.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np
import torch
from torch.autograd.function import once_differentiable

from . import capi
from .solver import bdd_hip_batch

__all__ = ["batch_index", "BatchIndex", "DualIterations", "DistributeDeferredDelta", "ComputeAllMinMarginalsDiff", "PerturbPrimalCosts",
           "ComputeLowerBoundperBDD", "ComputePerBDDSolutionsIdentityBackward", "ComputePerBDDSolutions", "GetSumMarginals",
           "GetMarginalProbability", "ComputePrimalSolution"]

BatchIndex = namedtuple("BatchIndex", "layer_offsets bdd_offsets variable_offsets layer_variables layer_bdds")
BatchIndex.__doc__ = """layer_offsets / bdd_offsets / variable_offsets: len(solvers) + 1 Python ints each, solver i owns [off[i], off[i + 1]) of a
per-layer / per-BDD / per-variable batch tensor.  layer_variables / layer_bdds: int64 tensors over the batch's layers holding the
variable / BDD of every layer as an index into the per-variable / per-BDD batch tensors (the solver's own index plus its offset)."""


class _Sizes:
    """what a list of solvers asks of the batch tensors; raises ValueError for a list no batch can be formed from"""

    def __init__(self, solvers):
        self.batch = solvers if isinstance(solvers, bdd_hip_batch) else None
        self.solvers = list(solvers.solvers if self.batch is not None else solvers)
        if not self.solvers:
            raise ValueError("solvers: the list is empty")
        types = {np.dtype(s.value_type) for s in self.solvers}
        if len(types) != 1:
            raise ValueError("solvers: all solvers must have one precision, got " + " and ".join(sorted(t.name for t in types)))
        self.dtype = torch.float64 if types.pop() == np.float64 else torch.float32
        devices = {int(s.device()) for s in self.solvers}
        if len(devices) != 1:
            raise ValueError(f"solvers: all solvers must be on one device, got devices {sorted(devices)}")
        self.device = devices.pop()
        self.layers = _offsets(s.nr_layers() for s in self.solvers)
        self.bdds = _offsets(s.nr_bdds() for s in self.solvers)
        self.variables = _offsets(s.nr_variables() for s in self.solvers)

    def check(self, *args):
        """every (name, tensor, offsets[, allow_scalar]) is a batch tensor over `offsets` (or, with allow_scalar, holds one value): type,
        dtype, shape and contiguity of all of them first, then the device of each; returns the first tensor"""
        for name, t, offsets, *scalar in args:
            n = offsets[-1]
            if not isinstance(t, torch.Tensor):
                raise ValueError(f"{name} must be a torch tensor, got {type(t).__name__}")
            if t.dtype != self.dtype:
                raise ValueError(f"{name} is {t.dtype}, the solvers' values are {self.dtype}")
            if not (scalar and scalar[0] and t.numel() == 1 and t.dim() <= 1):
                if t.dim() != 1:
                    raise ValueError(f"{name} has {t.dim()} dimensions, a batch tensor has one")
                if t.numel() != n:
                    raise ValueError(f"{name} has {t.numel()} values, the solvers need {n}" + (" (or one)" if scalar and scalar[0] else ""))
            if not t.is_contiguous():
                raise ValueError(f"{name} must be contiguous")
        for name, t, *_ in args:
            if not t.is_cuda or t.device.index != self.device:
                raise ValueError(f"{name} is on {t.device}, the solvers are on device {self.device}")
        return args[0][1]

    def slices(self, offsets):
        return [slice(a, b) for a, b in zip(offsets[:-1], offsets[1:])]


def _offsets(counts):
    out = [0]
    for c in counts:
        out.append(out[-1] + int(c))
    return out


def batch_index(solvers, device=None):
    """The offsets of a batch of solvers and what a GNN indexes with (BatchIndex).  The index tensors are built on the host and moved
    to `device` when one is given."""
    solvers = list(solvers.solvers if isinstance(solvers, bdd_hip_batch) else solvers)
    layers = _offsets(s.nr_layers() for s in solvers)
    bdds = _offsets(s.nr_bdds() for s in solvers)
    variables = _offsets(s.nr_variables() for s in solvers)
    lv = [torch.from_numpy(np.asarray(s.get_primal_variable_index(), np.int64) + v) for s, v in zip(solvers, variables)]
    lb = [torch.from_numpy(np.asarray(s.get_bdd_index(), np.int64) + b) for s, b in zip(solvers, bdds)]
    cat = lambda xs: torch.cat(xs) if xs else torch.zeros(0, dtype=torch.int64)
    lv, lb = cat(lv), cat(lb)
    if device is not None:
        lv, lb = lv.to(device), lb.to(device)
    return BatchIndex(layers, bdds, variables, lv, lb)


class _Ordered:
    """`with _Ordered(solvers):` — each handle's stream waits for torch's current stream on entry, and the current stream for each
    handle's on exit (also when a call raised: what it queued still reads the tensors).  Everything torch itself has to queue for the
    call (zero fills, clones) is queued before the block is entered."""

    def __init__(self, solvers):
        self.solvers = solvers

    def __enter__(self):
        self.stream = torch.cuda.current_stream().cuda_stream
        for s in self.solvers:
            s.stream_wait(self.stream)
        return self

    def __exit__(self, *exc):
        for s in self.solvers:
            s.stream_signal(self.stream)
        return False


def _batch_first(call, *args, also=(), **kwargs):
    """the first call of a batched path: False when the batch refuses it with BDDMMA_ERR_STATE — a member that has (had) an L-BFGS
    wrapper, for instance, with which the list form works — or with one of the codes in `also`; the refusal has touched nothing, so the
    caller runs the list form instead."""
    try:
        call(*args, **kwargs)
    except capi.BddMmaError as e:
        if any(str(e).startswith(f"bdd_mma error {code}:") for code in (capi.ERR_STATE, *also)):
            return False
        raise
    return True


def _batch_set_costs(batch, lo, hi, mm):
    """the first call of a batched tail (DistributeDeferredDelta, ComputeLowerBoundperBDD, ...): batch.set_solver_costs"""
    return _batch_first(batch.set_solver_costs, lo, hi, mm)


def _incoming(g, like):
    """an incoming gradient as a contiguous tensor; None (set_materialize_grads(False)) is zeros"""
    return torch.zeros_like(like) if g is None else g.contiguous()


# ---- plain helpers (bdd_cuda_torch.py:12-59) -------------------------------------------------------------------------------------------

def ComputePrimalSolution(solvers, lo_costs_batch, hi_costs_batch, def_mm_batch, init_delta, delta_growth_rate, num_itr_lb, verbose=False):
    """bdd_cuda_torch.py:12-20: sets every solver's costs and rounds with the incremental min-marginal agreement rounding
    (bddmma_incremental_mm_agreement_rounding); a list with one solution (a list of 0.0 / 1.0 per variable, empty when none was found)
    per solver.  The solvers' costs stay perturbed, as in the reference.  For a bdd_hip_batch ONE batch.set_solver_costs and ONE
    batch.primal_rounding_incremental (bddmma_incremental_mm_agreement_rounding_batch: every round one workgroup per member), none on a
    member, with the list form's results bit for bit.  The list form runs for a list, with verbose, and for a batch whose first call
    refuses with BDDMMA_ERR_STATE."""
    z = _Sizes(solvers)
    z.check(("lo_costs_batch", lo_costs_batch, z.layers), ("hi_costs_batch", hi_costs_batch, z.layers), ("def_mm_batch", def_mm_batch, z.layers))
    if z.batch is not None and not verbose:
        with _Ordered([z.batch]):
            batched = _batch_set_costs(z.batch, lo_costs_batch, hi_costs_batch, def_mm_batch)
            if batched:
                out = z.batch.primal_rounding_incremental(init_delta, delta_growth_rate, num_itr_lb)
        if batched:
            return out
    out = []
    with _Ordered(z.solvers):
        for s, l in zip(z.solvers, z.slices(z.layers)):
            s.set_solver_costs(lo_costs_batch[l], hi_costs_batch[l], def_mm_batch[l])
            out.append(s.primal_rounding_incremental(init_delta, delta_growth_rate, num_itr_lb, verbose))
    return out


def _with_costs(solvers, lo_costs_batch, hi_costs_batch):
    z = _Sizes(solvers)
    z.check(("lo_costs_batch", lo_costs_batch, z.layers), ("hi_costs_batch", hi_costs_batch, z.layers))
    return z, torch.zeros_like(lo_costs_batch)


def GetMarginalProbability(solvers, lo_costs_batch, hi_costs_batch):
    """bdd_cuda_torch.py:22-30: the smooth solution (smooth_solution_per_bdd) per layer, deferred differences zero.  For a bdd_hip_batch
    ONE batch.set_solver_costs and ONE batch.smooth_solution_per_bdd (bddmma_smooth_solution_batch: one workgroup per member), none on a
    member, with the list form's results bit for bit.  The list form runs for a list, and for a batch whose first call refuses with
    BDDMMA_ERR_STATE."""
    z, zero = _with_costs(solvers, lo_costs_batch, hi_costs_batch)
    prob_hi = torch.empty_like(lo_costs_batch)
    if z.batch is not None:
        with _Ordered([z.batch]):
            batched = _batch_set_costs(z.batch, lo_costs_batch, hi_costs_batch, zero)
            if batched:
                z.batch.smooth_solution_per_bdd(out=prob_hi)
        if batched:
            return prob_hi
    with _Ordered(z.solvers):
        for s, l in zip(z.solvers, z.slices(z.layers)):
            s.set_solver_costs(lo_costs_batch[l], hi_costs_batch[l], zero[l])
            s.smooth_solution_per_bdd(out=prob_hi[l])
    return prob_hi


def GetSumMarginals(solvers, lo_costs_batch, hi_costs_batch, get_logits):
    """bdd_cuda_torch.py:32-41: (sum_marginal_lo, sum_marginal_hi) per layer in the public layer order, logs when get_logits.  For a
    bdd_hip_batch ONE batch.set_solver_costs and ONE batch.sum_marginals_cuda (bddmma_sum_marginals_batch: one workgroup per member),
    none on a member, with the list form's results bit for bit.  The list form runs for a list, and for a batch whose first call refuses
    with BDDMMA_ERR_STATE."""
    z, zero = _with_costs(solvers, lo_costs_batch, hi_costs_batch)
    sm_lo, sm_hi = torch.empty_like(lo_costs_batch), torch.empty_like(hi_costs_batch)
    if z.batch is not None:
        with _Ordered([z.batch]):
            batched = _batch_set_costs(z.batch, lo_costs_batch, hi_costs_batch, zero)
            if batched:
                z.batch.sum_marginals_cuda(bool(get_logits), out=(sm_lo, sm_hi))
        if batched:
            return sm_lo, sm_hi
    var = torch.empty(max(b - a for a, b in zip(z.layers[:-1], z.layers[1:])), dtype=torch.int32, device=lo_costs_batch.device)
    with _Ordered(z.solvers):
        for s, l in zip(z.solvers, z.slices(z.layers)):
            s.set_solver_costs(lo_costs_batch[l], hi_costs_batch[l], zero[l])
            s.sum_marginals_cuda(False, bool(get_logits), out=(var, sm_lo[l], sm_hi[l]))
    return sm_lo, sm_hi


def ComputePerBDDSolutions(solvers, lo_costs_batch, hi_costs_batch):
    """bdd_cuda_torch.py:43-59: the arg-min path of every BDD (bdds_solution_vec) as 0 / 1 in the solvers' precision, per layer.  For a
    bdd_hip_batch ONE batch.set_solver_costs and ONE batch.bdds_solution_vec (bddmma_bdds_solution_batch: one workgroup per member), none
    on a member, with the list form's results bit for bit.  The list form runs for a list, and for a batch whose first call refuses with
    BDDMMA_ERR_STATE."""
    z, zero = _with_costs(solvers, lo_costs_batch, hi_costs_batch)
    sol = torch.empty(z.layers[-1], dtype=torch.int8, device=lo_costs_batch.device)
    if z.batch is not None:
        with _Ordered([z.batch]):
            batched = _batch_set_costs(z.batch, lo_costs_batch, hi_costs_batch, zero)
            if batched:
                z.batch.bdds_solution_vec(out=sol)
        if batched:
            return sol.to(z.dtype)
    with _Ordered(z.solvers):
        for s, l in zip(z.solvers, z.slices(z.layers)):
            s.set_solver_costs(lo_costs_batch[l], hi_costs_batch[l], zero[l])
            s.bdds_solution_vec(out=sol[l])
    return sol.to(z.dtype)


# ---- differentiable operators ------------------------------------------------------------------------------------------------------------

class DualIterations(torch.autograd.Function):
    """bdd_cuda_torch.py:61-182.  apply(solvers, lo_costs_batch, hi_costs_batch, def_mm_batch, dist_weights_batch, num_iterations, omega,
    grad_dual_itr_max_itr, improvement_slope, num_caches, compute_history_for_itrs, history_avg_beta) ->
    (lo, hi, def_mm, sol_avg, lb_first_diff_avg, lb_second_diff_avg).

    forward   learned_iterations on every solver, from the given costs and deferred differences — for a bdd_hip_batch whose members are all
              fused_small_learned(), three batch calls and none on a member: ONE
              batch.set_solver_costs, ONE batch.learned_iterations(_history) and ONE batch.get_solver_costs (the same results: bit-equal in float,
              and in double wherever no variable sits in more than two BDDs).  With improvement_slope > 0 the middle call is ONE
              batch.learned_iterations_stopping where every member is fused_small_stop(): the stopping rule runs inside the members'
              workgroups and the call returns each member's count.  With compute_history_for_itrs > 0 the same three calls
              where every member is fused_small_history() and num_iterations >= compute_history_for_itrs (what the reference asserts):
              the history steps run inside the members' workgroups.  omega is a tensor: one value (the scalar
              call) or one per layer (learned_iterations' omega_vec).  With improvement_slope > 0 the solvers may stop at different
              counts; each count is remembered (ctx.iterations_done), in the batched form from the call's returned counts.  The last three outputs are None unless compute_history_for_itrs > 0 (they start as
              zeros: an entry the history does not reach keeps that) and are not differentiable.
    backward  bddmma_grad_learned_iterations per solver with track_grad_for_num_itr = min(iterations done, grad_dual_itr_max_itr) and
              track_grad_after_itr = done - that: the untracked iterations are treated as constants, as in the reference.  For a
              bdd_hip_batch whose members are all fused_small_learned(), ONE batch.set_solver_costs and ONE batch.grad_iterations
              (bddmma_grad_learned_iterations_batch: one workgroup per member) where they ran the same number of iterations, or ONE
              batch.grad_iterations_counts (bddmma_grad_learned_iterations_counts_batch: every member with its own two counts) where
              they did not — a stopping rule —, instead of that loop, with the same results (bit-equal in float, and in double wherever
              no variable sits in more than two BDDs); with different counts a BDDMMA_ERR_STATE or BDDMMA_ERR_UNSUPPORTED refusal, which
              has touched nothing, gives the loop.  Gradients for
              lo, hi, def_mm, dist_weights and omega; one omega shared by several solvers gets the sum of their values, added in list
              order in the solvers' precision (on the torch side in both forms).  State contract of that call: a solver holds the saved input state on entry (set here) and
              again on return, both sweep states invalid; it refuses with BDDMMA_ERR_STATE (BddMmaError) while an L-BFGS wrapper is
              attached, and with BDDMMA_ERR_INVALID_ARGUMENT for a non-finite incoming gradient or a negative or non-finite weight or
              omega, each time leaving the solver untouched.  The reference's randomize_num_iterations belongs to its training loop and
              is not taken over."""

    @staticmethod
    def forward(ctx, solvers, lo_costs_batch, hi_costs_batch, def_mm_batch, dist_weights_batch, num_iterations, omega, grad_dual_itr_max_itr,
                improvement_slope, num_caches, compute_history_for_itrs, history_avg_beta):
        z = _Sizes(solvers)
        z.check(("lo_costs_batch", lo_costs_batch, z.layers), ("hi_costs_batch", hi_costs_batch, z.layers), ("def_mm_batch", def_mm_batch, z.layers),
                ("dist_weights_batch", dist_weights_batch, z.layers), ("omega", omega, z.layers, True))
        per_layer_omega = omega.numel() != 1
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(lo_costs_batch, hi_costs_batch, def_mm_batch, dist_weights_batch, omega)
        ctx.sizes, ctx.num_caches, ctx.grad_dual_itr_max_itr = z, int(num_caches), int(grad_dual_itr_max_itr)
        lo, hi, mm = (torch.empty_like(lo_costs_batch) for _ in range(3))
        history = int(compute_history_for_itrs)
        sol_avg = lb1 = lb2 = None
        if history > 0:
            sol_avg = torch.zeros_like(lo_costs_batch)
            lb1, lb2 = (torch.zeros(z.bdds[-1], dtype=z.dtype, device=lo_costs_batch.device) for _ in range(2))
            ctx.mark_non_differentiable(sol_avg, lb1, lb2)
        omega_scalar = None if per_layer_omega else float(omega.reshape(-1)[0].item())
        done = []
        stopping = float(improvement_slope) > 0   # the rule inside the members' workgroups: every member fused_small_stop()
        batched = z.batch is not None and all(s.fused_small_stop() if stopping else s.fused_small_learned() for s in z.solvers)
        if batched and history > 0:   # the history inside the members' workgroups; as the reference asserts, no more of it than iterations
            batched = int(num_iterations) >= history and all(s.fused_small_history() for s in z.solvers)
        if batched:
            hist = dict(compute_history_for_itr=history, history_avg_beta=float(history_avg_beta), sol_avg=sol_avg, lb_first_diff_avg=lb1,
                        lb_second_diff_avg=lb2) if history > 0 else {}
            done = [int(num_iterations)] * len(z.solvers)
            with _Ordered([z.batch]):   # batch calls only: each orders itself against the members' streams
                z.batch.set_solver_costs(lo_costs_batch, hi_costs_batch, def_mm_batch)
                if stopping:
                    done = z.batch.learned_iterations_stopping(dist_weights_batch, int(num_iterations), omega=0.5 if per_layer_omega else omega_scalar,
                                                               improvement_slope=float(improvement_slope), omega_vec=omega if per_layer_omega else None,
                                                               **hist)
                else:
                    z.batch.learned_iterations_history(dist_weights_batch, int(num_iterations), omega=0.5 if per_layer_omega else omega_scalar,
                                                       omega_vec=omega if per_layer_omega else None, **hist)
                z.batch.get_solver_costs(out=(lo, hi, mm))
            ctx.iterations_done, ctx.omega_scalar = done, omega_scalar
            return lo, hi, mm, sol_avg, lb1, lb2
        with _Ordered(z.solvers):
            for s, l, b in zip(z.solvers, z.slices(z.layers), z.slices(z.bdds)):
                s.set_solver_costs(lo_costs_batch[l], hi_costs_batch[l], def_mm_batch[l])
                hist = dict(sol_avg=sol_avg[l], lb_first_diff_avg=lb1[b], lb_second_diff_avg=lb2[b]) if history > 0 else {}
                done.append(s.learned_iterations(dist_weights_batch[l], int(num_iterations), omega=0.5 if per_layer_omega else omega_scalar,
                                                 improvement_slope=float(improvement_slope), compute_history_for_itr=history,
                                                 history_avg_beta=float(history_avg_beta), omega_vec=omega[l] if per_layer_omega else None, **hist))
                s.get_solver_costs(out=(lo[l], hi[l], mm[l]))
        ctx.iterations_done, ctx.omega_scalar = done, omega_scalar
        return lo, hi, mm, sol_avg, lb1, lb2

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_lo, grad_hi, grad_def_mm, _sol_avg=None, _lb_first=None, _lb_second=None):
        lo_costs_batch, hi_costs_batch, def_mm_batch, dist_weights_batch, omega = ctx.saved_tensors
        z = ctx.sizes
        # in-out for the library: copies of the incoming gradients
        g_lo, g_hi, g_mm = (torch.zeros_like(lo_costs_batch) if g is None else g.detach().clone(memory_format=torch.contiguous_format)
                            for g in (grad_lo, grad_hi, grad_def_mm))
        z.check(("grad_lo_costs_out", g_lo, z.layers), ("grad_hi_costs_out", g_hi, z.layers), ("grad_def_mm_out", g_mm, z.layers))
        g_w = torch.zeros_like(dist_weights_batch)
        scalar = ctx.omega_scalar is not None
        g_om = torch.zeros(len(z.solvers), dtype=z.dtype, device=omega.device) if scalar else torch.zeros_like(omega)
        done = ctx.iterations_done
        fused = z.batch is not None and all(s.fused_small_learned() for s in z.solvers)
        batched = False
        if fused and len(set(done)) == 1:   # one workgroup per member, every member's arrays at once; g_om[i] is member i's own sum
            batched = True
            with _Ordered([z.batch]):
                z.batch.set_solver_costs(lo_costs_batch, hi_costs_batch, def_mm_batch)
                n = min(done[0], ctx.grad_dual_itr_max_itr)
                z.batch.grad_iterations(dist_weights_batch, g_lo, g_hi, g_mm, omega=ctx.omega_scalar if scalar else 0.5,
                                        track_grad_after_itr=done[0] - n, track_grad_for_num_itr=n, num_caches=ctx.num_caches,
                                        omega_vec=None if scalar else omega, out=(g_w, g_om))
        elif fused:   # the members stopped at different counts: the same two calls, every member with its own
            tracked = [min(d, ctx.grad_dual_itr_max_itr) for d in done]
            with _Ordered([z.batch]):
                batched = _batch_set_costs(z.batch, lo_costs_batch, hi_costs_batch, def_mm_batch)
                if batched:
                    batched = _batch_first(z.batch.grad_iterations_counts, dist_weights_batch, g_lo, g_hi, g_mm, [d - n for d, n in zip(done, tracked)],
                                           tracked, omega=ctx.omega_scalar if scalar else 0.5, num_caches=ctx.num_caches,
                                           omega_vec=None if scalar else omega, out=(g_w, g_om), also=(capi.ERR_UNSUPPORTED,))
        if not batched:
            with _Ordered(z.solvers):
                for i, (s, l) in enumerate(zip(z.solvers, z.slices(z.layers))):
                    s.set_solver_costs(lo_costs_batch[l], hi_costs_batch[l], def_mm_batch[l])
                    n = min(done[i], ctx.grad_dual_itr_max_itr)
                    s.grad_iterations(dist_weights_batch[l], g_lo[l], g_hi[l], g_mm[l], omega=ctx.omega_scalar if scalar else 0.5,
                                      track_grad_after_itr=done[i] - n, track_grad_for_num_itr=n, num_caches=ctx.num_caches,
                                      omega_vec=None if scalar else omega[l], out=(g_w[l], g_om[i:i + 1] if scalar else g_om[l]))
        if scalar:
            total = g_om[0]
            for i in range(1, len(z.solvers)):
                total = total + g_om[i]
            g_om = total.reshape(omega.shape)
        return None, g_lo, g_hi, g_mm, g_w, None, g_om, None, None, None, None, None


class DistributeDeferredDelta(torch.autograd.Function):
    """bdd_cuda_torch.py:184-232.  apply(solvers, lo_costs_batch, hi_costs_batch, def_mm_batch) -> (lo, hi): distribute_delta on every solver.

    forward   for a bdd_hip_batch three batch calls and none on a member: ONE batch.set_solver_costs, ONE batch.distribute_delta and ONE
              batch.get_solver_costs, with the list form's results bit for bit.  The list form runs for a list, and for a batch whose
              first call refuses with BDDMMA_ERR_STATE.

    backward  grad_lo and grad_hi pass through (identity Jacobian) and grad_def_mm = where(def_mm > 0, grad_hi, -grad_lo), formed from
              the saved tensor.  That is what bddmma_grad_distribute_delta computes, but that call reads whatever distribute_delta last
              ran on the handle, and another Function may have used the solver between this forward and this backward.  No solver is
              touched; nothing is refused."""

    @staticmethod
    def forward(ctx, solvers, lo_costs_batch, hi_costs_batch, def_mm_batch):
        z = _Sizes(solvers)
        z.check(("lo_costs_batch", lo_costs_batch, z.layers), ("hi_costs_batch", hi_costs_batch, z.layers), ("def_mm_batch", def_mm_batch, z.layers))
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(def_mm_batch)
        lo, hi = (torch.empty_like(lo_costs_batch) for _ in range(2))
        if z.batch is not None:
            with _Ordered([z.batch]):   # batch calls only: each orders itself against the members' streams
                batched = _batch_set_costs(z.batch, lo_costs_batch, hi_costs_batch, def_mm_batch)
                if batched:
                    z.batch.distribute_delta()
                    z.batch.get_solver_costs(out=(lo, hi, None))
            if batched:
                return lo, hi
        rest = torch.empty_like(lo_costs_batch)
        with _Ordered(z.solvers):
            for s, l in zip(z.solvers, z.slices(z.layers)):
                s.set_solver_costs(lo_costs_batch[l], hi_costs_batch[l], def_mm_batch[l])
                s.distribute_delta()
                s.get_solver_costs(out=(lo[l], hi[l], rest[l]))   # rest: the deferred differences afterwards, all zero
        return lo, hi

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_lo, grad_hi):
        (def_mm_batch,) = ctx.saved_tensors
        g_lo, g_hi = _incoming(grad_lo, def_mm_batch), _incoming(grad_hi, def_mm_batch)
        return None, g_lo, g_hi, torch.where(def_mm_batch > 0, g_hi, -g_lo)


class ComputeAllMinMarginalsDiff(torch.autograd.Function):
    """bdd_cuda_torch.py:234-277.  apply(solvers, lo_costs_batch, hi_costs_batch) -> min_marginal_diff per layer, deferred differences zero.

    forward   for a bdd_hip_batch ONE batch.set_solver_costs and ONE batch.min_marginal_diff (bddmma_min_marginal_diff_batch: one workgroup
              per member), none on a member, with the list form's results bit for bit.  The list form runs for a list, and for a batch
              whose first call refuses with BDDMMA_ERR_STATE.
    backward  bddmma_grad_min_marginal_diff with the saved costs set again; for a bdd_hip_batch likewise ONE batch.set_solver_costs and ONE
              batch.grad_all_min_marginal_differences (bddmma_grad_min_marginal_diff_batch).  State contract of that call: it recomputes
              whichever stored sweep state is invalid and leaves both valid; arc costs, deferred differences and delta are not changed;
              the per-member call works with an L-BFGS wrapper attached; a non-finite incoming gradient is BDDMMA_ERR_INVALID_ARGUMENT
              (BddMmaError)."""

    @staticmethod
    def forward(ctx, solvers, lo_costs_batch, hi_costs_batch):
        z, zero = _with_costs(solvers, lo_costs_batch, hi_costs_batch)
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(lo_costs_batch, hi_costs_batch)
        ctx.sizes = z
        mm_diff = torch.empty_like(lo_costs_batch)
        if z.batch is not None:
            with _Ordered([z.batch]):
                batched = _batch_set_costs(z.batch, lo_costs_batch, hi_costs_batch, zero)
                if batched:
                    z.batch.min_marginal_diff(out=mm_diff)
            if batched:
                return mm_diff
        with _Ordered(z.solvers):
            for s, l in zip(z.solvers, z.slices(z.layers)):
                s.set_solver_costs(lo_costs_batch[l], hi_costs_batch[l], zero[l])
                s.min_marginal_diff(out=mm_diff[l])
        return mm_diff

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_mm_diff):
        lo_costs_batch, hi_costs_batch = ctx.saved_tensors
        z = ctx.sizes
        g = z.check(("grad_mm_diff_batch", _incoming(grad_mm_diff, lo_costs_batch), z.layers))
        zero = torch.zeros_like(lo_costs_batch)
        g_lo, g_hi = torch.empty_like(lo_costs_batch), torch.empty_like(hi_costs_batch)
        if z.batch is not None:
            with _Ordered([z.batch]):
                batched = _batch_set_costs(z.batch, lo_costs_batch, hi_costs_batch, zero)
                if batched:
                    z.batch.grad_all_min_marginal_differences(g, out=(g_lo, g_hi))
            if batched:
                return None, g_lo, g_hi
        with _Ordered(z.solvers):
            for s, l in zip(z.solvers, z.slices(z.layers)):
                s.set_solver_costs(lo_costs_batch[l], hi_costs_batch[l], zero[l])
                s.grad_all_min_marginal_differences(g[l], out=(g_lo[l], g_hi[l]))
        return None, g_lo, g_hi


class PerturbPrimalCosts(torch.autograd.Function):
    """bdd_cuda_torch.py:279-337.  apply(solvers, lo_costs_pert_batch, hi_costs_pert_batch, lo_costs_batch, hi_costs_batch) -> (lo, hi): the
    costs after update_costs(lo_pert, hi_pert) — every layer of a variable gets pert[variable] / nr_bdds(variable).  The perturbations
    are per-variable batch tensors; deferred differences zero.

    forward   for a bdd_hip_batch three batch calls and none on a member: ONE batch.set_solver_costs, ONE batch.update_costs
              (bddmma_update_costs_batch) and ONE batch.get_solver_costs, with the list form's results bit for bit.  The list form runs
              for a list, and for a batch whose first call refuses with BDDMMA_ERR_STATE.
    backward  the identity for lo and hi, bddmma_grad_cost_perturbation for the two perturbations; for a bdd_hip_batch ONE
              batch.grad_cost_perturbation (bddmma_grad_cost_perturbation_batch) instead of a call per member, the list form after a
              BDDMMA_ERR_STATE refusal.  That call reads nothing of the solver but its layout and changes nothing; a non-finite incoming
              gradient is BDDMMA_ERR_INVALID_ARGUMENT (BddMmaError)."""

    @staticmethod
    def forward(ctx, solvers, lo_costs_pert_batch, hi_costs_pert_batch, lo_costs_batch, hi_costs_batch):
        z = _Sizes(solvers)
        z.check(("lo_costs_pert_batch", lo_costs_pert_batch, z.variables), ("hi_costs_pert_batch", hi_costs_pert_batch, z.variables),
                ("lo_costs_batch", lo_costs_batch, z.layers), ("hi_costs_batch", hi_costs_batch, z.layers))
        ctx.set_materialize_grads(False)
        ctx.sizes = z
        ctx.like = (lo_costs_batch.new_empty(0), lo_costs_pert_batch.shape, lo_costs_batch.shape)
        zero = torch.zeros_like(lo_costs_batch)
        lo, hi, rest = (torch.empty_like(lo_costs_batch) for _ in range(3))
        if z.batch is not None:
            with _Ordered([z.batch]):   # batch calls only: each orders itself against the members' streams
                batched = _batch_set_costs(z.batch, lo_costs_batch, hi_costs_batch, zero)
                if batched:
                    z.batch.update_costs(lo_costs_pert_batch, hi_costs_pert_batch)
                    z.batch.get_solver_costs(out=(lo, hi, None))
            if batched:
                return lo, hi
        with _Ordered(z.solvers):
            for s, l, v in zip(z.solvers, z.slices(z.layers), z.slices(z.variables)):
                s.set_solver_costs(lo_costs_batch[l], hi_costs_batch[l], zero[l])
                s.update_costs(lo_costs_pert_batch[v], hi_costs_pert_batch[v])
                s.get_solver_costs(out=(lo[l], hi[l], rest[l]))
        return lo, hi

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_lo, grad_hi):
        z = ctx.sizes
        proto, pert_shape, layer_shape = ctx.like
        g_lo = proto.new_zeros(layer_shape) if grad_lo is None else grad_lo.contiguous()
        g_hi = proto.new_zeros(layer_shape) if grad_hi is None else grad_hi.contiguous()
        z.check(("grad_lo_costs_out", g_lo, z.layers), ("grad_hi_costs_out", g_hi, z.layers))
        p_lo, p_hi = proto.new_empty(pert_shape), proto.new_empty(pert_shape)
        if z.batch is not None:
            with _Ordered([z.batch]):
                batched = _batch_first(z.batch.grad_cost_perturbation, g_lo, g_hi, out=(p_lo, p_hi))
            if batched:
                return None, p_lo, p_hi, g_lo, g_hi
        with _Ordered(z.solvers):
            for s, l, v in zip(z.solvers, z.slices(z.layers), z.slices(z.variables)):
                s.grad_cost_perturbation(g_lo[l], g_hi[l], out=(p_lo[v], p_hi[v]))
        return None, p_lo, p_hi, g_lo, g_hi


class ComputeLowerBoundperBDD(torch.autograd.Function):
    """bdd_cuda_torch.py:339-401.  apply(solvers, lo_costs_batch, hi_costs_batch, smooth_gradients_temp=0.0) -> lower_bound_per_bdd, a per-BDD
    batch tensor; deferred differences zero.

    forward   for a bdd_hip_batch ONE batch.set_solver_costs and ONE batch.lower_bound_per_bdd, none on a member, with the list form's
              results bit for bit.  The list form runs for a list, and for a batch whose first call refuses with BDDMMA_ERR_STATE.
    backward  for a bdd_hip_batch with smooth_gradients_temp <= 0 likewise ONE batch.set_solver_costs and ONE
              batch.grad_lower_bound_per_bdd (bddmma_grad_lower_bound_per_bdd_batch: one workgroup per member).  Otherwise, per solver,
              smooth_gradients_temp <= 0: bddmma_grad_lower_bound_per_bdd (the arg-min path of every BDD; state contract of
              bddmma_bdds_solution).  > 0: the smooth variant on the saved costs divided by the temperature — as in the reference the
              scaling applies to the backward only, the forward value is the plain bound (state contract of bddmma_sum_marginals: both
              sweep states invalid and the cached bound dropped afterwards).  Neither changes arc costs, deferred differences or delta
              beyond the costs set here; both work with an L-BFGS wrapper attached; a non-finite incoming gradient is
              BDDMMA_ERR_INVALID_ARGUMENT (BddMmaError)."""

    @staticmethod
    def forward(ctx, solvers, lo_costs_batch, hi_costs_batch, smooth_gradients_temp=0.0):
        z, zero = _with_costs(solvers, lo_costs_batch, hi_costs_batch)
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(lo_costs_batch, hi_costs_batch)
        ctx.sizes, ctx.temp = z, float(smooth_gradients_temp)
        lb = torch.empty(z.bdds[-1], dtype=z.dtype, device=lo_costs_batch.device)
        if z.batch is not None:
            with _Ordered([z.batch]):
                batched = _batch_set_costs(z.batch, lo_costs_batch, hi_costs_batch, zero)
                if batched:
                    z.batch.lower_bound_per_bdd(out=lb)
            if batched:
                return lb
        with _Ordered(z.solvers):
            for s, l, b in zip(z.solvers, z.slices(z.layers), z.slices(z.bdds)):
                s.set_solver_costs(lo_costs_batch[l], hi_costs_batch[l], zero[l])
                s.lower_bound_per_bdd(out=lb[b])
        return lb

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_lb_per_bdd):
        lo_costs_batch, hi_costs_batch = ctx.saved_tensors
        z = ctx.sizes
        g = torch.zeros(z.bdds[-1], dtype=z.dtype, device=lo_costs_batch.device) if grad_lb_per_bdd is None else grad_lb_per_bdd.contiguous()
        z.check(("grad_lb_per_bdd_batch", g, z.bdds))
        smooth = ctx.temp > 0
        if smooth:
            lo_costs_batch, hi_costs_batch = lo_costs_batch / ctx.temp, hi_costs_batch / ctx.temp
        zero = torch.zeros_like(lo_costs_batch)
        g_lo, g_hi = torch.empty_like(lo_costs_batch), torch.empty_like(hi_costs_batch)
        if z.batch is not None and not smooth:
            with _Ordered([z.batch]):
                batched = _batch_set_costs(z.batch, lo_costs_batch, hi_costs_batch, zero)
                if batched:
                    z.batch.grad_lower_bound_per_bdd(g, out=(g_lo, g_hi))
            if batched:
                return None, g_lo, g_hi, None
        with _Ordered(z.solvers):
            for s, l, b in zip(z.solvers, z.slices(z.layers), z.slices(z.bdds)):
                s.set_solver_costs(lo_costs_batch[l], hi_costs_batch[l], zero[l])
                (s.grad_smooth_lower_bound_per_bdd if smooth else s.grad_lower_bound_per_bdd)(g[b], out=(g_lo[l], g_hi[l]))
        return None, g_lo, g_hi, None


class ComputePerBDDSolutionsIdentityBackward(torch.autograd.Function):
    """bdd_cuda_torch.py:403-430.  apply(solvers, lo_costs_batch, hi_costs_batch, norm_grad) -> ComputePerBDDSolutions (0 / 1 per layer).

    backward  a straight-through estimate, as in the reference: the incoming gradient times norm_grad (a number or a one-element tensor; None:
              1) goes to lo, its negative to hi (the solution falls as hi rises: "negative identity as Jacobian", :428-430).  No solver is
              touched; nothing is refused."""

    @staticmethod
    def forward(ctx, solvers, lo_costs_batch, hi_costs_batch, norm_grad=None):
        ctx.set_materialize_grads(False)
        ctx.norm_grad = norm_grad
        return ComputePerBDDSolutions(solvers, lo_costs_batch, hi_costs_batch)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_solution_hi):
        if grad_solution_hi is None:
            return None, None, None, None
        g = grad_solution_hi if ctx.norm_grad is None else grad_solution_hi * ctx.norm_grad
        return None, g, -g, None
