// kernels/batchsol.hpp — a batch's per-BDD solutions, cost updates and the gradient of a cost perturbation, one launch each (solver_bt.hpp:
// BatchT::bdds_solution, update_costs, grad_cost_perturbation).  k_small_solution_batch: bdds_solution (unsorted) of every member, one
// workgroup per member, wave p on pack p; k_small_update_batch: update_costs of every member; k_small_grad_perturb_batch:
// grad_cost_perturbation of every member.  Not part of kernels.hpp: the kernels are instantiated in solver_bp_f32.hip / solver_bp_f64.hip
// only (solver_bp.hpp); solver_bt.hpp includes this file for the item and the getters.  Behind kernels.hpp.
#pragma once
#include "batchbound.hpp"   // BoundItem, bound_region_bytes, bound_path_pass

namespace bddmma {

// bdds_solution(sorted = 0) of every member, wave p on pack p (n_packs <= NW): the path pass of k_small_grad_lb_batch
// (kernels/batchbound.hpp: bound_path_pass, the pack's region bound_region_bytes) and the decision of each of the pack's layers as a
// char, 0 where no node of the layer is on the path.  A wave reads and writes its own pack's layers only: no workgroup barrier.
template <typename REAL, int NW>
__global__ void __launch_bounds__(64 * NW) k_small_solution_batch(const BoundItem<REAL>* __restrict__ items, char* __restrict__ sol)
{
    constexpr uint32_t S = sizeof(REAL);
    extern __shared__ __attribute__((aligned(16))) unsigned char dyn_lds[];
    const BoundItem<REAL>& it = items[blockIdx.x];
    const uint32_t tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane((int)(tid >> 6));
    const uint32_t lane = tid & 63u;
    const uint32_t p = (uint32_t)wave;
    if (p >= it.n_packs) return;
    uint32_t layer0, nlayers, dc;
    const bool swept = bound_path_pass<REAL>(dyn_lds, it, p, lane, layer0, nlayers, dc);
    char* const o = sol + (size_t)it.src + layer0;
    // (a pack without a hop has no path: its layers, if any, are what the memset of the per-member call leaves)
    for (uint32_t j = lane; j < nlayers; j += 64u) o[j] = swept && lds_ld<REAL>(dyn_lds, dc + j * S) != REAL(0) ? 1 : 0;
}

// What a member's workgroup needs for the two per-variable operators, one entry per member of the batch in the caller's order,
// read-only for the launches.  Member i's values start at `src` in each concatenated layer array and at `src_v` in each concatenated
// per-variable array.
template <typename REAL>
struct PerturbItem {
    REAL* lohi;
    const int32_t* layer_var;     // layer -> variable
    const int32_t* nbdds;         // variable -> number of its BDDs
    const uint32_t* var_ptr;      // variable -> its range in var_layers
    const uint32_t* var_layers;
    uint32_t n_layers, n_vars;
    uint32_t src, src_v;
};

// update_costs(lo_i, hi_i), both full length, of every member i, a workgroup of 256 threads each: per layer the variable's share
// ew_cost_quotient and the sum ew_cost_add (kernels/elementwise.hpp), which k_cost_quotients and k_update_costs evaluate in two
// launches; no flag, as no vector is shorter than nr_variables.  A null side is left alone.  No value is checked, as the per-member call
// checks none.
template <typename REAL, typename TIN>
__global__ void __launch_bounds__(256) k_small_update_batch(const PerturbItem<REAL>* __restrict__ items, const TIN* __restrict__ lo, const TIN* __restrict__ hi)
{
    using P2 = typename Pair<REAL>::type;
    const PerturbItem<REAL>& it = items[blockIdx.x];
    const uint32_t do_lo = lo != nullptr, do_hi = hi != nullptr;
    for (uint32_t l = threadIdx.x; l < it.n_layers; l += 256u) {
        const int v = it.layer_var[l];
        const double nb = (double)it.nbdds[v];
        CostQuot d;
        d.lo = do_lo ? ew_cost_quotient(lo[(size_t)it.src_v + v], nb) : 0.0;
        d.hi = do_hi ? ew_cost_quotient(hi[(size_t)it.src_v + v], nb) : 0.0;
        P2 c = reinterpret_cast<P2*>(it.lohi)[l];
        ew_cost_add<REAL>(c, d, 0u, do_lo, do_hi);
        reinterpret_cast<P2*>(it.lohi)[l] = c;
    }
}

// grad_cost_perturbation of every member, a workgroup of 256 threads each: a thread per variable, ew_grad_perturb
// (kernels/elementwise.hpp: k_grad_perturb's sums and quotient) on the member's part of the caller's arrays.
template <typename REAL>
__global__ void __launch_bounds__(256) k_small_grad_perturb_batch(const PerturbItem<REAL>* __restrict__ items, const REAL* __restrict__ g_lo, const REAL* __restrict__ g_hi,
                                                                  REAL* __restrict__ out_lo, REAL* __restrict__ out_hi)
{
    const PerturbItem<REAL>& it = items[blockIdx.x];
    const REAL* const lo = g_lo + it.src;
    const REAL* const hi = g_hi + it.src;
    for (uint32_t v = threadIdx.x; v < it.n_vars; v += 256u) {
        REAL s0, s1;
        ew_grad_perturb<REAL>(lo, hi, it.var_ptr, it.var_layers, v, s0, s1);
        out_lo[(size_t)it.src_v + v] = s0;
        out_hi[(size_t)it.src_v + v] = s1;
    }
}

// Its argument check: the smallest 2 * member + array (0: grad_lo, 1: grad_hi) with a value that is not finite -> *bad, i.e. the first
// offending member and, of its arrays, the first in the per-member call's order
template <typename REAL>
__global__ void __launch_bounds__(256) k_small_grad_perturb_check(const PerturbItem<REAL>* __restrict__ items, const REAL* __restrict__ g_lo, const REAL* __restrict__ g_hi,
                                                                  uint32_t* __restrict__ bad)
{
    const PerturbItem<REAL>& it = items[blockIdx.x];
    bool b0 = false, b1 = false;
    for (uint32_t l = threadIdx.x; l < it.n_layers; l += 256u) {
        b0 |= !rfinite(g_lo[(size_t)it.src + l]);
        b1 |= !rfinite(g_hi[(size_t)it.src + l]);
    }
    if (b0) atomicMin(bad, 2u * blockIdx.x);
    else if (b1) atomicMin(bad, 2u * blockIdx.x + 1u);
}

// The instantiations (defined in solver_bp.hpp, compiled in solver_bp_f32.hip / _f64.hip): the solution kernel for members of `nw` waves
template <typename REAL>
using SolutionFn = void (*)(const BoundItem<REAL>*, char*);
template <typename REAL, typename TIN>
using PerturbUpdateFn = void (*)(const PerturbItem<REAL>*, const TIN*, const TIN*);
template <typename REAL>
using PerturbGradFn = void (*)(const PerturbItem<REAL>*, const REAL*, const REAL*, REAL*, REAL*);
template <typename REAL>
using PerturbCheckFn = void (*)(const PerturbItem<REAL>*, const REAL*, const REAL*, uint32_t*);
template <typename REAL>
SolutionFn<REAL> solution_fn(int nw);
template <typename REAL, typename TIN>
PerturbUpdateFn<REAL, TIN> perturb_update_fn();
template <typename REAL>
PerturbGradFn<REAL> perturb_grad_fn();
template <typename REAL>
PerturbCheckFn<REAL> perturb_check_fn();

}  // namespace bddmma
