// solver_bp.hpp — a batch's per-BDD solutions, cost updates and the gradient of a cost perturbation (kernels/batchsol.hpp:
// k_small_solution_batch, k_small_update_batch, k_small_grad_perturb_batch).  Included by solver_bp_f32.hip / solver_bp_f64.hip only, so
// that these kernels compile in translation units of their own, beside the batch's other kernels (solver_bt_*.hip, solver_bb_*.hip, ...).
#pragma once
#include "kernels.hpp"
#include "kernels/batchsol.hpp"

namespace bddmma {

// The solution kernel for members of `nw` waves (BatchT::bdds_solution groups its members by it, as the bound gradient does).
template <typename REAL>
SolutionFn<REAL> solution_fn(int nw)
{
    switch (nw) {
        case 1: return &k_small_solution_batch<REAL, 1>;
        case 2: return &k_small_solution_batch<REAL, 2>;
        case 4: return &k_small_solution_batch<REAL, 4>;
        case 8: return &k_small_solution_batch<REAL, 8>;
        default: return &k_small_solution_batch<REAL, 16>;
    }
}
// TIN: the element type of the caller's vectors (bddmma_update_costs_batch: elem_precision)
template <typename REAL, typename TIN>
PerturbUpdateFn<REAL, TIN> perturb_update_fn()
{
    return &k_small_update_batch<REAL, TIN>;
}
template <typename REAL>
PerturbGradFn<REAL> perturb_grad_fn()
{
    return &k_small_grad_perturb_batch<REAL>;
}
template <typename REAL>
PerturbCheckFn<REAL> perturb_check_fn()
{
    return &k_small_grad_perturb_check<REAL>;
}

}  // namespace bddmma
