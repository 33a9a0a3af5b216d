// solver_bb.hpp — a batch's per-BDD bounds, their gradient and distribute_delta (kernels/batchbound.hpp: k_small_bounds_batch,
// k_small_grad_lb_batch, k_small_distribute_batch).  Included by solver_bb_f32.hip / solver_bb_f64.hip only, so that these kernels compile
// in translation units of their own, beside the batch's other kernels (solver_bt_*.hip, solver_bc_*.hip, ...).
#pragma once
#include "kernels.hpp"
#include "kernels/batchbound.hpp"

namespace bddmma {

// The gradient kernel for members of `nw` waves (BatchT::grad_lower_bound_per_bdd groups its members by it).
template <typename REAL>
BoundGradFn<REAL> bound_grad_fn(int nw)
{
    switch (nw) {
        case 1: return &k_small_grad_lb_batch<REAL, 1>;
        case 2: return &k_small_grad_lb_batch<REAL, 2>;
        case 4: return &k_small_grad_lb_batch<REAL, 4>;
        case 8: return &k_small_grad_lb_batch<REAL, 8>;
        default: return &k_small_grad_lb_batch<REAL, 16>;
    }
}
template <typename REAL>
BoundGetFn<REAL> bound_get_fn()
{
    return &k_small_bounds_batch<REAL>;
}
template <typename REAL>
BoundCheckFn<REAL> bound_check_fn()
{
    return &k_small_grad_lb_check<REAL>;
}
template <typename REAL>
BoundDistFn<REAL> bound_dist_fn()
{
    return &k_small_distribute_batch<REAL>;
}

}  // namespace bddmma
