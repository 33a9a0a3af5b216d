// solver_bl.hpp — a batch's lower bounds in one launch (kernels/batchlb.hpp: k_small_bound_batch).  Included by solver_bl_f32.hip /
// solver_bl_f64.hip only, so that the kernel compiles in translation units of its own, beside the batch's other kernels (solver_bt_*.hip,
// solver_bc_*.hip).
#pragma once
#include "kernels.hpp"
#include "kernels/batchlb.hpp"

namespace bddmma {

// The kernel for members of `nw` waves (BatchT::lower_bounds groups its members by it, as set_solver_costs does).
template <typename REAL>
BoundSumFn<REAL> bound_sum_fn(int nw)
{
    switch (nw) {
        case 1: return &k_small_bound_batch<REAL, 1>;
        case 2: return &k_small_bound_batch<REAL, 2>;
        case 4: return &k_small_bound_batch<REAL, 4>;
        case 8: return &k_small_bound_batch<REAL, 8>;
        default: return &k_small_bound_batch<REAL, 16>;
    }
}

}  // namespace bddmma
