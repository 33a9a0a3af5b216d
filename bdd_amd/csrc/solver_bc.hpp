// solver_bc.hpp — a batch's set / get of the solver costs (kernels/batchcosts.hpp: k_small_set_batch, k_small_get_batch).  Included by
// solver_bc_f32.hip / solver_bc_f64.hip only, so that these kernels compile in translation units of their own, beside the batch's other
// kernels (solver_bt_*.hip, solver_sl_*.hip, solver_gs_*.hip).
#pragma once
#include "kernels.hpp"
#include "kernels/batchcosts.hpp"

namespace bddmma {

// The set kernel for members of `nw` waves (BatchT::set_solver_costs groups its members by it).
template <typename REAL>
CostsSetFn<REAL> costs_set_fn(int nw)
{
    switch (nw) {
        case 1: return &k_small_set_batch<REAL, 1>;
        case 2: return &k_small_set_batch<REAL, 2>;
        case 4: return &k_small_set_batch<REAL, 4>;
        case 8: return &k_small_set_batch<REAL, 8>;
        default: return &k_small_set_batch<REAL, 16>;
    }
}
template <typename REAL>
CostsGetFn<REAL> costs_get_fn()
{
    return &k_small_get_batch<REAL>;
}

}  // namespace bddmma
