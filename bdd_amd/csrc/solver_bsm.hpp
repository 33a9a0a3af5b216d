// solver_bsm.hpp — a batch's sum-marginals, smooth solutions and smooth bound gradient (kernels/batchsm.hpp: k_small_summarg_batch).
// Included by solver_bsm_f32.hip / solver_bsm_f64.hip only, so that this kernel compiles in translation units of its own, beside the
// batch's other kernels (solver_bt_*.hip, solver_bb_*.hip, solver_bm_*.hip, ...).
#pragma once
#include "kernels.hpp"
#include "kernels/batchsm.hpp"

namespace bddmma {

// The kernel for members of `nw` waves (BatchT::bsm_run groups its members by it).
template <typename REAL>
SmBatchFn<REAL> sm_batch_fn(int nw)
{
    switch (nw) {
        case 1: return &k_small_summarg_batch<REAL, 1>;
        case 2: return &k_small_summarg_batch<REAL, 2>;
        case 4: return &k_small_summarg_batch<REAL, 4>;
        case 8: return &k_small_summarg_batch<REAL, 8>;
        default: return &k_small_summarg_batch<REAL, 16>;
    }
}

}  // namespace bddmma
