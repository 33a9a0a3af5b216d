// solver_bm.hpp — a batch's min-marginal differences and their gradient (kernels/batchmm.hpp: k_small_mmdiff_batch, k_small_grad_mm_batch,
// k_small_grad_mm_check).  Included by solver_bm_f32.hip / solver_bm_f64.hip only, so that these kernels compile in translation units of
// their own, beside the batch's other kernels (solver_bt_*.hip, solver_bb_*.hip, ...).
#pragma once
#include "kernels.hpp"
#include "kernels/batchmm.hpp"

namespace bddmma {

// The kernels for members of `nw` waves (BatchT::min_marginal_diff / grad_min_marginal_diff group their members by it).
template <typename REAL>
MmDiffFn<REAL> mm_diff_fn(int nw)
{
    switch (nw) {
        case 1: return &k_small_mmdiff_batch<REAL, 1>;
        case 2: return &k_small_mmdiff_batch<REAL, 2>;
        case 4: return &k_small_mmdiff_batch<REAL, 4>;
        case 8: return &k_small_mmdiff_batch<REAL, 8>;
        default: return &k_small_mmdiff_batch<REAL, 16>;
    }
}
template <typename REAL>
MmGradFn<REAL> mm_grad_fn(int nw)
{
    switch (nw) {
        case 1: return &k_small_grad_mm_batch<REAL, 1>;
        case 2: return &k_small_grad_mm_batch<REAL, 2>;
        case 4: return &k_small_grad_mm_batch<REAL, 4>;
        case 8: return &k_small_grad_mm_batch<REAL, 8>;
        default: return &k_small_grad_mm_batch<REAL, 16>;
    }
}
template <typename REAL>
MmCheckFn<REAL> mm_check_fn()
{
    return &k_small_grad_mm_check<REAL>;
}

}  // namespace bddmma
