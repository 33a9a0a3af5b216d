// solver_sl.hpp — the learned form of the one-workgroup kernels (kernels/small.hpp: k_learned_small, k_learned_small_batch) for
// SolverT<REAL>.  Included by solver_sl_f32.hip / solver_sl_f64.hip only, so that these kernels compile in translation units of their
// own, beside the plain ones (solver_f32.hip / solver_f64.hip) and the plain batch kernels (solver_bt_f32.hip / _f64.hip).
#pragma once
#include "solver_impl.hpp"

namespace bddmma {

// This solver's instantiation (its wave count; records in LDS on the learned layout's own budget) and its dynamic-LDS limit.
template <typename REAL>
int SolverT<REAL>::sl_prepare()
{
    HIPCHK(hipSetDevice(device));
    small_ln_kern = {pick<1, 2, 4, 8, 16>(small_nw, [&](auto NW) -> SmallLnFn {
                         return small_ln_rl ? &k_learned_small<REAL, NW.value, true> : &k_learned_small<REAL, NW.value, false>;
                     }),
                     small_ln_lds};
    return raise_lds_limit(small_ln_kern);
}

// The batch form's instantiation for members of `nw` waves (BatchT::learned_iterations, solver_bt.hpp).
template <typename REAL>
typename SolverT<REAL>::SmallLnBatchFn SolverT<REAL>::sl_batch_fn(int nw, bool rl)
{
    return pick<1, 2, 4, 8, 16>((uint32_t)nw, [&](auto NW) -> SmallLnBatchFn {
        return rl ? &k_learned_small_batch<REAL, NW.value, true> : &k_learned_small_batch<REAL, NW.value, false>;
    });
}

}  // namespace bddmma
