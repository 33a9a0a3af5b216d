// solver_sh.hpp — the learned one-workgroup kernels with their history step (kernels/smallhist.hpp: k_learned_small_hist_batch) for
// SolverT<REAL>.  Included by solver_sh_f32.hip / solver_sh_f64.hip only, so that these kernels compile in translation units of their own,
// beside the learned ones without a history (solver_sl_f32.hip / _f64.hip).
#pragma once
#include "solver_impl.hpp"
#include "kernels/smallhist.hpp"

namespace bddmma {

// The instantiation for members of `nw` waves (BatchT::learned_iterations_history, solver_bt.hpp).
template <typename REAL>
typename SolverT<REAL>::SmallHistFn SolverT<REAL>::sh_batch_fn(int nw, bool rl)
{
    return pick<1, 2, 4, 8, 16>((uint32_t)nw, [&](auto NW) -> SmallHistFn {
        return rl ? &k_learned_small_hist_batch<REAL, NW.value, true> : &k_learned_small_hist_batch<REAL, NW.value, false>;
    });
}

}  // namespace bddmma
