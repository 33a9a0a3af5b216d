// solver_ss.hpp — the learned one-workgroup kernels that stop on the bound's slope (kernels/smallstop.hpp: k_learned_small_stop_batch,
// k_learned_small_hist_stop_batch) for SolverT<REAL>.  Included by solver_ss_f32.hip / solver_ss_f64.hip only, so that these kernels — the only
// STOP instantiations of small_iterate — compile in translation units of their own, beside the learned ones (solver_sl_*, solver_sh_*).
#pragma once
#include "solver_impl.hpp"
#include "kernels/smallhist.hpp"
#include "kernels/smallstop.hpp"

namespace bddmma {

// The instantiation for members of `nw` waves, without or with the history step (BatchT::learned_iterations_stop, solver_bt.hpp).
template <typename REAL>
typename SolverT<REAL>::SmallStopFn SolverT<REAL>::ss_batch_fn(int nw, bool rl, bool hist)
{
    return pick<1, 2, 4, 8, 16>((uint32_t)nw, [&](auto NW) -> SmallStopFn {
        if (hist) {
            if (rl) return &k_learned_small_hist_stop_batch<REAL, NW.value, true>;
            if constexpr (small_stop_built<REAL>(NW.value, false)) return &k_learned_small_hist_stop_batch<REAL, NW.value, false>;
            else return nullptr;   // not admitted: SolverT::small_stop_ok
        }
        return rl ? &k_learned_small_stop_batch<REAL, NW.value, true> : &k_learned_small_stop_batch<REAL, NW.value, false>;
    });
}

}  // namespace bddmma
