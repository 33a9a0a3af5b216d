// solver_gs.hpp — the batch form of the backward of the learned iterations (kernels/gradsmall.hpp: k_grad_small_batch, k_grad_small_load,
// k_grad_small_untracked_batch, k_grad_small_counts_batch)
// for SolverT<REAL>.  Included by solver_gs_f32.hip / solver_gs_f64.hip only, so that these kernels compile in translation units of their
// own, beside the per-handle reverse sweeps (solver_gi_*.hip) and the learned one-workgroup kernels (solver_sl_*.hip).
#pragma once
#include "solver_impl.hpp"
#include "kernels/gradsmall.hpp"

namespace bddmma {

// The instantiation for members of `nw` waves whose learned form keeps its records in LDS (`rl`) or not (BatchT::grad_learned_iterations).
template <typename REAL>
typename SolverT<REAL>::GradSmallFn SolverT<REAL>::gs_batch_fn(int nw, bool rl)
{
    return pick<1, 2, 4, 8, 16>((uint32_t)nw, [&](auto NW) -> GradSmallFn {
        return rl ? &k_grad_small_batch<REAL, NW.value, true> : &k_grad_small_batch<REAL, NW.value, false>;
    });
}
// ... and of the two kernels of the call with per-member counts (BatchT::grad_learned_iterations_counts)
template <typename REAL>
typename SolverT<REAL>::GradSmallUntrackedFn SolverT<REAL>::gs_untracked_fn(int nw, bool rl)
{
    return pick<1, 2, 4, 8, 16>((uint32_t)nw, [&](auto NW) -> GradSmallUntrackedFn {
        return rl ? &k_grad_small_untracked_batch<REAL, NW.value, true> : &k_grad_small_untracked_batch<REAL, NW.value, false>;
    });
}
template <typename REAL>
typename SolverT<REAL>::GradSmallCountsFn SolverT<REAL>::gs_counts_fn(int nw, bool rl)
{
    return pick<1, 2, 4, 8, 16>((uint32_t)nw, [&](auto NW) -> GradSmallCountsFn {
        return rl ? &k_grad_small_counts_batch<REAL, NW.value, true> : &k_grad_small_counts_batch<REAL, NW.value, false>;
    });
}
template <typename REAL>
typename SolverT<REAL>::GradSmallLoadFn SolverT<REAL>::gs_load_fn()
{
    return &k_grad_small_load<REAL>;
}

}  // namespace bddmma
