// solver_br.hpp — a batch's round of primal rounding (kernels/batchround.hpp: k_small_round_batch).  Included by solver_br_f32.hip /
// solver_br_f64.hip only, so that this kernel compiles in translation units of its own, beside the batch's other kernels
// (solver_bt_*.hip, solver_bm_*.hip, ...).
#pragma once
#include "kernels.hpp"
#include "kernels/batchround.hpp"

namespace bddmma {

// The kernel for members of `nw` waves (BatchT::rounding_round groups its members by it).
template <typename REAL>
RoundFn<REAL> round_fn(int nw)
{
    switch (nw) {
        case 1: return &k_small_round_batch<REAL, 1>;
        case 2: return &k_small_round_batch<REAL, 2>;
        case 4: return &k_small_round_batch<REAL, 4>;
        case 8: return &k_small_round_batch<REAL, 8>;
        default: return &k_small_round_batch<REAL, 16>;
    }
}

}  // namespace bddmma
