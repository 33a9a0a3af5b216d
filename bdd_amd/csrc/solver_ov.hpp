// solver_ov.hpp — the solve sweeps' OV instantiations (omega per layer, DevPtrs::omega_lay: learned iterations with omega_vec) for
// SolverT<REAL>.  Included by solver_ov_f32.hip / solver_ov_f64.hip only, so that these kernels compile in translation units of their
// own, beside the plain ones (solver_f32.hip / solver_f64.hip).
#pragma once
#include "solver_impl.hpp"

namespace bddmma {

// The solver's rules, resolved for the OV instantiations (resolve_sweep<.., true> is named here alone), and their dynamic-LDS limits by
// the rule of the plain ones (raise_lds_limits).
template <typename REAL>
int SolverT<REAL>::ov_prepare()
{
    HIPCHK(hipSetDevice(device));
    for (int bwd = 0; bwd < 2; ++bwd) {
        ov_sweep[bwd] = resolve_sweep<FWD_SOLVE, true>(bwd);
        if (int rc = raise_lds_limits(ov_sweep[bwd])) return rc;
    }
    return BDDMMA_OK;
}

}  // namespace bddmma
