// solver_ov.hpp — the solve sweeps' OV instantiations (omega per layer, DevPtrs::omega_lay: learned iterations with omega_vec) for
// SolverT<REAL>: their launches and launch attributes.  Included by solver_ov_f32.hip / solver_ov_f64.hip only, so that these kernels
// compile in translation units of their own, beside the plain ones (solver_f32.hip / solver_f64.hip).
#pragma once
#include "solver_impl.hpp"

namespace bddmma {

template <typename REAL>
int SolverT<REAL>::launch_fwd_ov(const REAL* delta_lay, REAL omega)
{
    return launch_fwd<FWD_SOLVE, true>(delta_lay, omega, BDDMMA_K_FORWARD_MM);
}
template <typename REAL>
int SolverT<REAL>::launch_bwd_ov(const REAL* delta_lay, REAL omega)
{
    return launch_bwd<BWD_SOLVE, true>(delta_lay, omega, BDDMMA_K_BACKWARD_MM);
}

// The dynamic-LDS limits init() gives the plain solve sweeps, for the OV instantiation of each kernel the layout can launch (the OV
// kernels use the same LDS).  The first generation's limit is set whatever its size (init: only above 64 KiB; a limit is not a reservation).
template <typename REAL>
int SolverT<REAL>::ov_prepare()
{
    HIPCHK(hipSetDevice(device));
#define SET_OV(K_, BYTES_) HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&K_), hipFuncAttributeMaxDynamicSharedMemorySize, (int)(BYTES_)))
    if (nb_.n_packs) {
        const uint32_t n1 = stage_lds + seg_bytes(wpb);
#define SET_N(R_, W_)                                                                                                                   \
    SET_OV((k_fwd_narrow<REAL, R_, FWD_SOLVE, W_, true, false, true>), n1); SET_OV((k_bwd_narrow<REAL, R_, BWD_SOLVE, W_, true, false, true>), n1); \
    SET_OV((k_fwd_narrow<REAL, R_, FWD_SOLVE, W_, false, false, true>), n1); SET_OV((k_bwd_narrow<REAL, R_, BWD_SOLVE, W_, false, false, true>), n1)
#define SET_N_W(R_) \
    switch (wpb) { case 1: SET_N(R_, 1); break; case 2: SET_N(R_, 2); break; case 4: SET_N(R_, 4); break; default: SET_N(R_, 8); break; }
        switch (pack_width) {
            case 64: SET_N_W(1) break;
            case 128: SET_N_W(2) break;
            default: SET_N_W(4) break;
        }
#undef SET_N_W
#undef SET_N
        if (pack_width == 128 && wpb == 4) { SET_OV((k_fwd_narrow<REAL, 2, FWD_SOLVE, 4, false, true, true>), n1); SET_OV((k_bwd_narrow<REAL, 2, BWD_SOLVE, 4, false, true, true>), n1); }
        if (pack_width == 128 && wpb == 8) { SET_OV((k_fwd_narrow<REAL, 2, FWD_SOLVE, 8, false, true, true>), n1); SET_OV((k_bwd_narrow<REAL, 2, BWD_SOLVE, 8, false, true, true>), n1); }
    }
    if (use_res2) {
#define SET_RES2(W_) SET_OV((k_fwd_res2<REAL, W_, true>), res2_lds); SET_OV((k_bwd_res2<REAL, W_, true>), res2_lds)
        switch (wpb) { case 1: SET_RES2(1); break; case 2: SET_RES2(2); break; case 4: SET_RES2(4); break; default: SET_RES2(8); break; }
#undef SET_RES2
    } else if (use_res) {
#define SET_RES(R_, W_) SET_OV((k_fwd_res<REAL, R_, W_, true>), res_lds + seg_bytes(wpb)); SET_OV((k_bwd_res<REAL, R_, W_, true>), res_lds + seg_bytes(wpb))
#define SET_RES_W(R_) \
    switch (wpb) { case 1: SET_RES(R_, 1); break; case 2: SET_RES(R_, 2); break; case 4: SET_RES(R_, 4); break; default: SET_RES(R_, 8); break; }
        switch (pack_width) {
            case 64: SET_RES_W(1) break;
            case 128: SET_RES_W(2) break;
            default: SET_RES_W(4) break;
        }
#undef SET_RES_W
#undef SET_RES
    }
    if (use_narrow3) {
#define SET_N3(W_, NT_) SET_OV((k_fwd_narrow3<REAL, W_, NT_, true>), stage_lds); SET_OV((k_bwd_narrow3<REAL, W_, NT_, true>), stage_lds)
        if (wpb == 4) { SET_N3(4, false); } else { SET_N3(8, false); }
        if constexpr (sizeof(REAL) == 8) {
            if (wpb == 4) { SET_N3(4, true); } else { SET_N3(8, true); }
        }
#undef SET_N3
    }
    if (wb_.n_packs) {
#define SET_W(N_) SET_OV((k_fwd_wide2<REAL, FWD_SOLVE, N_, true>), wide_lds); SET_OV((k_bwd_wide2<REAL, BWD_SOLVE, N_, true>), wide_lds)
        if (wide_npt == 1) { SET_W(1); } else if (wide_npt == 2) { SET_W(2); } else { SET_W(4); }
#undef SET_W
    }
#undef SET_OV
    return BDDMMA_OK;
}

}  // namespace bddmma
