// solver_sm_f32.hip — sum-marginals and the smooth solution of SolverT<float> (solver_sm.hpp, kernels/summarg.hpp), as one translation unit.
#include "solver_sm.hpp"

namespace bddmma {
template int SolverT<float>::sm_prepare();
template int SolverT<float>::sm_launch_fwd();
template int SolverT<float>::sm_launch_bwd();
template int SolverT<float>::sm_sum_marginals(int, int, int32_t*, void*, void*, int);
template int SolverT<float>::sm_smooth_solution(void*, int);
}  // namespace bddmma
