// solver_sm_f64.hip — sum-marginals and the smooth solution of SolverT<double> (solver_sm.hpp, kernels/summarg.hpp), as one translation unit.
#include "solver_sm.hpp"

namespace bddmma {
template int SolverT<double>::sm_prepare();
template int SolverT<double>::sm_launch_fwd();
template int SolverT<double>::sm_launch_bwd();
template int SolverT<double>::sm_sum_marginals(int, int, int32_t*, void*, void*, int);
template int SolverT<double>::sm_smooth_solution(void*, int);
}  // namespace bddmma
