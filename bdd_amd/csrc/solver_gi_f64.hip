// solver_gi_f64.hip — the backward of the learned iterations of SolverT<double> (solver_gi.hpp, kernels/graditer.hpp), as one translation unit.
#include "solver_gi.hpp"

namespace bddmma {
template int SolverT<double>::gi_prepare(uint64_t);
template int SolverT<double>::gi_grad_learned_iterations(const void*, int, double, const void*, int, void*, void*, void*, void*, void*, uint64_t, uint64_t, uint64_t, int);
template int SolverT<double>::gi_time_kernel(int, uint64_t, double*);
}  // namespace bddmma
