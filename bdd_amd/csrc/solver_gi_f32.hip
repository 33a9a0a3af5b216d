// solver_gi_f32.hip — the backward of the learned iterations of SolverT<float> (solver_gi.hpp, kernels/graditer.hpp), as one translation unit.
#include "solver_gi.hpp"

namespace bddmma {
template int SolverT<float>::gi_prepare(uint64_t);
template int SolverT<float>::gi_grad_learned_iterations(const void*, int, double, const void*, int, void*, void*, void*, void*, void*, uint64_t, uint64_t, uint64_t, int);
template int SolverT<float>::gi_time_kernel(int, uint64_t, double*);
}  // namespace bddmma
