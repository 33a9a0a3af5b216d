// solver_ss_f32.hip — the learned one-workgroup kernels that stop on the bound's slope of SolverT<float> (solver_ss.hpp,
// kernels/smallstop.hpp), as one translation unit.
#include "solver_ss.hpp"

namespace bddmma {
template SolverT<float>::SmallStopFn SolverT<float>::ss_batch_fn(int, bool, bool);
}  // namespace bddmma
