// solver_ss_f64.hip — the learned one-workgroup kernels that stop on the bound's slope of SolverT<double> (solver_ss.hpp,
// kernels/smallstop.hpp), as one translation unit.
#include "solver_ss.hpp"

namespace bddmma {
template SolverT<double>::SmallStopFn SolverT<double>::ss_batch_fn(int, bool, bool);
}  // namespace bddmma
