// solver_sh_f64.hip — the learned one-workgroup kernels with their history step of SolverT<double> (solver_sh.hpp, kernels/smallhist.hpp), as
// one translation unit.
#include "solver_sh.hpp"

namespace bddmma {
template SolverT<double>::SmallHistFn SolverT<double>::sh_batch_fn(int, bool);
}  // namespace bddmma
