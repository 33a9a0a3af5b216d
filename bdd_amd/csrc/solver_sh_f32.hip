// solver_sh_f32.hip — the learned one-workgroup kernels with their history step of SolverT<float> (solver_sh.hpp, kernels/smallhist.hpp), as
// one translation unit.
#include "solver_sh.hpp"

namespace bddmma {
template SolverT<float>::SmallHistFn SolverT<float>::sh_batch_fn(int, bool);
}  // namespace bddmma
