// solver_gs_f32.hip — the batch backward kernels of SolverT<float> (solver_gs.hpp, kernels/gradsmall.hpp), as one translation unit.
#include "solver_gs.hpp"

namespace bddmma {
template SolverT<float>::GradSmallFn SolverT<float>::gs_batch_fn(int, bool);
template SolverT<float>::GradSmallLoadFn SolverT<float>::gs_load_fn();
}  // namespace bddmma
