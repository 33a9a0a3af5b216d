// solver_gs_f32.hip — the batch backward kernels of SolverT<float> (solver_gs.hpp, kernels/gradsmall.hpp), as one translation unit.
#include "solver_gs.hpp"

namespace bddmma {
template SolverT<float>::GradSmallFn SolverT<float>::gs_batch_fn(int, bool);
template SolverT<float>::GradSmallLoadFn SolverT<float>::gs_load_fn();
template SolverT<float>::GradSmallUntrackedFn SolverT<float>::gs_untracked_fn(int, bool);
template SolverT<float>::GradSmallCountsFn SolverT<float>::gs_counts_fn(int, bool);
}  // namespace bddmma
