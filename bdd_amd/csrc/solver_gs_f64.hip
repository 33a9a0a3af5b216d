// solver_gs_f64.hip — the batch backward kernels of SolverT<double> (solver_gs.hpp, kernels/gradsmall.hpp), as one translation unit.
#include "solver_gs.hpp"

namespace bddmma {
template SolverT<double>::GradSmallFn SolverT<double>::gs_batch_fn(int, bool);
template SolverT<double>::GradSmallLoadFn SolverT<double>::gs_load_fn();
template SolverT<double>::GradSmallUntrackedFn SolverT<double>::gs_untracked_fn(int, bool);
template SolverT<double>::GradSmallCountsFn SolverT<double>::gs_counts_fn(int, bool);
}  // namespace bddmma
