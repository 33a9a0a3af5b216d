// solver_bl_f64.hip — the batch's bound kernel in double (solver_bl.hpp, kernels/batchlb.hpp), as one translation unit.
#include "solver_bl.hpp"

namespace bddmma {
template BoundSumFn<double> bound_sum_fn<double>(int);
}  // namespace bddmma
