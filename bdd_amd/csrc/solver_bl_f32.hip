// solver_bl_f32.hip — the batch's bound kernel in float (solver_bl.hpp, kernels/batchlb.hpp), as one translation unit.
#include "solver_bl.hpp"

namespace bddmma {
template BoundSumFn<float> bound_sum_fn<float>(int);
}  // namespace bddmma
