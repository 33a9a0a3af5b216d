// solver_bb_f32.hip — the batch's bound kernels in float (solver_bb.hpp, kernels/batchbound.hpp), as one translation unit.
#include "solver_bb.hpp"

namespace bddmma {
template BoundGradFn<float> bound_grad_fn<float>(int);
template BoundGetFn<float> bound_get_fn<float>();
template BoundCheckFn<float> bound_check_fn<float>();
template BoundDistFn<float> bound_dist_fn<float>();
}  // namespace bddmma
