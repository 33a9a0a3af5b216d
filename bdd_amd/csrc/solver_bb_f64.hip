// solver_bb_f64.hip — the batch's bound kernels in double (solver_bb.hpp, kernels/batchbound.hpp), as one translation unit.
#include "solver_bb.hpp"

namespace bddmma {
template BoundGradFn<double> bound_grad_fn<double>(int);
template BoundGetFn<double> bound_get_fn<double>();
template BoundCheckFn<double> bound_check_fn<double>();
template BoundDistFn<double> bound_dist_fn<double>();
}  // namespace bddmma
