// solver_bc_f32.hip — the batch's cost kernels in float (solver_bc.hpp, kernels/batchcosts.hpp), as one translation unit.
#include "solver_bc.hpp"

namespace bddmma {
template CostsSetFn<float> costs_set_fn<float>(int);
template CostsGetFn<float> costs_get_fn<float>();
}  // namespace bddmma
