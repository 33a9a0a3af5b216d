// solver_bc_f64.hip — the batch's cost kernels in double (solver_bc.hpp, kernels/batchcosts.hpp), as one translation unit.
#include "solver_bc.hpp"

namespace bddmma {
template CostsSetFn<double> costs_set_fn<double>(int);
template CostsGetFn<double> costs_get_fn<double>();
}  // namespace bddmma
