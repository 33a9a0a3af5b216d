// solver_bsm_f64.hip — the batch's sum-marginal kernel in double (solver_bsm.hpp, kernels/batchsm.hpp), as one translation unit.
#include "solver_bsm.hpp"

namespace bddmma {
template SmBatchFn<double> sm_batch_fn<double>(int);
}  // namespace bddmma
