// solver_bsm_f32.hip — the batch's sum-marginal kernel in float (solver_bsm.hpp, kernels/batchsm.hpp), as one translation unit.
#include "solver_bsm.hpp"

namespace bddmma {
template SmBatchFn<float> sm_batch_fn<float>(int);
}  // namespace bddmma
