// solver_bm_f32.hip — the batch's min-marginal kernels in float (solver_bm.hpp, kernels/batchmm.hpp), as one translation unit.
#include "solver_bm.hpp"

namespace bddmma {
template MmDiffFn<float> mm_diff_fn<float>(int);
template MmGradFn<float> mm_grad_fn<float>(int);
template MmCheckFn<float> mm_check_fn<float>();
}  // namespace bddmma
