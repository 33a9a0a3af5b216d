// solver_bm_f64.hip — the batch's min-marginal kernels in double (solver_bm.hpp, kernels/batchmm.hpp), as one translation unit.
#include "solver_bm.hpp"

namespace bddmma {
template MmDiffFn<double> mm_diff_fn<double>(int);
template MmGradFn<double> mm_grad_fn<double>(int);
template MmCheckFn<double> mm_check_fn<double>();
}  // namespace bddmma
