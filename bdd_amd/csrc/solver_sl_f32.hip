// solver_sl_f32.hip — the learned one-workgroup kernels of SolverT<float> (solver_sl.hpp, kernels/small.hpp), as one translation unit.
#include "solver_sl.hpp"

namespace bddmma {
template int SolverT<float>::sl_prepare();
template SolverT<float>::SmallLnBatchFn SolverT<float>::sl_batch_fn(int, bool);
}  // namespace bddmma
