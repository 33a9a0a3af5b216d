// solver_sl_f64.hip — the learned one-workgroup kernels of SolverT<double> (solver_sl.hpp, kernels/small.hpp), as one translation unit.
#include "solver_sl.hpp"

namespace bddmma {
template int SolverT<double>::sl_prepare();
template SolverT<double>::SmallLnBatchFn SolverT<double>::sl_batch_fn(int, bool);
}  // namespace bddmma
