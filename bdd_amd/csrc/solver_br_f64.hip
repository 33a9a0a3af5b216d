// solver_br_f64.hip — the batch's rounding round in double (solver_br.hpp, kernels/batchround.hpp), as one translation unit.
#include "solver_br.hpp"

namespace bddmma {
template RoundFn<double> round_fn<double>(int);
}  // namespace bddmma
