// solver_br_f32.hip — the batch's rounding round in float (solver_br.hpp, kernels/batchround.hpp), as one translation unit.
#include "solver_br.hpp"

namespace bddmma {
template RoundFn<float> round_fn<float>(int);
}  // namespace bddmma
