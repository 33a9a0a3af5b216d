// solver_ov_f32.hip — the OV instantiations of SolverT<float>'s solve sweeps (solver_ov.hpp), as one translation unit.
#include "solver_ov.hpp"

namespace bddmma {
template int SolverT<float>::ov_prepare();
}  // namespace bddmma
