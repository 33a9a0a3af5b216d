// solver_ov_f64.hip — the OV instantiations of SolverT<double>'s solve sweeps (solver_ov.hpp), as one translation unit.
#include "solver_ov.hpp"

namespace bddmma {
template int SolverT<double>::ov_prepare();
}  // namespace bddmma
