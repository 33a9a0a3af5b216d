// solver_bp_f32.hip — the batch's solution, cost-update and perturbation-gradient kernels in float (solver_bp.hpp, kernels/batchsol.hpp), as one translation unit.
#include "solver_bp.hpp"

namespace bddmma {
template SolutionFn<float> solution_fn<float>(int);
template PerturbUpdateFn<float, float> perturb_update_fn<float, float>();
template PerturbUpdateFn<float, double> perturb_update_fn<float, double>();
template PerturbGradFn<float> perturb_grad_fn<float>();
template PerturbCheckFn<float> perturb_check_fn<float>();
}  // namespace bddmma
