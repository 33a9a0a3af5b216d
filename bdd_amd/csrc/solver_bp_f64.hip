// solver_bp_f64.hip — the batch's solution, cost-update and perturbation-gradient kernels in double (solver_bp.hpp, kernels/batchsol.hpp), as one translation unit.
#include "solver_bp.hpp"

namespace bddmma {
template SolutionFn<double> solution_fn<double>(int);
template PerturbUpdateFn<double, float> perturb_update_fn<double, float>();
template PerturbUpdateFn<double, double> perturb_update_fn<double, double>();
template PerturbGradFn<double> perturb_grad_fn<double>();
template PerturbCheckFn<double> perturb_check_fn<double>();
}  // namespace bddmma
