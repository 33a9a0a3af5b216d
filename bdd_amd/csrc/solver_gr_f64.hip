// solver_gr_f64.hip — the backward operators of SolverT<double> (solver_gr.hpp, kernels/gradmm.hpp), as one translation unit.
#include "solver_gr.hpp"

namespace bddmma {
template int SolverT<double>::gr_prepare();
template int SolverT<double>::gr_launch_down();
template int SolverT<double>::gr_launch_up();
template int SolverT<double>::gr_load(double*, const void*, uint64_t, int, const char*);
template int SolverT<double>::gr_load_device(const SolverT<double>::LoadSpec*, int, uint64_t, const char*);
template int SolverT<double>::gr_min_marginal_diff(const void*, void*, void*, int);
template int SolverT<double>::gr_lower_bound_per_bdd(const void*, void*, void*, int, int);
template int SolverT<double>::gr_distribute_delta(const void*, const void*, void*, int);
template int SolverT<double>::gr_cost_perturbation(const void*, const void*, void*, void*, int);
}  // namespace bddmma
