// solver_gr_f32.hip — the backward operators of SolverT<float> (solver_gr.hpp, kernels/gradmm.hpp), as one translation unit.
#include "solver_gr.hpp"

namespace bddmma {
template int SolverT<float>::gr_prepare();
template int SolverT<float>::gr_launch_down();
template int SolverT<float>::gr_launch_up();
template int SolverT<float>::gr_load(float*, const void*, uint64_t, int, const char*);
template int SolverT<float>::gr_load_device(const SolverT<float>::LoadSpec*, int, uint64_t, const char*);
template int SolverT<float>::gr_min_marginal_diff(const void*, void*, void*, int);
template int SolverT<float>::gr_lower_bound_per_bdd(const void*, void*, void*, int, int);
template int SolverT<float>::gr_distribute_delta(const void*, const void*, void*, int);
template int SolverT<float>::gr_cost_perturbation(const void*, const void*, void*, void*, int);
}  // namespace bddmma
