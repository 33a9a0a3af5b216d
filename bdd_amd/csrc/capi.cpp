// capi.cpp — extern "C" entry points of include/bdd_mma.h (everything except the L-BFGS ones,
// which live in lbfgs.hip).  No exception crosses this boundary.
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <new>
#include <string>
#include <vector>

#include "../../include/bdd_mma.h"
#include "layout.hpp"
#include "solver.hpp"

using namespace bddmma;

struct bddmma_lbfgs;
extern "C" int bddmma_lbfgs_iteration(bddmma_lbfgs* l);
extern "C" int bddmma_lbfgs_update_costs(bddmma_lbfgs* l, const void* lo, uint64_t n_lo, const void* hi, uint64_t n_hi, int elem_precision,
                                         int on_device);

namespace {
thread_local std::string g_err;

template <typename F>
int guarded(bddmma_solver* s, F&& f)
{
    if (!s || !s->impl) return BDDMMA_ERR_INVALID_ARGUMENT;
    try {
        return f(s->impl);
    } catch (const std::bad_alloc&) {
        s->impl->err = "out of host memory";
        return BDDMMA_ERR_DEVICE;
    } catch (const std::exception& e) {
        s->impl->err = e.what();
        return BDDMMA_ERR_DEVICE;
    }
}
template <typename F>
int guarded(const bddmma_solver* s, F&& f) { return guarded(const_cast<bddmma_solver*>(s), f); }

template <typename F>
int guarded_batch(bddmma_batch* b, F&& f)
{
    if (!b || !b->impl) return BDDMMA_ERR_INVALID_ARGUMENT;
    try {
        return f(b->impl);
    } catch (const std::exception& e) {
        b->impl->err = e.what();
        return BDDMMA_ERR_DEVICE;
    }
}

template <typename T>
int copy_host(const std::vector<T>& v, T* out)
{
    if (!out) return BDDMMA_ERR_INVALID_ARGUMENT;
    if (!v.empty()) std::memcpy(out, v.data(), v.size() * sizeof(T));
    return BDDMMA_OK;
}
}  // namespace

extern "C" {

int bddmma_create(bddmma_solver** out, int precision, int device, const bddmma_instruction* instr,
                  const uint64_t* bdd_delims, uint64_t n_bdds, const double* costs_hi, uint64_t n_costs,
                  const bddmma_options* opts)
{
    if (!out) return BDDMMA_ERR_INVALID_ARGUMENT;
    *out = nullptr;
    try {
#ifdef BDDMMA_EXPERIMENTAL  // make EXPERIMENTAL=1: phase timings of the construction on stderr (tools/construct_time.py)
        static const bool timing = std::getenv("BDDMMA_LAYOUT_TIMING") != nullptr;
#else
        constexpr bool timing = false;
#endif
        auto t_last = std::chrono::steady_clock::now();
        auto lap = [&](const char* what) {
            if (!timing) return;
            const auto now = std::chrono::steady_clock::now();
            std::fprintf(stderr, "[create] %-28s %8.1f ms\n", what, std::chrono::duration<double, std::milli>(now - t_last).count());
            t_last = now;
        };
        HostLayout L;
        ChipInfo chip;
        int rc = query_chip(device, &chip, g_err);
        if (rc) return rc;
        rc = build_layout(instr, bdd_delims, n_bdds, opts, L, g_err, false, precision == BDDMMA_F64 ? 8 : 4, chip);
        if (rc) return rc;
        lap("host layout");
        SolverBase* impl = nullptr;
        rc = create_solver(&impl, precision, device, L, opts, g_err);
        if (rc) return rc;
        lap("device buffers + upload");
        impl->n_packs_narrow = L.narrow.n_packs();
        impl->n_packs_wide = L.wide.n_packs() + L.huge.n_packs();
        if (costs_hi && n_costs) {
            rc = impl->update_costs(nullptr, 0, costs_hi, n_costs, BDDMMA_F64, 0);
            if (rc) {
                g_err = impl->err;
                delete impl;
                return rc;
            }
        }
        lap("update_costs");
        *out = new bddmma_solver{impl};
        return BDDMMA_OK;
    } catch (const std::exception& e) {
        g_err = e.what();
        return BDDMMA_ERR_DEVICE;
    }
}

int bddmma_device_count(void) { return device_count(); }
int bddmma_device_chip(int device, uint32_t* n_cus, uint32_t* lds_bytes_per_cu, uint64_t* max_resident_threads)
{
    if (device < 0 || device >= device_count()) { g_err = "no such HIP device"; return BDDMMA_ERR_DEVICE; }
    ChipInfo chip;
    const int rc = query_chip(device, &chip, g_err);
    if (rc) return rc;
    if (n_cus) *n_cus = chip.n_cus;
    if (lds_bytes_per_cu) *lds_bytes_per_cu = chip.lds_bytes;
    if (max_resident_threads) *max_resident_threads = chip.max_resident_threads;
    return BDDMMA_OK;
}
int bddmma_set_layout_threads(int n)
{
    if (n < 0) return BDDMMA_ERR_INVALID_ARGUMENT;
    set_layout_threads((unsigned)n);
    return BDDMMA_OK;
}
int bddmma_set_thread_layout_threads(int n)
{
    if (n < 0) return BDDMMA_ERR_INVALID_ARGUMENT;
    set_thread_layout_threads((unsigned)n);
    return BDDMMA_OK;
}

void bddmma_destroy(bddmma_solver* s)
{
    if (!s) return;
    delete s->impl;
    delete s;
}

const char* bddmma_last_error(const bddmma_solver* s) { return (s && s->impl) ? s->impl->err.c_str() : g_err.c_str(); }

uint64_t bddmma_nr_variables(const bddmma_solver* s) { return s && s->impl ? s->impl->n_vars : 0; }
uint64_t bddmma_nr_bdds(const bddmma_solver* s) { return s && s->impl ? s->impl->n_bdds : 0; }
uint64_t bddmma_nr_layers(const bddmma_solver* s) { return s && s->impl ? s->impl->n_layers : 0; }
uint64_t bddmma_nr_bdd_nodes(const bddmma_solver* s) { return s && s->impl ? s->impl->n_input_nodes : 0; }
uint64_t bddmma_nr_hops(const bddmma_solver* s) { return s && s->impl ? s->impl->n_hops : 0; }
uint64_t bddmma_nr_packs(const bddmma_solver* s) { return s && s->impl ? s->impl->n_packs_narrow + s->impl->n_packs_wide : 0; }
int bddmma_solve_sweep_kind(const bddmma_solver* s) { return s && s->impl ? s->impl->solve_sweep_kind : -1; }
int bddmma_fused_small(const bddmma_solver* s) { return s && s->impl ? (s->impl->fused_small ? 1 : 0) : -1; }
int bddmma_fused_small_learned(const bddmma_solver* s) { return s && s->impl ? (s->impl->fused_small_learned ? 1 : 0) : -1; }
int bddmma_fused_small_history(const bddmma_solver* s) { return s && s->impl ? (s->impl->fused_small_history ? 1 : 0) : -1; }
int bddmma_fused_small_stop(const bddmma_solver* s) { return s && s->impl ? (s->impl->fused_small_stop ? 1 : 0) : -1; }
int bddmma_nontemporal_loads(const bddmma_solver* s) { return s && s->impl ? (s->impl->nt_loads ? 1 : 0) : -1; }
int bddmma_potentials_on_chip(const bddmma_solver* s) { return s && s->impl ? (s->impl->pot_on_chip ? 1 : 0) : -1; }
int bddmma_onchip_hops(const bddmma_solver* s) { return s && s->impl ? s->impl->onchip_hops : -1; }
int bddmma_lane_sweeps(const bddmma_solver* s) { return s && s->impl ? (s->impl->lane_sweeps ? 1 : 0) : -1; }
int bddmma_precision(const bddmma_solver* s) { return s && s->impl ? s->impl->precision : -1; }
int bddmma_device(const bddmma_solver* s) { return s && s->impl ? s->impl->device : -1; }
uint64_t bddmma_device_bytes(const bddmma_solver* s) { return s && s->impl ? s->impl->dev_bytes : 0; }
uint64_t bddmma_device_allocated_bytes(const bddmma_solver* s) { return s && s->impl ? s->impl->dev_alloc_bytes : 0; }

int bddmma_num_bdds_per_var(const bddmma_solver* s, int32_t* out)
{
    return guarded(s, [&](SolverBase* b) { return copy_host(b->h_nbdds, out); });
}
int bddmma_layer_variables(const bddmma_solver* s, int32_t* out)
{
    return guarded(s, [&](SolverBase* b) { return copy_host(b->h_layer_var, out); });
}
int bddmma_layer_bdds(const bddmma_solver* s, int32_t* out)
{
    return guarded(s, [&](SolverBase* b) { return copy_host(b->h_layer_bdd, out); });
}
int bddmma_nodes_per_hop(const bddmma_solver* s, uint64_t* out)
{
    return guarded(s, [&](SolverBase* b) { return copy_host(b->nodes_per_hop, out); });
}
int bddmma_layers_per_hop(const bddmma_solver* s, uint64_t* out)
{
    return guarded(s, [&](SolverBase* b) { return copy_host(b->layers_per_hop, out); });
}

int bddmma_update_costs(bddmma_solver* s, const void* lo, uint64_t n_lo, const void* hi, uint64_t n_hi,
                        int elem_precision, int on_device)
{
    return guarded(s, [&](SolverBase* b) {
        if (elem_precision != BDDMMA_F32 && elem_precision != BDDMMA_F64) {
            b->err = "elem_precision must be BDDMMA_F32 or BDDMMA_F64";
            return BDDMMA_ERR_INVALID_ARGUMENT;
        }
        return b->update_costs(lo, n_lo, hi, n_hi, elem_precision, on_device);
    });
}
int bddmma_set_cost(bddmma_solver* s, double c, uint64_t var)
{
    return guarded(s, [&](SolverBase* b) { return b->set_cost(c, var); });
}
int bddmma_get_solver_costs(const bddmma_solver* s, void* lo, void* hi, void* mm, int on_device)
{
    return guarded(s, [&](SolverBase* b) { return b->get_solver_costs(lo, hi, mm, on_device); });
}
int bddmma_set_solver_costs(bddmma_solver* s, const void* lo, const void* hi, const void* mm, int on_device)
{
    return guarded(s, [&](SolverBase* b) { return b->set_solver_costs(lo, hi, mm, on_device); });
}
int bddmma_primal_objective_vec(bddmma_solver* s, void* out, int on_device)
{
    return guarded(s, [&](SolverBase* b) { return b->primal_objective_vec(out, on_device); });
}
int bddmma_forward_run(bddmma_solver* s) { return guarded(s, [&](SolverBase* b) { return b->forward_run(); }); }
int bddmma_backward_run(bddmma_solver* s) { return guarded(s, [&](SolverBase* b) { return b->backward_run(); }); }
int bddmma_lower_bound(bddmma_solver* s, double* lb)
{
    return guarded(s, [&](SolverBase* b) { return lb ? b->lower_bound(lb) : BDDMMA_ERR_INVALID_ARGUMENT; });
}
int bddmma_lower_bound_per_bdd(bddmma_solver* s, void* out, int on_device)
{
    return guarded(s, [&](SolverBase* b) { return b->lower_bound_per_bdd(out, on_device); });
}
int bddmma_iteration(bddmma_solver* s, double omega)
{
    return guarded(s, [&](SolverBase* b) { return b->iteration(omega); });
}
int bddmma_iterations(bddmma_solver* s, double omega, uint64_t n)
{
    return guarded(s, [&](SolverBase* b) { return b->iterations(omega, n); });
}
int bddmma_learned_iterations(bddmma_solver* s, const void* dist_weights, int weights_on_device, uint64_t num_itr, double omega,
                              double improvement_slope, void* sol_avg, void* lb_first_diff_avg, void* lb_second_diff_avg,
                              uint64_t compute_history_for_itr, double history_avg_beta, int outputs_on_device, uint64_t* itr_done)
{
    return guarded(s, [&](SolverBase* b) {
        return b->learned_iterations(dist_weights, weights_on_device, num_itr, omega, improvement_slope, sol_avg, lb_first_diff_avg,
                                     lb_second_diff_avg, compute_history_for_itr, history_avg_beta, outputs_on_device, itr_done, nullptr, 0);
    });
}
int bddmma_learned_iterations_omega_vec(bddmma_solver* s, const void* dist_weights, int weights_on_device, uint64_t num_itr, const void* omega_vec,
                                        int omega_vec_on_device, double improvement_slope, void* sol_avg, void* lb_first_diff_avg,
                                        void* lb_second_diff_avg, uint64_t compute_history_for_itr, double history_avg_beta, int outputs_on_device,
                                        uint64_t* itr_done)
{
    return guarded(s, [&](SolverBase* b) {
        if (!omega_vec) {
            if (itr_done) *itr_done = 0;
            b->err = "learned_iterations: omega_vec is null";
            return BDDMMA_ERR_INVALID_ARGUMENT;
        }
        return b->learned_iterations(dist_weights, weights_on_device, num_itr, 0.0, improvement_slope, sol_avg, lb_first_diff_avg,
                                     lb_second_diff_avg, compute_history_for_itr, history_avg_beta, outputs_on_device, itr_done, omega_vec,
                                     omega_vec_on_device);
    });
}
int bddmma_isotropic_dist_weights(bddmma_solver* s, void* out, int on_device)
{
    return guarded(s, [&](SolverBase* b) { return out ? b->isotropic_dist_weights(out, on_device) : BDDMMA_ERR_INVALID_ARGUMENT; });
}
int bddmma_forward_mm(bddmma_solver* s, double omega, void* d, int on_device)
{
    return guarded(s, [&](SolverBase* b) { return d ? b->forward_mm(omega, d, on_device) : BDDMMA_ERR_INVALID_ARGUMENT; });
}
int bddmma_backward_mm(bddmma_solver* s, double omega, void* d, int on_device)
{
    return guarded(s, [&](SolverBase* b) { return d ? b->backward_mm(omega, d, on_device) : BDDMMA_ERR_INVALID_ARGUMENT; });
}
int bddmma_normalize_delta(const bddmma_solver* s, void* d, int on_device)
{
    return guarded(s, [&](SolverBase* b) { return d ? b->normalize_delta(d, on_device) : BDDMMA_ERR_INVALID_ARGUMENT; });
}
int bddmma_distribute_delta(bddmma_solver* s) { return guarded(s, [&](SolverBase* b) { return b->distribute_delta(); }); }
int bddmma_get_delta(const bddmma_solver* s, void* out, int on_device)
{
    return guarded(s, [&](SolverBase* b) { return out ? b->get_delta(out, on_device) : BDDMMA_ERR_INVALID_ARGUMENT; });
}
int bddmma_set_delta(bddmma_solver* s, const void* in, int on_device)
{
    return guarded(s, [&](SolverBase* b) { return in ? b->set_delta(in, on_device) : BDDMMA_ERR_INVALID_ARGUMENT; });
}
int bddmma_min_marginals(bddmma_solver* s, int sorted, int32_t* var, void* mm0, void* mm1, int on_device)
{
    return guarded(s, [&](SolverBase* b) { return b->min_marginals(sorted, var, mm0, mm1, on_device); });
}
int bddmma_min_marginal_diff(bddmma_solver* s, void* out, int on_device)
{
    return guarded(s, [&](SolverBase* b) { return out ? b->min_marginal_diff(out, on_device) : BDDMMA_ERR_INVALID_ARGUMENT; });
}
int bddmma_sum_marginals(bddmma_solver* s, int sorted, int log_probs, int32_t* var, void* sm0, void* sm1, int on_device)
{
    return guarded(s, [&](SolverBase* b) { return (sm0 && sm1) ? b->sum_marginals(sorted, log_probs, var, sm0, sm1, on_device) : BDDMMA_ERR_INVALID_ARGUMENT; });
}
int bddmma_smooth_solution(bddmma_solver* s, void* out, int on_device)
{
    return guarded(s, [&](SolverBase* b) { return out ? b->smooth_solution(out, on_device) : BDDMMA_ERR_INVALID_ARGUMENT; });
}
int bddmma_grad_min_marginal_diff(bddmma_solver* s, const void* grad_mm, void* grad_lo_out, void* grad_hi_out, int on_device)
{
    return guarded(s, [&](SolverBase* b) {
        return (grad_mm && grad_lo_out && grad_hi_out) ? b->grad_min_marginal_diff(grad_mm, grad_lo_out, grad_hi_out, on_device) : BDDMMA_ERR_INVALID_ARGUMENT;
    });
}
int bddmma_grad_lower_bound_per_bdd(bddmma_solver* s, const void* grad_lb_per_bdd, void* grad_lo_out, void* grad_hi_out, int smooth, int on_device)
{
    return guarded(s, [&](SolverBase* b) {
        return (grad_lb_per_bdd && grad_lo_out && grad_hi_out) ? b->grad_lower_bound_per_bdd(grad_lb_per_bdd, grad_lo_out, grad_hi_out, smooth, on_device)
                                                               : BDDMMA_ERR_INVALID_ARGUMENT;
    });
}
int bddmma_grad_distribute_delta(bddmma_solver* s, const void* grad_lo, const void* grad_hi, void* grad_deferred_mm_out, int on_device)
{
    return guarded(s, [&](SolverBase* b) {
        return (grad_lo && grad_hi && grad_deferred_mm_out) ? b->grad_distribute_delta(grad_lo, grad_hi, grad_deferred_mm_out, on_device) : BDDMMA_ERR_INVALID_ARGUMENT;
    });
}
int bddmma_grad_learned_iterations(bddmma_solver* s, const void* dist_weights, int weights_on_device, double omega, const void* omega_vec,
                                   int omega_vec_on_device, void* grad_lo, void* grad_hi, void* grad_mm, void* grad_dist_weights_out, void* grad_omega_out,
                                   uint64_t track_grad_after_itr, uint64_t track_grad_for_num_itr, uint64_t num_caches, int on_device)
{
    return guarded(s, [&](SolverBase* b) {
        return b->grad_learned_iterations(dist_weights, weights_on_device, omega, omega_vec, omega_vec_on_device, grad_lo, grad_hi, grad_mm,
                                          grad_dist_weights_out, grad_omega_out, track_grad_after_itr, track_grad_for_num_itr, num_caches, on_device);
    });
}
int bddmma_grad_cost_perturbation(bddmma_solver* s, const void* grad_lo, const void* grad_hi, void* grad_lo_pert_out, void* grad_hi_pert_out, int on_device)
{
    return guarded(s, [&](SolverBase* b) {
        return (grad_lo && grad_hi && grad_lo_pert_out && grad_hi_pert_out) ? b->grad_cost_perturbation(grad_lo, grad_hi, grad_lo_pert_out, grad_hi_pert_out, on_device)
                                                                            : BDDMMA_ERR_INVALID_ARGUMENT;
    });
}
int bddmma_bdds_solution(bddmma_solver* s, int sorted, char* sol, int on_device)
{
    return guarded(s, [&](SolverBase* b) { return sol ? b->bdds_solution(sorted, sol, on_device) : BDDMMA_ERR_INVALID_ARGUMENT; });
}
int bddmma_net_solver_costs(const bddmma_solver* s, void* out, int on_device)
{
    return guarded(s, [&](SolverBase* b) { return out ? b->net_solver_costs(out, on_device) : BDDMMA_ERR_INVALID_ARGUMENT; });
}
int bddmma_make_dual_feasible(const bddmma_solver* s, void* g, int on_device)
{
    return guarded(s, [&](SolverBase* b) { return g ? b->make_dual_feasible(g, on_device) : BDDMMA_ERR_INVALID_ARGUMENT; });
}
int bddmma_gradient_step(bddmma_solver* s, const void* g, double step, int on_device)
{
    return guarded(s, [&](SolverBase* b) { return g ? b->gradient_step(g, step, on_device) : BDDMMA_ERR_INVALID_ARGUMENT; });
}

// run_solver, include/run_solver_util.h:10-77.  host_loop: the reference's literal loop (iteration, lower_bound, tests on the host) for the
// plain solver too — bddmma_run_solver_host_loop, the twin the device-resident loop is tested against.
static int run_solver_impl(bddmma_solver* s, bddmma_lbfgs* lbfgs, uint64_t max_iter, double tolerance, double improvement_slope, double time_limit,
                           int verbose, bddmma_run_result* res, bool host_loop)
{
    return guarded(s, [&](SolverBase* b) {
        if (improvement_slope < 0.0 || improvement_slope >= 1.0 || time_limit < 0.0 || tolerance < 0.0) {
            b->err = "run_solver: invalid termination criteria";  // asserts at run_solver_util.h:13-15
            return BDDMMA_ERR_INVALID_ARGUMENT;
        }
        // plain MMA: the loop runs with its termination tests on the device (no host round trip per iteration); the L-BFGS wrapper
        // decides its steps on the host anyway and keeps the sequential loop below
        if (!lbfgs && !host_loop) return b->run_plain(max_iter, tolerance, improvement_slope, time_limit, verbose, res);
        const auto t0 = std::chrono::steady_clock::now();
        auto elapsed = [&]() { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); };
        double lb_initial;
        int rc = b->lower_bound(&lb_initial);
        if (rc) return rc;
        double lb_first = std::numeric_limits<double>::max(), lb_prev = lb_initial, lb_post = lb_initial;
        if (verbose) std::printf("[bdd solver] initial lower bound = %.10g, time = %.3f s\n", lb_prev, elapsed());
        uint64_t iter = 0;
        int reason = 0;
        for (; iter < max_iter; ++iter) {
            rc = lbfgs ? bddmma_lbfgs_iteration(lbfgs) : b->iteration(0.5);
            if (rc) return rc;
            lb_prev = lb_post;
            if ((rc = b->lower_bound(&lb_post))) return rc;
            if (iter == 0) lb_first = lb_post;
            const double t = elapsed();
            if (verbose) std::printf("[bdd solver] iteration %llu, lower bound = %.10g, time = %.3f s\n", (unsigned long long)iter, lb_post, t);
            if (t > time_limit) { reason = 1; ++iter; break; }
            if (std::abs(lb_prev - lb_post) < std::abs(tolerance * lb_prev)) { reason = 2; ++iter; break; }
            if (std::abs(lb_prev - lb_post) < improvement_slope * std::abs(lb_initial - lb_first)) { reason = 3; ++iter; break; }
            if (lb_post == std::numeric_limits<double>::infinity()) { reason = 4; ++iter; break; }
        }
        if (verbose) std::printf("[bdd solver] final lower bound = %.10g\n", lb_post);
        if (res) {
            res->iterations = iter;
            res->lb_initial = lb_initial;
            res->lb_final = lb_post;
            res->seconds = elapsed();
            res->stop_reason = reason;
        }
        return BDDMMA_OK;
    });
}
int bddmma_run_solver(bddmma_solver* s, bddmma_lbfgs* lbfgs, uint64_t max_iter, double tolerance, double improvement_slope, double time_limit,
                      int verbose, bddmma_run_result* res)
{
    return run_solver_impl(s, lbfgs, max_iter, tolerance, improvement_slope, time_limit, verbose, res, false);
}
int bddmma_run_solver_host_loop(bddmma_solver* s, bddmma_lbfgs* lbfgs, uint64_t max_iter, double tolerance, double improvement_slope,
                                double time_limit, int verbose, bddmma_run_result* res)
{
    return run_solver_impl(s, lbfgs, max_iter, tolerance, improvement_slope, time_limit, verbose, res, true);
}

// ---- batches of one-workgroup instances (solver.hpp: BatchBase)
int bddmma_batch_create(bddmma_batch** out, bddmma_solver* const* members, uint64_t n)
{
    if (out) *out = nullptr;
    if (!out || !members || n == 0) {
        g_err = !out ? "batch: null output pointer" : !members ? "batch: null member array" : "batch: no members";
        return BDDMMA_ERR_INVALID_ARGUMENT;
    }
    try {
        std::vector<SolverBase*> impls(n);
        for (uint64_t i = 0; i < n; ++i) {
            if (!members[i] || !members[i]->impl) {
                g_err = "batch member " + std::to_string(i) + ": null handle";
                return BDDMMA_ERR_INVALID_ARGUMENT;
            }
            impls[i] = members[i]->impl;
        }
        BatchBase* impl = nullptr;
        const int rc = create_batch(&impl, impls.data(), n, g_err);
        if (rc) return rc;
        *out = new bddmma_batch{impl};
        return BDDMMA_OK;
    } catch (const std::exception& e) {
        g_err = e.what();
        return BDDMMA_ERR_DEVICE;
    }
}
void bddmma_batch_destroy(bddmma_batch* b)
{
    if (!b) return;
    delete b->impl;
    delete b;
}
const char* bddmma_batch_last_error(const bddmma_batch* b) { return (b && b->impl) ? b->impl->err.c_str() : g_err.c_str(); }
uint64_t bddmma_batch_size(const bddmma_batch* b) { return b && b->impl ? b->impl->size() : 0; }
int bddmma_batch_iterations(bddmma_batch* b, double omega, uint64_t n)
{
    return guarded_batch(b, [&](BatchBase* i) { return i->iterations(omega, n); });
}
int bddmma_learned_iterations_batch(bddmma_batch* b, const void* dist_weights, const void* omega_vec, double omega, uint64_t num_itr, int on_device)
{
    return guarded_batch(b, [&](BatchBase* i) { return i->learned_iterations(dist_weights, omega_vec, omega, num_itr, on_device); });
}
int bddmma_learned_iterations_history_batch(bddmma_batch* b, const void* dist_weights, const void* omega_vec, double omega, uint64_t num_itr, void* sol_avg,
                                            void* lb_first_diff_avg, void* lb_second_diff_avg, uint64_t compute_history_for_itr, double history_avg_beta,
                                            int on_device)
{
    return guarded_batch(b, [&](BatchBase* i) {
        return i->learned_iterations_history(dist_weights, omega_vec, omega, num_itr, sol_avg, lb_first_diff_avg, lb_second_diff_avg, compute_history_for_itr,
                                             history_avg_beta, on_device);
    });
}
int bddmma_learned_iterations_stop_batch(bddmma_batch* b, const void* dist_weights, const void* omega_vec, double omega, uint64_t num_itr,
                                         double improvement_slope, void* sol_avg, void* lb_first_diff_avg, void* lb_second_diff_avg,
                                         uint64_t compute_history_for_itr, double history_avg_beta, int on_device, uint64_t* iterations_done)
{
    return guarded_batch(b, [&](BatchBase* i) {
        return i->learned_iterations_stop(dist_weights, omega_vec, omega, num_itr, improvement_slope, sol_avg, lb_first_diff_avg, lb_second_diff_avg,
                                          compute_history_for_itr, history_avg_beta, on_device, iterations_done);
    });
}
int bddmma_grad_learned_iterations_batch(bddmma_batch* b, const void* dist_weights, const void* omega_vec, double omega, void* grad_lo, void* grad_hi,
                                         void* grad_mm, void* grad_dist_weights_out, void* grad_omega_out, uint64_t track_grad_after_itr,
                                         uint64_t track_grad_for_num_itr, uint64_t num_caches, int on_device)
{
    return guarded_batch(b, [&](BatchBase* i) {
        return i->grad_learned_iterations(dist_weights, omega_vec, omega, grad_lo, grad_hi, grad_mm, grad_dist_weights_out, grad_omega_out, track_grad_after_itr,
                                          track_grad_for_num_itr, num_caches, on_device);
    });
}
int bddmma_grad_learned_iterations_counts_batch(bddmma_batch* b, const void* dist_weights, const void* omega_vec, double omega, void* grad_lo, void* grad_hi,
                                                void* grad_mm, void* grad_dist_weights_out, void* grad_omega_out, const uint64_t* track_grad_after_itr,
                                                const uint64_t* track_grad_for_num_itr, uint64_t num_caches, int on_device)
{
    return guarded_batch(b, [&](BatchBase* i) {
        return i->grad_learned_iterations_counts(dist_weights, omega_vec, omega, grad_lo, grad_hi, grad_mm, grad_dist_weights_out, grad_omega_out,
                                                 track_grad_after_itr, track_grad_for_num_itr, num_caches, on_device);
    });
}
int bddmma_set_solver_costs_batch(bddmma_batch* b, const void* lo, const void* hi, const void* mm, int on_device)
{
    return guarded_batch(b, [&](BatchBase* i) { return i->set_solver_costs(lo, hi, mm, on_device); });
}
int bddmma_get_solver_costs_batch(bddmma_batch* b, void* lo, void* hi, void* mm, int on_device)
{
    return guarded_batch(b, [&](BatchBase* i) { return i->get_solver_costs(lo, hi, mm, on_device); });
}
int bddmma_stream_wait_batch(bddmma_batch* b, void* hip_stream) { return guarded_batch(b, [&](BatchBase* i) { return i->stream_wait((hipStream_t)hip_stream); }); }
int bddmma_stream_signal_batch(bddmma_batch* b, void* hip_stream) { return guarded_batch(b, [&](BatchBase* i) { return i->stream_signal((hipStream_t)hip_stream); }); }
int bddmma_lower_bound_per_bdd_batch(bddmma_batch* b, void* out, int on_device)
{
    return guarded_batch(b, [&](BatchBase* i) {
        if (!out) { i->err = "batch lower_bound_per_bdd: null output pointer"; return (int)BDDMMA_ERR_INVALID_ARGUMENT; }
        return i->lower_bound_per_bdd(out, on_device);
    });
}
int bddmma_grad_lower_bound_per_bdd_batch(bddmma_batch* b, const void* grad_lb_per_bdd, void* grad_lo_out, void* grad_hi_out, int on_device)
{
    return guarded_batch(b, [&](BatchBase* i) {
        if (!grad_lb_per_bdd || !grad_lo_out || !grad_hi_out) { i->err = "batch grad_lower_bound_per_bdd: null pointer"; return (int)BDDMMA_ERR_INVALID_ARGUMENT; }
        return i->grad_lower_bound_per_bdd(grad_lb_per_bdd, grad_lo_out, grad_hi_out, on_device);
    });
}
int bddmma_distribute_delta_batch(bddmma_batch* b) { return guarded_batch(b, [&](BatchBase* i) { return i->distribute_delta(); }); }
int bddmma_min_marginal_diff_batch(bddmma_batch* b, void* out, int on_device)
{
    return guarded_batch(b, [&](BatchBase* i) {
        if (!out) { i->err = "batch min_marginal_diff: null output pointer"; return (int)BDDMMA_ERR_INVALID_ARGUMENT; }
        return i->min_marginal_diff(out, on_device);
    });
}
int bddmma_grad_min_marginal_diff_batch(bddmma_batch* b, const void* grad_mm, void* grad_lo_out, void* grad_hi_out, int on_device)
{
    return guarded_batch(b, [&](BatchBase* i) {
        if (!grad_mm || !grad_lo_out || !grad_hi_out) { i->err = "batch grad_min_marginal_diff: null pointer"; return (int)BDDMMA_ERR_INVALID_ARGUMENT; }
        return i->grad_min_marginal_diff(grad_mm, grad_lo_out, grad_hi_out, on_device);
    });
}
int bddmma_sum_marginals_batch(bddmma_batch* b, int log_probs, void* sm0, void* sm1, int on_device)
{
    return guarded_batch(b, [&](BatchBase* i) {
        if (!sm0 || !sm1) { i->err = "batch sum_marginals: null output pointer"; return (int)BDDMMA_ERR_INVALID_ARGUMENT; }
        return i->sum_marginals(log_probs, sm0, sm1, on_device);
    });
}
int bddmma_smooth_solution_batch(bddmma_batch* b, void* out, int on_device)
{
    return guarded_batch(b, [&](BatchBase* i) {
        if (!out) { i->err = "batch smooth_solution: null output pointer"; return (int)BDDMMA_ERR_INVALID_ARGUMENT; }
        return i->smooth_solution(out, on_device);
    });
}
int bddmma_grad_smooth_lower_bound_per_bdd_batch(bddmma_batch* b, const void* grad_lb_per_bdd, void* grad_lo_out, void* grad_hi_out, int on_device)
{
    return guarded_batch(b, [&](BatchBase* i) {
        if (!grad_lb_per_bdd || !grad_lo_out || !grad_hi_out) { i->err = "batch grad_smooth_lower_bound_per_bdd: null pointer"; return (int)BDDMMA_ERR_INVALID_ARGUMENT; }
        return i->grad_smooth_lower_bound_per_bdd(grad_lb_per_bdd, grad_lo_out, grad_hi_out, on_device);
    });
}
int bddmma_batch_time_iterations(bddmma_batch* b, double omega, uint64_t n, double* ms)
{
    return guarded_batch(b, [&](BatchBase* i) {
        if (!ms) { i->err = "batch: null output pointer"; return (int)BDDMMA_ERR_INVALID_ARGUMENT; }
        return i->time_iterations(omega, n, ms);
    });
}
int bddmma_batch_run_solver(bddmma_batch* b, uint64_t max_iter, double tolerance, double improvement_slope, double time_limit, bddmma_run_result* res)
{
    return guarded_batch(b, [&](BatchBase* i) { return i->run_plain(max_iter, tolerance, improvement_slope, time_limit, res); });
}
int bddmma_lower_bound_batch(bddmma_batch* b, double* out, int on_device)
{
    return guarded_batch(b, [&](BatchBase* i) {
        if (!out) { i->err = "batch lower_bound: null output pointer"; return (int)BDDMMA_ERR_INVALID_ARGUMENT; }
        return i->lower_bounds(out, on_device, true);
    });
}
int bddmma_batch_lower_bounds(bddmma_batch* b, double* out)
{
    return guarded_batch(b, [&](BatchBase* i) {
        if (!out) { i->err = "batch: null output pointer"; return (int)BDDMMA_ERR_INVALID_ARGUMENT; }
        return i->lower_bounds(out, 0, false);
    });
}

// perturb_primal_costs (incremental_mm_agreement_rounding_cuda.cu:262-331).  The cost update goes through the solver type the
// caller holds: with an L-BFGS wrapper that is lbfgs::update_costs, which drops the (s, y) history first (lbfgs_impl.h:343-364).
static int perturb_round(SolverBase* b, bddmma_lbfgs* lbfgs, double cur_delta, uint32_t round, uint32_t seed, uint32_t counts[4], char* sol,
                         void* c0_host, void* c1_host, int* applied)
{
    int rc = b->rounding_round(cur_delta, round, seed, counts, sol, c0_host, c1_host, lbfgs == nullptr, applied);
    if (rc || !*applied || !lbfgs) return rc;
    void *c0 = nullptr, *c1 = nullptr;
    if ((rc = b->rounding_scratch(&c0, &c1))) return rc;
    return bddmma_lbfgs_update_costs(lbfgs, c0, b->n_vars, c1, b->n_vars, b->precision, 1);
}

int bddmma_perturb_primal_costs(bddmma_solver* s, bddmma_lbfgs* lbfgs, double cur_delta, uint32_t round_index, uint32_t seed,
                                uint32_t counts[4], char* sol, void* cost_delta_0, void* cost_delta_1)
{
    if (!sol || !counts) return BDDMMA_ERR_INVALID_ARGUMENT;
    return guarded(s, [&](SolverBase* b) {
        int applied = 0;
        return perturb_round(b, lbfgs, cur_delta, round_index, seed, counts, sol, cost_delta_0, cost_delta_1, &applied);
    });
}

// incremental_mm_agreement_rounding_cuda (incremental_mm_agreement_rounding_cuda.cu:333-372)
int bddmma_incremental_mm_agreement_rounding(bddmma_solver* s, bddmma_lbfgs* lbfgs, double init_delta, double delta_growth_rate,
                                             uint64_t num_itr_lb, uint64_t num_rounds, uint32_t seed, int verbose, char* sol, int* found)
{
    if (!sol || !found) return BDDMMA_ERR_INVALID_ARGUMENT;
    *found = 0;
    return guarded(s, [&](SolverBase* b) {
        if (!(delta_growth_rate > 0) || !(init_delta > 0)) {
            b->err = "rounding: init_delta and delta_growth_rate must be positive";  // asserts at :336-337
            return BDDMMA_ERR_INVALID_ARGUMENT;
        }
        int rc = b->distribute_delta();
        if (rc) return rc;
        double lb;
        if ((rc = b->lower_bound(&lb))) return rc;
        if (verbose) std::printf("[incremental primal rounding] lower bound after distributing delta: %.10g\n", lb);
        double cur_delta = init_delta / delta_growth_rate;
        for (uint64_t round = 0; round < num_rounds; ++round) {
            cur_delta = std::min(cur_delta * delta_growth_rate, 1e6);
            uint32_t counts[4];
            int applied = 0;
            if ((rc = perturb_round(b, lbfgs, cur_delta, (uint32_t)round, seed, counts, sol, nullptr, nullptr, &applied))) return rc;
            if (verbose)
                std::printf("[incremental primal rounding] round %llu, cost delta %g: #ones %u, #zeros %u, #equal %u, #inconsistent %u\n",
                            (unsigned long long)round, cur_delta, counts[0], counts[1], counts[2], counts[3]);
            if (!applied) {
                *found = 1;
                return BDDMMA_OK;
            }
            bddmma_run_result rr;
            rc = bddmma_run_solver(s, lbfgs, num_itr_lb, 1e-7, 0.0001, std::numeric_limits<double>::max(), 0, &rr);  // :366
            if (rc) return rc;
            if (verbose) std::printf("[incremental primal rounding] lower bound = %.10g\n", rr.lb_final);
        }
        return BDDMMA_OK;
    });
}

// ... and both for a batch: bddmma_perturb_primal_costs(member i, NULL, ...) / bddmma_incremental_mm_agreement_rounding(member i, NULL,
// ..., seed, 0, ...) of every member, one launch per round and wave count present (solver_bt.hpp: BatchT::rounding_round, rounding)
int bddmma_perturb_primal_costs_batch(bddmma_batch* b, double cur_delta, uint32_t round_index, uint32_t seed, uint32_t* counts, char* sol,
                                      void* cost_delta_0, void* cost_delta_1)
{
    return guarded_batch(b, [&](BatchBase* i) {
        if (!counts || !sol) { i->err = "batch perturb_primal_costs: null output pointer"; return (int)BDDMMA_ERR_INVALID_ARGUMENT; }
        return i->perturb_primal_costs(cur_delta, round_index, seed, counts, sol, cost_delta_0, cost_delta_1);
    });
}
int bddmma_incremental_mm_agreement_rounding_batch(bddmma_batch* b, double init_delta, double delta_growth_rate, uint64_t num_itr_lb,
                                                   uint64_t num_rounds, uint32_t seed, char* sol, int* found, uint64_t* rounds)
{
    return guarded_batch(b, [&](BatchBase* i) {
        if (!sol || !found) { i->err = "batch rounding: null output pointer"; return (int)BDDMMA_ERR_INVALID_ARGUMENT; }
        if (!(delta_growth_rate > 0) || !(init_delta > 0)) {
            i->err = "batch rounding: init_delta and delta_growth_rate must be positive";
            return (int)BDDMMA_ERR_INVALID_ARGUMENT;
        }
        return i->rounding(init_delta, delta_growth_rate, num_itr_lb, num_rounds, seed, sol, found, rounds);
    });
}

// bddmma_bdds_solution(member i, 0, ..) / bddmma_update_costs(member i, .., nr_variables(i), .., nr_variables(i), ..) /
// bddmma_grad_cost_perturbation(member i, ..) of every member, one launch per kernel instantiation present (solver_bt.hpp:
// BatchT::bdds_solution, update_costs, grad_cost_perturbation)
int bddmma_bdds_solution_batch(bddmma_batch* b, char* sol, int on_device)
{
    return guarded_batch(b, [&](BatchBase* i) {
        if (!sol) { i->err = "batch bdds_solution: null output pointer"; return (int)BDDMMA_ERR_INVALID_ARGUMENT; }
        return i->bdds_solution(sol, on_device);
    });
}
int bddmma_update_costs_batch(bddmma_batch* b, const void* lo, const void* hi, int elem_precision, int on_device)
{
    return guarded_batch(b, [&](BatchBase* i) { return i->update_costs(lo, hi, elem_precision, on_device); });
}
int bddmma_grad_cost_perturbation_batch(bddmma_batch* b, const void* grad_lo, const void* grad_hi, void* grad_lo_pert_out, void* grad_hi_pert_out, int on_device)
{
    return guarded_batch(b, [&](BatchBase* i) {
        if (!grad_lo || !grad_hi || !grad_lo_pert_out || !grad_hi_pert_out) { i->err = "batch grad_cost_perturbation: null pointer"; return (int)BDDMMA_ERR_INVALID_ARGUMENT; }
        return i->grad_cost_perturbation(grad_lo, grad_hi, grad_lo_pert_out, grad_hi_pert_out, on_device);
    });
}

// ---- checkpoint (bdd_cuda_base.cu:1486-1550: every index array of the layout + the costs are archived) -------------------------
// File: magic, header {precision, #arrays, sizeof(LayoutScalars), sizeof(bddmma_options)}, LayoutScalars, options, the layout arrays
// as {id, element size, count, data} records (layout.hpp: visit_layout_arrays), then lo / hi / deferred mm / delta.  Loading
// uploads the arrays as they are: build_layout does not run again.
static const char kMagic[8] = {'B', 'D', 'D', 'M', 'M', 'A', '0', '7'};  // 07: hop_root of the wide packs too; 06: hop_root (staggered packs); 05: checksum of the layout section; 04: narrow node words carry the layer index

namespace {
struct FileCloser {
    FILE* f;
    ~FileCloser() { if (f) std::fclose(f); }
};
}  // namespace

int bddmma_save(const bddmma_solver* s, const char* path)
{
    return guarded(s, [&](SolverBase* b) {
        if (!path) return BDDMMA_ERR_INVALID_ARGUMENT;
        const size_t R = b->precision == BDDMMA_F64 ? 8 : 4;
        HostLayout H;
        int rc = b->download_layout(H);
        if (rc) return rc;
        std::vector<char> lo(b->n_layers * R), hi(b->n_layers * R), mm(b->n_layers * R), delta(2 * b->n_vars * R);
        if ((rc = b->get_solver_costs(lo.data(), hi.data(), mm.data(), 0))) return rc;
        if ((rc = b->get_delta(delta.data(), 0))) return rc;
        FileCloser fc{std::fopen(path, "wb")};
        FILE* f = fc.f;
        if (!f) { b->err = std::string("cannot open ") + path; return BDDMMA_ERR_IO; }
        bool ok = true;
        auto w = [&](const void* p, size_t n) { ok = ok && (n == 0 || std::fwrite(p, 1, n, f) == n); };
        uint64_t n_arrays = 0;
        visit_layout_arrays(H, [&](int, auto&) { ++n_arrays; });
        const uint64_t hdr[4] = {(uint64_t)b->precision, n_arrays, sizeof(LayoutScalars), sizeof(bddmma_options)};
        const LayoutScalars sc = layout_scalars(H);
        w(kMagic, 8); w(hdr, sizeof(hdr)); w(&sc, sizeof(sc)); w(&b->saved_opts, sizeof(bddmma_options));
        Checksum cs;
        cs.add(&sc, sizeof(sc));
        cs.add(&b->saved_opts, sizeof(bddmma_options));
        visit_layout_arrays(H, [&](int id, auto& vec) {
            const uint64_t rec[3] = {(uint64_t)id, sizeof(vec[0]), vec.size()};
            w(rec, sizeof(rec));
            w(vec.data(), vec.size() * sizeof(vec[0]));
            cs.add(rec, sizeof(rec));
            cs.add(vec.data(), vec.size() * sizeof(vec[0]));
        });
        const uint64_t sum = cs.value();
        w(&sum, sizeof(sum));
        w(lo.data(), lo.size()); w(hi.data(), hi.size()); w(mm.data(), mm.size()); w(delta.data(), delta.size());
        fc.f = nullptr;
        ok = (std::fclose(f) == 0) && ok;
        if (!ok) { b->err = std::string("write failed: ") + path; return BDDMMA_ERR_IO; }
        return BDDMMA_OK;
    });
}

int bddmma_load(bddmma_solver** out, int device, const char* path)
{
    if (!out || !path) return BDDMMA_ERR_INVALID_ARGUMENT;
    *out = nullptr;
    FileCloser fc{std::fopen(path, "rb")};
    FILE* f = fc.f;
    if (!f) { g_err = std::string("cannot open ") + path; return BDDMMA_ERR_IO; }
    SolverBase* impl = nullptr;
    try {
        bool ok = true;
        auto r = [&](void* p, size_t n) { ok = ok && (n == 0 || std::fread(p, 1, n, f) == n); };
        if (std::fseek(f, 0, SEEK_END) != 0) { g_err = "cannot seek"; return BDDMMA_ERR_IO; }
        const uint64_t file_size = (uint64_t)std::ftell(f);
        std::rewind(f);
        char magic[8];
        uint64_t hdr[4] = {0, 0, 0, 0};
        r(magic, 8); r(hdr, sizeof(hdr));
        if (!ok || std::memcmp(magic, kMagic, 8) != 0 || hdr[0] > 1 || hdr[2] != sizeof(LayoutScalars) || hdr[3] != sizeof(bddmma_options) ||
            hdr[1] > 1000) {
            g_err = std::string("not a bdd_mma checkpoint (or one of another version): ") + path;
            return BDDMMA_ERR_IO;
        }
        LayoutScalars sc{};
        bddmma_options opts{};
        r(&sc, sizeof(sc)); r(&opts, sizeof(opts));
        HostLayout H;
        set_layout_scalars(H, sc);
        bool bad = false;
        Checksum cs;
        cs.add(&sc, sizeof(sc));
        cs.add(&opts, sizeof(opts));
        for (uint64_t a = 0; a < hdr[1] && ok && !bad; ++a) {
            uint64_t rec[3] = {0, 0, 0};
            r(rec, sizeof(rec));
            if (!ok) break;
            cs.add(rec, sizeof(rec));
            // a count the rest of the file cannot hold means a truncated or corrupt record: refuse before allocating
            if (rec[1] == 0 || rec[1] > 8 || rec[2] > (file_size - (uint64_t)std::ftell(f)) / rec[1]) { bad = true; break; }
            bool found = false;
            visit_layout_arrays(H, [&](int id, auto& vec) {
                if ((uint64_t)id != rec[0] || found) return;
                found = true;
                if (sizeof(vec[0]) != rec[1]) { bad = true; return; }
                vec.resize(rec[2]);
                r(vec.data(), rec[2] * rec[1]);
                if (ok) cs.add(vec.data(), rec[2] * rec[1]);
            });
            if (!found) bad = true;
        }
        std::string why;
        if (ok && !bad) {
            uint64_t sum = 0;
            r(&sum, sizeof(sum));
            if (ok && sum != cs.value()) { bad = true; why = "layout checksum mismatch"; }
        }
        if (!ok || bad || !layout_plausible(H, why)) {
            g_err = "corrupt or truncated checkpoint" + (why.empty() ? std::string() : " (" + why + ")");
            return BDDMMA_ERR_IO;
        }
        {   // the cost section must be complete before a device is touched
            const uint64_t Rb = hdr[0] == (uint64_t)BDDMMA_F64 ? 8 : 4, need = (3 * H.n_layers + 2 * H.n_vars) * Rb;
            if (file_size - (uint64_t)std::ftell(f) < need) { g_err = "corrupt or truncated checkpoint (cost section incomplete)"; return BDDMMA_ERR_IO; }
        }
        int rc = create_solver(&impl, (int)hdr[0], device, H, &opts, g_err);
        if (rc) return rc;
        impl->n_packs_narrow = H.narrow.n_packs();
        impl->n_packs_wide = H.wide.n_packs() + H.huge.n_packs();
        const size_t R = impl->precision == BDDMMA_F64 ? 8 : 4;
        std::vector<char> lo(impl->n_layers * R), hi(impl->n_layers * R), mm(impl->n_layers * R), delta(2 * impl->n_vars * R);
        r(lo.data(), lo.size()); r(hi.data(), hi.size()); r(mm.data(), mm.size()); r(delta.data(), delta.size());
        if (!ok) { g_err = "truncated checkpoint"; delete impl; return BDDMMA_ERR_IO; }
        rc = impl->set_solver_costs(lo.data(), hi.data(), mm.data(), 0);
        if (rc == BDDMMA_OK) rc = impl->set_delta(delta.data(), 0);
        if (rc) { g_err = impl->err; delete impl; return rc; }
        *out = new bddmma_solver{impl};
        return BDDMMA_OK;
    } catch (const std::exception& e) {
        delete impl;
        g_err = e.what();
        return BDDMMA_ERR_IO;
    }
}

int bddmma_synchronize(bddmma_solver* s) { return guarded(s, [&](SolverBase* b) { return b->synchronize(); }); }
int bddmma_stream_wait(bddmma_solver* s, void* hip_stream) { return guarded(s, [&](SolverBase* b) { return b->stream_wait((hipStream_t)hip_stream); }); }
int bddmma_stream_signal(bddmma_solver* s, void* hip_stream) { return guarded(s, [&](SolverBase* b) { return b->stream_signal((hipStream_t)hip_stream); }); }
int bddmma_set_profiling(bddmma_solver* s, int on) { return guarded(s, [&](SolverBase* b) { return b->set_profiling(on); }); }
int bddmma_get_profile(bddmma_solver* s, bddmma_profile* out)
{
    return guarded(s, [&](SolverBase* b) { return out ? b->get_profile(out) : BDDMMA_ERR_INVALID_ARGUMENT; });
}
int bddmma_time_kernel(bddmma_solver* s, int kind, uint64_t reps, double* ms)
{
    return guarded(s, [&](SolverBase* b) { return ms ? b->time_kernel(kind, reps, ms) : BDDMMA_ERR_INVALID_ARGUMENT; });
}
int bddmma_time_iterations(bddmma_solver* s, double omega, uint64_t n, double* ms)
{
    return guarded(s, [&](SolverBase* b) { return ms ? b->time_iterations(omega, n, ms) : BDDMMA_ERR_INVALID_ARGUMENT; });
}

// ---- host-only debug ABI (no GPU needed): lets CPU tests inspect the device layout ---------------
struct bddmma_layout {
    HostLayout L;
};
int bddmma_layout_create(bddmma_layout** out, const bddmma_instruction* instr, const uint64_t* delims, uint64_t n_bdds,
                         const bddmma_options* opts)
{
    return bddmma_layout_create_for_chip(out, instr, delims, n_bdds, opts, 4, 0, 0);
}
int bddmma_layout_create_for_chip(bddmma_layout** out, const bddmma_instruction* instr, const uint64_t* delims, uint64_t n_bdds,
                                  const bddmma_options* opts, int real_size, uint32_t n_cus, uint32_t lds_bytes_per_cu)
{
    if (!out || (real_size != 4 && real_size != 8)) return BDDMMA_ERR_INVALID_ARGUMENT;
    *out = nullptr;
    try {
        auto* l = new bddmma_layout();
        ChipInfo chip;
        if (n_cus) chip.n_cus = n_cus;
        if (lds_bytes_per_cu) chip.lds_bytes = lds_bytes_per_cu;
        int rc = build_layout(instr, delims, n_bdds, opts, l->L, g_err, true, (uint32_t)real_size, chip);
        if (rc) { delete l; return rc; }
        *out = l;
        return BDDMMA_OK;
    } catch (const std::exception& e) {
        g_err = e.what();
        return BDDMMA_ERR_DEVICE;
    }
}
void bddmma_layout_destroy(bddmma_layout* l) { delete l; }
// what: 0 n_slots, 1 narrow_slots, 2 n_layers, 3 narrow packs, 4 wide packs, 5 n_hops, 6 n_vars,
//       7 narrow (pack,hop) records, 8 wide (pack,hop) records, 9 bins, 10 vars per bin, 11 stage groups,
//       12 narrow layers, 13 stage cap, 14 waves per block, 15 (quad, round) records, 16 pack width,
//       17 huge packs, 18 huge (pack,hop) records, 19 huge pack width, 20 distinct narrow words stored on the device,
//       21 entries ordered by (variable, bdd), 22 resident sweeps possible, 23 / 24 largest narrow pack in slots / layers
uint64_t bddmma_layout_size(const bddmma_layout* l, int what)
{
    const HostLayout& L = l->L;
    if (what >= 100) {  // 100 + id: elements of that array of the checkpoint format (layout.hpp: visit_layout_arrays)
        uint64_t n = 0;
        visit_layout_arrays(L, [&](int id, const auto& v) { if (id == what - 100) n = v.size(); });
        return n;
    }
    switch (what) {
        case 0: return L.n_slots;
        case 1: return L.narrow_slots;
        case 2: return L.n_layers;
        case 3: return L.narrow.n_packs();
        case 4: return L.wide.n_packs();
        case 5: return L.n_hops;
        case 6: return L.n_vars;
        case 7: return L.narrow.hop_node_off.empty() ? 0 : L.narrow.hop_node_off.size() - 1;
        case 8: return L.wide.hop_node_off.empty() ? 0 : L.wide.hop_node_off.size() - 1;
        case 9: return L.ex.n_bins;
        case 10: return L.ex.vars_per_bin;
        case 11: return L.ex.grp_hop_end.size();
        case 12: return L.ex.grp_layer_off.empty() ? 0 : L.ex.grp_layer_off.back();
        case 13: return L.ex.stage_cap;
        case 14: return L.ex.waves_per_block;
        case 16: return L.pack_width;
        case 17: return L.huge.n_packs();
        case 18: return L.huge.hop_node_off.empty() ? 0 : L.huge.hop_node_off.size() - 1;
        case 19: return L.huge_pack_width;
        case 20: return L.narrow_words_unique.size();
        case 15: return L.ex.cs_ptr.empty() ? 0 : L.ex.cs_ptr.size() - 1;
        case 21: return L.ex.entry_by_var ? 1 : 0;
        case 22: return L.res.ok ? 1 : 0;
        case 23: return L.res.max_slots;
        case 24: return L.res.max_layers;
        default: return 0;
    }
}
// which: 0 narrow_words(u32) 1 wide_words(u64) 2 slot_to_instr(u64) 3 layer_var(i32) 4 layer_bdd(i32)
//        5/6/7/8 narrow pack_hop_ptr/hop_node_off/hop_layer_off(u32)/pack_steps(u8)   9/10/11/12 wide ...
//        13 var_ptr(u32) 14 var_layers(u32) 15 bdd_root_slot(u32)
//        16 bin_ptr(u32) 17 evar(u32) 18 lpos(u32) 19 vpos(u32) 20 pack_group_ptr 21 grp_layer_off 22 grp_hop_end
//        23 quad_round_ptr 24 cs_ptr 25 cs_entry(u32) 26 cs_slot(u16)   27/28/29/30 huge pack_hop_ptr/hop_node_off/hop_layer_off/pack_steps
//        31 narrow_words_unique(u32) 32 narrow_word_off(u32, per narrow pack)
//        35 pack_hdr(u32 x 8 per narrow pack) 36 quad_hdr(u32 x 4 per quad)
int bddmma_layout_copy(const bddmma_layout* l, int which, void* out)
{
    const HostLayout& L = l->L;
    auto cp = [&](const auto& v) {
        if (!v.empty()) std::memcpy(out, v.data(), v.size() * sizeof(v[0]));
        return BDDMMA_OK;
    };
    if (which >= 100) {  // 100 + id: that array of the checkpoint format
        int rc = BDDMMA_ERR_INVALID_ARGUMENT;
        visit_layout_arrays(L, [&](int id, const auto& v) { if (id == which - 100) rc = cp(v); });
        return rc;
    }
    switch (which) {
        case 0: return cp(L.narrow_words);
        case 1: return cp(L.wide_words);
        case 2: return cp(L.slot_to_instr);
        case 3: return cp(L.layer_var);
        case 4: return cp(L.layer_bdd);
        case 5: return cp(L.narrow.pack_hop_ptr);
        case 6: return cp(L.narrow.hop_node_off);
        case 7: return cp(L.narrow.hop_layer_off);
        case 8: return cp(L.narrow.pack_steps);
        case 9: return cp(L.wide.pack_hop_ptr);
        case 10: return cp(L.wide.hop_node_off);
        case 11: return cp(L.wide.hop_layer_off);
        case 12: return cp(L.wide.pack_steps);
        case 13: return cp(L.var_ptr);
        case 14: return cp(L.var_layers);
        case 15: return cp(L.bdd_root_slot);
        case 16: return cp(L.ex.bin_ptr);
        case 17: return cp(L.ex.evar);
        case 18: return cp(L.ex.lpos);
        case 19: return cp(L.ex.vpos);
        case 20: return cp(L.ex.pack_group_ptr);
        case 21: return cp(L.ex.grp_layer_off);
        case 22: return cp(L.ex.grp_hop_end);
        case 23: return cp(L.ex.quad_round_ptr);
        case 24: return cp(L.ex.cs_ptr);
        case 25: return cp(L.ex.cs_entry);
        case 26: return cp(L.ex.cs_slot);
        case 27: return cp(L.huge.pack_hop_ptr);
        case 28: return cp(L.huge.hop_node_off);
        case 29: return cp(L.huge.hop_layer_off);
        case 30: return cp(L.huge.pack_steps);
        case 31: return cp(L.narrow_words_unique);
        case 32: return cp(L.narrow_word_off);
        case 35: return cp(L.res.pack_hdr);
        case 36: return cp(L.res.quad_hdr);
        default: return BDDMMA_ERR_INVALID_ARGUMENT;
    }
}
int bddmma_layout_res2_records(const bddmma_layout* l, int real_size, uint32_t* info, uint32_t* words, uint32_t* rec_off)
{
    if (!l || !info || (real_size != 4 && real_size != 8)) return BDDMMA_ERR_INVALID_ARGUMENT;
    const HostLayout& L = l->L;
    const uint32_t ns = res2_slot_capacity((uint32_t)real_size, L.res.max_slots), nl = res2_layer_capacity((uint32_t)real_size, L.res.max_layers);  // as SolverT::init
    Res2Records R;
    build_res2_records(L, (uint32_t)real_size, ns, nl, R);
    info[0] = R.ok ? 1u : 0u; info[1] = (uint32_t)R.rec.size(); info[2] = ns; info[3] = nl; info[4] = R.max_hops;
    if (words && !R.rec.empty()) std::memcpy(words, R.rec.data(), R.rec.size() * sizeof(uint32_t));
    if (rec_off && !R.rec_off.empty()) std::memcpy(rec_off, R.rec_off.data(), R.rec_off.size() * sizeof(uint32_t));
    return BDDMMA_OK;
}

int bddmma_layout_seg_exchange(const bddmma_layout* l, int threads, int real_size, uint32_t* info, uint32_t* bin, uint16_t* perm, uint32_t* thr)
{
    if (!l || !info || (real_size != 4 && real_size != 8) || threads <= 0) return BDDMMA_ERR_INVALID_ARGUMENT;
    SegExchange S;
    build_seg_exchange(l->L, (uint32_t)threads, (uint32_t)real_size, S);
    info[0] = S.ok ? 1u : 0u; info[1] = (uint32_t)S.bin.size(); info[2] = (uint32_t)S.perm.size(); info[3] = (uint32_t)S.thr.size();
    info[4] = S.max_entries; info[5] = S.max_slots; info[6] = S.max_groups;
    if (bin && !S.bin.empty()) std::memcpy(bin, S.bin.data(), S.bin.size() * sizeof(uint32_t));
    if (perm && !S.perm.empty()) std::memcpy(perm, S.perm.data(), S.perm.size() * sizeof(uint16_t));
    if (thr && !S.thr.empty()) std::memcpy(thr, S.thr.data(), S.thr.size() * sizeof(uint32_t));
    return BDDMMA_OK;
}

int bddmma_layout_stream_records(const bddmma_layout* l, int real_size, uint32_t* info, uint32_t* words, uint32_t* rec_off)
{
    if (!l || !info || (real_size != 4 && real_size != 8)) return BDDMMA_ERR_INVALID_ARGUMENT;
    StreamRecords R;
    build_stream_records(l->L, (uint32_t)real_size, R);
    info[0] = R.ok ? 1u : 0u; info[1] = (uint32_t)R.rec.size();
    if (words && !R.rec.empty()) std::memcpy(words, R.rec.data(), R.rec.size() * sizeof(uint32_t));
    if (rec_off && !R.rec_off.empty()) std::memcpy(rec_off, R.rec_off.data(), R.rec_off.size() * sizeof(uint32_t));
    return BDDMMA_OK;
}

int bddmma_layout_layer_records(const bddmma_layout* l, int real_size, uint32_t* info, uint32_t* words, uint32_t* rec_off)
{
    if (!l || !info || (real_size != 4 && real_size != 8)) return BDDMMA_ERR_INVALID_ARGUMENT;
    LayerRecords R;
    build_layer_records(l->L, (uint32_t)real_size, R);
    info[0] = R.ok ? 1u : 0u; info[1] = (uint32_t)R.rec.size();
    if (words && !R.rec.empty()) std::memcpy(words, R.rec.data(), R.rec.size() * sizeof(uint32_t));
    if (rec_off && !R.rec_off.empty()) std::memcpy(rec_off, R.rec_off.data(), R.rec_off.size() * sizeof(uint32_t));
    return BDDMMA_OK;
}

int bddmma_layout_lane_codes(const bddmma_layout* l, int real_size, uint32_t* info, uint32_t* words, uint32_t* code_off)
{
    if (!l || !info || (real_size != 4 && real_size != 8)) return BDDMMA_ERR_INVALID_ARGUMENT;
    LayerRecords R;
    build_layer_records(l->L, (uint32_t)real_size, R);
    LaneCodes K;
    build_lane_codes(l->L, (uint32_t)real_size, R, K);
    info[0] = K.ok ? 1u : 0u; info[1] = (uint32_t)K.words.size(); info[2] = K.affine ? 1u : 0u;
    if (words && !K.words.empty()) std::memcpy(words, K.words.data(), K.words.size() * sizeof(uint32_t));
    if (code_off && !K.code_off.empty()) std::memcpy(code_off, K.code_off.data(), K.code_off.size() * sizeof(uint32_t));
    return BDDMMA_OK;
}

}  // extern "C"
