// solver.hpp — precision-erased solver interface behind the C-ABI (include/bdd_mma.h).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <limits>
#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "../../include/bdd_mma.h"
#include "layout.hpp"

namespace bddmma {

struct SolverBase {
    int precision = BDDMMA_F32, device = -1;
    hipStream_t stream = nullptr;
    std::string err;
    uint64_t n_vars = 0, n_bdds = 0, n_layers = 0, n_hops = 0, n_input_nodes = 0, n_slots = 0;
    int solve_sweep_kind = 0;  // bddmma_solve_sweep_kind (include/bdd_mma.h): which kernels run the narrow packs' solve sweeps
    uint32_t pack_width = 0, wide_pack_width = 0, wide_slot_base = 0;
    uint64_t dev_bytes = 0;          // bytes of the arrays the solver holds
    uint64_t dev_alloc_bytes = 0;    // bytes hipMalloc'd for them (arena capacity included: >= dev_bytes)
    bool fwd_valid = false, bwd_valid = false;  // forward_state_valid_ / backward_state_valid_ (bdd_cuda_base.h:205-206): d_F / d_T in memory are current
    // lb_partial belongs to the current costs: set by every backward sweep, cleared by whatever clears bwd_valid.  Differs from bwd_valid after
    // the on-chip solve sweeps of iteration() (kernels/narrow4.hpp), which leave the bound's partial sums but no costs-to-terminal in memory.
    bool lb_valid = false;
    uint64_t cost_epoch = 0;                    // counts the calls that changed arc costs other than through a solve sweep (update_costs, set_cost, gradient steps, ...)
    bool deterministic = false;
    std::vector<uint64_t> nodes_per_hop, layers_per_hop;
    std::vector<int32_t> h_nbdds, h_layer_var, h_layer_bdd;
    std::vector<uint32_t> h_var_ptr;
    uint32_t n_packs_narrow = 0, n_packs_wide = 0;
    // checkpoint support (bdd_cuda_base.cu:1486-1550): the layout itself is archived — scalars here, arrays fetched from the device
    LayoutScalars lay_scalars{};
    bddmma_options saved_opts{};
    virtual int download_layout(HostLayout& H) = 0;  // rebuilds a HostLayout from what the device holds
    virtual int init_from_layout(const HostLayout& L, const bddmma_options* opts) = 0;  // device buffers + upload (create_solver)

    // profiling: one hipEvent pair per launch group on `stream`
    bool profiling = false;        // hipEvent pairs are recorded for every `prof_stride`-th iteration only: an event
    uint32_t prof_stride = 1;      // pair per launch costs ~4 us of stream time (measured: -14 % it/s at stride 1)
    uint64_t prof_iter = 0;
    bool prof_active = false;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev_pool;
    std::vector<int> ev_class;
    size_t ev_used = 0;
    hipEvent_t ev_t0 = nullptr, ev_t1 = nullptr;
    hipEvent_t ev_order = nullptr;  // bddmma_stream_wait / _signal: timing disabled, created on first use

    virtual ~SolverBase() {}
    virtual int forward_run() = 0;
    virtual int backward_run() = 0;
    virtual int lower_bound(double* lb) = 0;
    // The same bound without the host waiting for it: enqueue the backward run + reduction into one of two pinned slots, fetch it
    // later (the fetch waits for the stream).  The value is the bound of the costs at enqueue time, whatever was enqueued behind it.
    virtual int lower_bound_enqueue(int slot) = 0;
    virtual int lower_bound_fetch(int slot, double* lb) = 0;
    virtual int lower_bound_per_bdd(void* out, int on_device) = 0;
    virtual int iteration(double omega) = 0;
    // n iterations; instances that fit one workgroup run them inside one launch (kernels/small.hpp), everything else calls iteration() n times
    virtual int iterations(double omega, uint64_t n)
    {
        for (uint64_t i = 0; i < n; ++i)
            if (int rc = iteration(omega)) return rc;
        return BDDMMA_OK;
    }
    // bdd_cuda_learned_mma::iterations (bdd_cuda_learned_mma.cu:184-270): iterations with per-layer distribution weights, the state
    // contract of include/bdd_mma.h (bddmma_learned_iterations); omega_vec non-null: one omega per layer in place of the scalar
    // (bddmma_learned_iterations_omega_vec)
    virtual int learned_iterations(const void* dist_weights, int weights_on_device, uint64_t num_itr, double omega, double improvement_slope,
                                   void* sol_avg, void* lb_first_diff_avg, void* lb_second_diff_avg, uint64_t compute_history_for_itr,
                                   double history_avg_beta, int outputs_on_device, uint64_t* itr_done, const void* omega_vec,
                                   int omega_vec_on_device) = 0;
    virtual int isotropic_dist_weights(void* out, int on_device) = 0;
    double initial_lb_change = std::numeric_limits<double>::infinity();  // set_initial_lb_change (bdd_cuda_learned_mma.h:111-116): set once
    // number of L-BFGS wrappers attached to this solver (bddmma_lbfgs_create / _destroy); shared so that a wrapper destroyed after its
    // solver does not touch freed memory
    std::shared_ptr<int> lbfgs_attached = std::make_shared<int>(0);
    bool fused_small = false;   // whole iterations in one launch (diagnostics: bddmma_fused_small)
    bool fused_small_learned = false;   // ... and whole learned iterations (bddmma_fused_small_learned)
    bool fused_small_history = false;   // ... and their history step, in a batch (bddmma_fused_small_history)
    bool fused_small_stop = false;      // ... and the stopping rule on the bound's slope, in a batch (bddmma_fused_small_stop)
    bool nt_loads = false;      // the solve sweeps' non-temporal instantiation (diagnostics: bddmma_nontemporal_loads)
    bool pot_on_chip = false;   // iteration()'s solve sweeps rebuild F and T on chip (diagnostics: bddmma_potentials_on_chip)
    bool lane_sweeps = false;   // ... and they are the lane-per-BDD pair, kernels/narrow5.hpp (diagnostics: bddmma_lane_sweeps)
    int onchip_hops = 0;        // ... the hop capacity of the kernels that do: 0, 10, 12 or 16 (diagnostics: bddmma_onchip_hops)
    // run_solver (include/run_solver_util.h:10-77) around iteration(): termination tests on the device, see solver_impl.hpp
    virtual int run_plain(uint64_t max_iter, double tolerance, double slope, double time_limit, int verbose, bddmma_run_result* res) = 0;
    virtual int forward_mm(double omega, void* delta, int on_device) = 0;
    virtual int backward_mm(double omega, void* delta, int on_device) = 0;
    virtual int normalize_delta(void* delta, int on_device) = 0;
    virtual int distribute_delta() = 0;
    virtual int get_delta(void* out, int on_device) = 0;
    virtual int set_delta(const void* in, int on_device) = 0;
    virtual int update_costs(const void* lo, uint64_t n_lo, const void* hi, uint64_t n_hi, int elem_precision, int on_device) = 0;
    virtual int set_cost(double c, uint64_t var) = 0;
    virtual int get_solver_costs(void* lo, void* hi, void* mm, int on_device) = 0;
    virtual int set_solver_costs(const void* lo, const void* hi, const void* mm, int on_device) = 0;
    virtual int primal_objective_vec(void* out, int on_device) = 0;
    virtual int min_marginals(int sorted, int32_t* var, void* mm0, void* mm1, int on_device) = 0;
    virtual int min_marginal_diff(void* out, int on_device) = 0;
    // sum_marginals_cuda(get_sorted, get_log_probs) / smooth_solution_cuda (bdd_cuda_base.cu:788-1064): the sweeps in the (log-sum-exp, +)
    // semiring; state contract in include/bdd_mma.h (bddmma_sum_marginals)
    virtual int sum_marginals(int sorted, int log_probs, int32_t* var, void* sm0, void* sm1, int on_device) = 0;
    virtual int smooth_solution(void* out, int on_device) = 0;
    // the single-shot backward operators of bdd_cuda_learned_mma (bdd_cuda_learned_mma.h:82-110): transpose-Jacobian products with respect to
    // the arc costs; arrays in layer order, state contracts in include/bdd_mma.h (bddmma_grad_*)
    virtual int grad_min_marginal_diff(const void* grad_mm, void* grad_lo, void* grad_hi, int on_device) = 0;
    virtual int grad_lower_bound_per_bdd(const void* grad_lb, void* grad_lo, void* grad_hi, int smooth, int on_device) = 0;
    virtual int grad_distribute_delta(const void* grad_lo, const void* grad_hi, void* grad_deferred_mm, int on_device) = 0;
    virtual int grad_cost_perturbation(const void* grad_lo, const void* grad_hi, void* grad_lo_pert, void* grad_hi_pert, int on_device) = 0;
    // grad_iterations (bdd_cuda_learned_mma.cu:308-385): the transpose-Jacobian product of `n` learned iterations run after `after` untracked
    // ones; grad_lo / grad_hi / grad_mm in-out; contract in include/bdd_mma.h (bddmma_grad_learned_iterations)
    virtual int grad_learned_iterations(const void* dist_weights, int weights_on_device, double omega, const void* omega_vec, int omega_vec_on_device,
                                        void* grad_lo, void* grad_hi, void* grad_mm, void* grad_dist_weights_out, void* grad_omega_out, uint64_t after,
                                        uint64_t n, uint64_t num_caches, int on_device) = 0;
    virtual int bdds_solution(int sorted, char* sol, int on_device) = 0;
    virtual int net_solver_costs(void* out, int on_device) = 0;
    virtual int make_dual_feasible(void* g, int on_device) = 0;
    virtual int gradient_step(const void* g, double step, int on_device) = 0;
    virtual int projection_means(const void* g_dev) = 0;                       // per-variable means of a device vector, kept inside the solver
    virtual int gradient_step_projected(const void* g_dev, double step) = 0;   // costs += step * (g - its per-variable mean)
    // projection_means of a vector that is a linear combination of stored ones (layout.hpp: LinComb), formed on the fly; `tag` is what
    // gradient_step_projected will be called with.  Only where projection_fuses_lincomb() (staged projection, narrow packs only).
    virtual bool projection_fuses_lincomb() const = 0;
    virtual int projection_means_lincomb(const LinComb& lc, const void* tag) = 0;
    virtual void* stream_handle() = 0;
    // L-BFGS wrapper (lbfgs.hip): the argmin paths straight into a device buffer with nothing but stream order (bdds_solution() also
    // copies and synchronises; `prezeroed`: the caller has left the buffer all 0, the sweep only writes the layers on a path), and
    // net_solver_costs() as a view: x = (hi - lo) + deferred mm per layer.
    struct LbfgsViews {
        const void* x_layer;       // REAL per layer
    };
    virtual int bdds_solution_async(char* dev_out, int prezeroed) = 0;
    // From the first call on the backward solve sweeps also write x in layer order (one coalesced 4-8 byte store per layer, formed from
    // the new arc costs and the deferred difference while both are in the sweep's hands), so that the wrapper reads x without the 5 M random
    // gathers of net_solver_costs() and without re-reading {lo, hi}; rebuilt by net_solver_costs()'s gather when something else has changed
    // costs or deferred values since the last backward solve sweep.
    virtual int lbfgs_views(LbfgsViews* out) = 0;
    virtual int time_kernel(int kind, uint64_t reps, double* ms) = 0;
    // one round of perturb_primal_costs (incremental_mm_agreement_rounding_cuda.cu:262-331); counts = #one,#zero,#equal,#inconsistent
    // `applied` = 0 when the solution was read off (all variables one / zero) and the costs were left alone; c0_host / c1_host
    // (REAL[n_vars], may be null) receive the perturbation.  With apply_update = false the perturbation is computed but not applied.
    virtual int rounding_round(double delta, uint32_t round, uint32_t seed, uint32_t counts[4], char* sol_host, void* c0_host, void* c1_host,
                               bool apply_update, int* applied) = 0;
    virtual int rounding_scratch(void** c0_dev, void** c1_dev) = 0;  // device vectors holding the last perturbation (REAL[n_vars] each)

    int synchronize();
    // bddmma_stream_wait / bddmma_stream_signal: `stream` behind everything queued on `other` so far / the reverse, by an event; the host
    // does not wait (the batch object orders its stream against its members' the same way, solver_bt.hpp)
    int stream_wait(hipStream_t other);
    int stream_signal(hipStream_t other);
    void prof_begin(int kclass);
    void prof_end(int kclass);
    int set_profiling(int on);
    int get_profile(bddmma_profile* out);
    int time_iterations(double omega, uint64_t n, double* ms);
};

// A batch of solvers whose instances fit one workgroup each (fused_small): its calls run every member's iterations concurrently, one
// workgroup per member, one launch per kernel instantiation present (kernels/small.hpp: k_iterate_small_batch; solver_bt.hpp: BatchT).
// The members are borrowed: they must outlive the batch, and they stay usable on their own between the batch's calls.
//
// Ordering: a call behaves as if the same call had been made on each member in turn.  The batch has a stream of its own; a call first
// records an event on every member's stream and makes the batch stream wait for it (ordered after everything queued on the members),
// launches, then records one event on the batch stream that every member's stream waits for (everything queued on a member afterwards
// is ordered after the call).  No host synchronisation; two event calls per member and call on entry, one on exit.
//
// State refusals are made per call, before anything is launched: BDDMMA_ERR_STATE and every member untouched when a member has
// profiling on, has (had) an L-BFGS wrapper attached or is inside run_solver.
struct BatchBase {
    std::string err;
    virtual ~BatchBase() {}
    virtual uint64_t size() const = 0;
    virtual int iterations(double omega, uint64_t n) = 0;   // SolverBase::iterations(omega, n) of every member
    // run_plain of every member (tests in its workgroup, its own control block; one clock and one time limit for the batch); res[size()]
    // mask (may be null): size() entries in member order; a member whose entry is non-zero takes no part and keeps its state
    virtual int run_plain(uint64_t max_iter, double tolerance, double slope, double time_limit, bddmma_run_result* res, const char* mask = nullptr) = 0;
    virtual int time_iterations(double omega, uint64_t n, double* ms) = 0;   // iterations() between hipEvents on the batch stream; waits
    // SolverBase::lower_bound of every member: the stale members' backward sweeps and every member's reduction in one launch per wave count
    // present (kernels/batchlb.hpp), one host wait.  on_device: the doubles go to the caller's device array on the batch's stream, the host
    // does not wait and no cached bound is set.  check_members: the refusals of every batch call first (include/bdd_mma.h:
    // bddmma_lower_bound_batch; bddmma_batch_lower_bounds passes false)
    virtual int lower_bounds(double* out, int on_device = 0, bool check_members = false) = 0;
    // SolverBase::learned_iterations(w_i, num_itr, omega, slope 0, no history) of every member, or its omega_vec form; dist_weights /
    // omega_vec: the members' REAL[nr_layers] one behind the other in the caller's order (include/bdd_mma.h: bddmma_learned_iterations_batch)
    virtual int learned_iterations(const void* dist_weights, const void* omega_vec, double omega, uint64_t num_itr, int on_device) = 0;
    // ... with compute_history_for_itr / history_avg_beta and the three history outputs: sol_avg as the layer arrays, the two per-BDD
    // arrays the members' REAL[nr_bdds] one behind the other (include/bdd_mma.h: bddmma_learned_iterations_history_batch)
    virtual int learned_iterations_history(const void* dist_weights, const void* omega_vec, double omega, uint64_t num_itr, void* sol_avg,
                                           void* lb_first_diff_avg, void* lb_second_diff_avg, uint64_t compute_history_for_itr, double history_avg_beta,
                                           int on_device) = 0;
    // SolverBase::learned_iterations(w_i, num_itr, omega, improvement_slope, history) of every member with the member's count of iterations
    // run in iterations_done[i]: the stopping rule inside the member's workgroup (include/bdd_mma.h: bddmma_learned_iterations_stop_batch)
    virtual int learned_iterations_stop(const void* dist_weights, const void* omega_vec, double omega, uint64_t num_itr, double improvement_slope,
                                        void* sol_avg, void* lb_first_diff_avg, void* lb_second_diff_avg, uint64_t compute_history_for_itr,
                                        double history_avg_beta, int on_device, uint64_t* iterations_done) = 0;
    // SolverBase::grad_learned_iterations of every member with its part of every array, one workgroup per member in one launch
    // (include/bdd_mma.h: bddmma_grad_learned_iterations_batch)
    virtual int grad_learned_iterations(const void* dist_weights, const void* omega_vec, double omega, void* grad_lo, void* grad_hi, void* grad_mm,
                                        void* grad_dist_weights_out, void* grad_omega_out, uint64_t track_grad_after_itr, uint64_t track_grad_for_num_itr,
                                        uint64_t num_caches, int on_device) = 0;
    // ... with member i's own two counts in track_grad_after_itr[i] / track_grad_for_num_itr[i] (host arrays; include/bdd_mma.h:
    // bddmma_grad_learned_iterations_counts_batch)
    virtual int grad_learned_iterations_counts(const void* dist_weights, const void* omega_vec, double omega, void* grad_lo, void* grad_hi, void* grad_mm,
                                               void* grad_dist_weights_out, void* grad_omega_out, const uint64_t* track_grad_after_itr,
                                               const uint64_t* track_grad_for_num_itr, uint64_t num_caches, int on_device) = 0;
    // SolverBase::set_solver_costs followed by backward_run of every member / SolverBase::get_solver_costs of every member, one launch per
    // kernel instantiation present; the arrays as in learned_iterations, each may be null (include/bdd_mma.h: bddmma_set_solver_costs_batch)
    virtual int set_solver_costs(const void* lo, const void* hi, const void* mm, int on_device) = 0;
    virtual int get_solver_costs(void* lo, void* hi, void* mm, int on_device) = 0;
    // SolverBase::lower_bound_per_bdd / grad_lower_bound_per_bdd (smooth = 0) / distribute_delta of every member, one launch per kernel
    // instantiation present (kernels/batchbound.hpp); per-BDD arrays: the members' REAL[nr_bdds] one behind the other, layer arrays as in
    // learned_iterations (include/bdd_mma.h: bddmma_lower_bound_per_bdd_batch, bddmma_grad_lower_bound_per_bdd_batch, bddmma_distribute_delta_batch)
    virtual int lower_bound_per_bdd(void* out, int on_device) = 0;
    virtual int grad_lower_bound_per_bdd(const void* grad_lb, void* grad_lo, void* grad_hi, int on_device) = 0;
    virtual int distribute_delta() = 0;
    // SolverBase::min_marginal_diff / grad_min_marginal_diff of every member, one launch per kernel instantiation present
    // (kernels/batchmm.hpp; include/bdd_mma.h: bddmma_min_marginal_diff_batch, bddmma_grad_min_marginal_diff_batch)
    virtual int min_marginal_diff(void* out, int on_device) = 0;
    virtual int grad_min_marginal_diff(const void* grad_mm, void* grad_lo, void* grad_hi, int on_device) = 0;
    // SolverBase::sum_marginals (unsorted, no var) / smooth_solution / grad_lower_bound_per_bdd (smooth = 1) of every member, one launch
    // per kernel instantiation present (kernels/batchsm.hpp; include/bdd_mma.h: bddmma_sum_marginals_batch, bddmma_smooth_solution_batch,
    // bddmma_grad_smooth_lower_bound_per_bdd_batch)
    virtual int sum_marginals(int log_probs, void* sm0, void* sm1, int on_device) = 0;
    virtual int smooth_solution(void* out, int on_device) = 0;
    virtual int grad_smooth_lower_bound_per_bdd(const void* grad_lb, void* grad_lo, void* grad_hi, int on_device) = 0;
    // SolverBase::rounding_round (apply_update) of every member in one launch per kernel instantiation present, and the loop of
    // bddmma_incremental_mm_agreement_rounding over all members at once (kernels/batchround.hpp; include/bdd_mma.h:
    // bddmma_perturb_primal_costs_batch, bddmma_incremental_mm_agreement_rounding_batch); host arrays, per-variable ones the members'
    // nr_variables entries one behind the other
    virtual int perturb_primal_costs(double delta, uint32_t round, uint32_t seed, uint32_t* counts, char* sol, void* c0, void* c1) = 0;
    virtual int rounding(double init_delta, double growth, uint64_t num_itr_lb, uint64_t num_rounds, uint32_t seed, char* sol, int* found, uint64_t* rounds) = 0;
    // SolverBase::bdds_solution (unsorted) / update_costs (both vectors full length or null) / grad_cost_perturbation of every member, one
    // launch per kernel instantiation present (kernels/batchsol.hpp; include/bdd_mma.h: bddmma_bdds_solution_batch,
    // bddmma_update_costs_batch, bddmma_grad_cost_perturbation_batch); per-variable arrays: the members' nr_variables entries one behind
    // the other, layer arrays as in learned_iterations
    virtual int bdds_solution(char* sol, int on_device) = 0;
    virtual int update_costs(const void* lo, const void* hi, int elem_precision, int on_device) = 0;
    virtual int grad_cost_perturbation(const void* grad_lo, const void* grad_hi, void* grad_lo_pert, void* grad_hi_pert, int on_device) = 0;
    // the batch stream behind everything queued on `other` so far / the reverse, by an event the batch owns; the host does not wait
    virtual int stream_wait(hipStream_t other) = 0;
    virtual int stream_signal(hipStream_t other) = 0;
};
// Refuses (before any device call): BDDMMA_ERR_INVALID_ARGUMENT for n == 0, a null member or a member listed twice; BDDMMA_ERR_UNSUPPORTED for
// a member that is not fused_small or differs from member 0 in precision or device; BDDMMA_ERR_STATE for profiling / an L-BFGS wrapper.
int create_batch(BatchBase** out, SolverBase* const* members, uint64_t n, std::string& err);

int device_count();
int query_chip(int device, ChipInfo* out, std::string& err);  // CU count and LDS per CU of `device` (hipDeviceProp)
int create_solver(SolverBase** out, int precision, int device, const HostLayout& L, const bddmma_options* opts, std::string& err);

}  // namespace bddmma

// the opaque C handles
struct bddmma_solver {
    bddmma::SolverBase* impl = nullptr;
};
struct bddmma_batch {
    bddmma::BatchBase* impl = nullptr;
};
