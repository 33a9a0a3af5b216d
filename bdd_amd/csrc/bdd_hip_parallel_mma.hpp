// bdd_hip_parallel_mma.hpp — header-only C++ class over the C-ABI (include/bdd_mma.h) that satisfies the
// reference's relaxation-solver concept, so it can be listed as one more alternative of
// `bdd_solver::solver_type` (reference: include/bdd_solver/bdd_solver.h:64-69) and constructed where
// `"relaxation solver": "cuda parallel mma"` is handled (src/bdd_solver/bdd_solver.cpp:164-176).
// Member names, argument meaning and error behaviour (std::runtime_error) follow
// LPMP::bdd_cuda_parallel_mma<REAL> / bdd_cuda_base<REAL>.  Needs no HIP headers: device vectors are
// raw device pointers (`device_ptr<REAL>`) owned by the caller or by the handle.
#pragma once
#include <algorithm>
#include <array>
#include <cstdint>
#include <functional>
#include <stdexcept>
#include <string>
#include <tuple>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/bdd_mma.h"

namespace LPMP {

template <typename REAL>
class bdd_hip_parallel_mma {
    static_assert(std::is_same<REAL, float>::value || std::is_same<REAL, double>::value, "REAL must be float or double");

   public:
    using value_type = REAL;
    static constexpr int precision = std::is_same<REAL, double>::value ? BDDMMA_F64 : BDDMMA_F32;

    bdd_hip_parallel_mma() = default;

    // From the flat storage of BDD::bdd_collection: `instr` = bdd_instructions.data() (bit-identical layout),
    // `delims` = bdd_delimiters.data().  Mirrors bdd_cuda_parallel_mma(const bdd_collection&, const std::vector<double>&).
    bdd_hip_parallel_mma(const bddmma_instruction* instr, const uint64_t* delims, size_t nr_bdds,
                         const std::vector<double>& costs_hi = {}, int device = 0, const bddmma_options* opts = nullptr)
    {
        check(bddmma_create(&h_, precision, device, instr, delims, nr_bdds, costs_hi.data(), costs_hi.size(), opts), nullptr);
    }
    // Any type with the accessors of BDD::bdd_collection used by the reference constructor
    // (bdd_cuda_base.cu:55-144): nr_bdds(), nr_bdd_nodes(b), offset(b), operator()(b, i).
    template <typename BDD_COLLECTION, typename = decltype(std::declval<const BDD_COLLECTION&>().nr_bdds())>
    explicit bdd_hip_parallel_mma(const BDD_COLLECTION& bdd_col, const std::vector<double>& costs_hi = {}, int device = 0)
    {
        std::vector<bddmma_instruction> instr;
        std::vector<uint64_t> delims;
        flatten(bdd_col, instr, delims);
        check(bddmma_create(&h_, precision, device, instr.data(), delims.data(), bdd_col.nr_bdds(), costs_hi.data(), costs_hi.size(), nullptr), nullptr);
    }
    // The collection's BDDs as the dense arrays bddmma_create takes (arc targets re-based from the collection's storage offsets to the
    // dense array).  Needs no GPU: oracle/ref_driver.cpp instantiates it with the reference's own BDD::bdd_collection
    // (include/bdd_collection/bdd_collection.h:206 `operator()(bdd_nr, offset)`) and tests/test_bdd_builders.py compares the result with
    // the reference-side export.
    template <typename BDD_COLLECTION>
    static void flatten(const BDD_COLLECTION& bdd_col, std::vector<bddmma_instruction>& instr, std::vector<uint64_t>& delims)
    {
        instr.clear();
        delims.assign(1, 0);
        for (size_t b = 0; b < bdd_col.nr_bdds(); ++b) {
            const size_t off = bdd_col.offset(b), base = instr.size();
            for (size_t i = 0; i < bdd_col.nr_bdd_nodes(b); ++i) {
                const auto in = bdd_col(b, off + i);
                const bool term = in.index >= BDDMMA_BOTSINK;
                instr.push_back({term ? in.lo : in.lo - off + base, term ? in.hi : in.hi - off + base, in.index});
            }
            delims.push_back(instr.size());
        }
    }
    ~bdd_hip_parallel_mma() { bddmma_destroy(h_); }
    bdd_hip_parallel_mma(bdd_hip_parallel_mma&& o) noexcept : h_(o.h_) { o.h_ = nullptr; }
    bdd_hip_parallel_mma& operator=(bdd_hip_parallel_mma&& o) noexcept
    {
        if (this != &o) { bddmma_destroy(h_); h_ = o.h_; o.h_ = nullptr; }
        return *this;
    }
    bdd_hip_parallel_mma(const bdd_hip_parallel_mma&) = delete;
    bdd_hip_parallel_mma& operator=(const bdd_hip_parallel_mma&) = delete;

    // ---- sizes (bdd_cuda_base.h:98-116)
    size_t nr_variables() const { return bddmma_nr_variables(h_); }
    size_t nr_bdds() const { return bddmma_nr_bdds(h_); }
    size_t nr_layers() const { return bddmma_nr_layers(h_); }
    // a bdd_hip_batch can run this solver's learned iterations with their history inside one workgroup (bddmma_fused_small_history)
    bool fused_small_history() const { return bddmma_fused_small_history(h_) == 1; }
    // a bdd_hip_batch can run this solver's stopping rule (improvement_slope > 0) inside its workgroup too (bddmma_fused_small_stop)
    bool fused_small_stop() const { return bddmma_fused_small_stop(h_) == 1; }
    size_t nr_bdd_nodes() const { return bddmma_nr_bdd_nodes(h_); }
    size_t nr_hops() const { return bddmma_nr_hops(h_); }
    size_t nr_bdds(const size_t var) const
    {
        std::vector<int32_t> n(nr_variables());
        check(bddmma_num_bdds_per_var(h_, n.data()));
        return n.at(var);
    }
    // nr_layers(hop) / nr_bdd_nodes(hop), bdd_cuda_base.h:106-113, for hop < nr_hops(): non-terminal layers / nodes at that distance from
    // the roots (the reference counts the terminal layers of BDDs that end at the hop as well; nr_layers() here is non-terminal)
    size_t nr_layers(const int hop_index) const { return per_hop(bddmma_layers_per_hop).at((size_t)hop_index); }
    size_t nr_bdd_nodes(const int hop_index) const { return per_hop(bddmma_nodes_per_hop).at((size_t)hop_index); }
    // var_constraint_indices(), bdd_cuda_base.h:121 / bdd_cuda_base.cu:1450-1461: (primal variable, BDD) of every dual variable, hop-major
    std::pair<std::vector<int>, std::vector<int>> var_constraint_indices() const
    {
        std::vector<int32_t> v(nr_layers()), b(nr_layers());
        check(bddmma_layer_variables(h_, v.data()));
        check(bddmma_layer_bdds(h_, b.data()));
        return {std::vector<int>(v.begin(), v.end()), std::vector<int>(b.begin(), b.end())};
    }
    std::vector<int> get_primal_variable_index() const { return var_constraint_indices().first; }
    std::vector<int> get_bdd_index() const { return var_constraint_indices().second; }
    std::vector<int> get_num_bdds_per_var() const
    {
        std::vector<int32_t> n(nr_variables());
        check(bddmma_num_bdds_per_var(h_, n.data()));
        return std::vector<int>(n.begin(), n.end());
    }

    // ---- costs (bdd_cuda_base.cu:439-558)
    void update_costs(const std::vector<REAL>& cost_delta_0, const std::vector<REAL>& cost_delta_1)
    {
        check(bddmma_update_costs(h_, cost_delta_0.data(), cost_delta_0.size(), cost_delta_1.data(), cost_delta_1.size(), precision, 0));
    }
    void update_costs(const REAL* dev_cost_delta_0, size_t n0, const REAL* dev_cost_delta_1, size_t n1)  // device_vector overload
    {
        check(bddmma_update_costs(h_, dev_cost_delta_0, n0, dev_cost_delta_1, n1, precision, 1));
    }
    void set_cost(const double c, const size_t var) { check(bddmma_set_cost(h_, c, var)); }
    std::vector<REAL> get_primal_objective_vector_host()
    {
        std::vector<REAL> v(nr_variables());
        check(bddmma_primal_objective_vec(h_, v.data(), 0));
        return v;
    }
    void compute_primal_objective_vec(REAL* dev_primal_obj) { check(bddmma_primal_objective_vec(h_, dev_primal_obj, 1)); }
    // get_solver_costs / set_solver_costs, bdd_cuda_base.h:124-135 (bdd_cuda_base.cu:1308-1344): {lo, hi, deferred mm difference}, nr_layers() each.
    // Device pointers as in the reference; the tuple-returning form hands out host vectors (no device_vector type here).
    void get_solver_costs(REAL* dev_lo, REAL* dev_hi, REAL* dev_deferred_mm_diff) const
    {
        check(bddmma_get_solver_costs(h_, dev_lo, dev_hi, dev_deferred_mm_diff, 1));
    }
    using SOLVER_COSTS_VECS = std::tuple<std::vector<REAL>, std::vector<REAL>, std::vector<REAL>>;
    SOLVER_COSTS_VECS get_solver_costs() const
    {
        const size_t L = nr_layers();
        SOLVER_COSTS_VECS c{std::vector<REAL>(L), std::vector<REAL>(L), std::vector<REAL>(L)};
        check(bddmma_get_solver_costs(h_, std::get<0>(c).data(), std::get<1>(c).data(), std::get<2>(c).data(), 0));
        return c;
    }
    void set_solver_costs(const REAL* dev_lo, const REAL* dev_hi, const REAL* dev_deferred_mm_diff)
    {
        check(bddmma_set_solver_costs(h_, dev_lo, dev_hi, dev_deferred_mm_diff, 1));
    }
    void set_solver_costs(const SOLVER_COSTS_VECS& c)
    {
        if (std::get<0>(c).size() != nr_layers() || std::get<1>(c).size() != nr_layers() || std::get<2>(c).size() != nr_layers())
            throw std::runtime_error("bdd_hip_parallel_mma: set_solver_costs needs nr_layers() entries per vector");
        check(bddmma_set_solver_costs(h_, std::get<0>(c).data(), std::get<1>(c).data(), std::get<2>(c).data(), 0));
    }

    // ---- sweeps and bounds
    void forward_run() { check(bddmma_forward_run(h_)); }
    void backward_run() { check(bddmma_backward_run(h_)); }
    double lower_bound()
    {
        double lb;
        check(bddmma_lower_bound(h_, &lb));
        return lb;
    }
    // lower_bound_per_bdd(device_ptr), bdd_cuda_base.h:70 (bdd_cuda_base.cu:1253-1259): nr_bdds() values
    void lower_bound_per_bdd(REAL* dev_lb_per_bdd) { check(bddmma_lower_bound_per_bdd(h_, dev_lb_per_bdd, 1)); }
    std::vector<REAL> lower_bound_per_bdd_host()
    {
        std::vector<REAL> lb(nr_bdds());
        check(bddmma_lower_bound_per_bdd(h_, lb.data(), 0));
        return lb;
    }

    // ---- parallel mma (bdd_cuda_parallel_mma.cu:142-153, 207-257, 301-346, 410-430)
    void iteration(const REAL omega = 0.5) { check(bddmma_iteration(h_, omega)); }
    void forward_mm(const REAL omega, std::vector<REAL>& delta_lo_hi) { check(bddmma_forward_mm(h_, omega, delta_lo_hi.data(), 0)); }
    void backward_mm(const REAL omega, std::vector<REAL>& delta_lo_hi) { check(bddmma_backward_mm(h_, omega, delta_lo_hi.data(), 0)); }
    void forward_mm(const REAL omega, REAL* dev_delta_lo_hi) { check(bddmma_forward_mm(h_, omega, dev_delta_lo_hi, 1)); }
    void backward_mm(const REAL omega, REAL* dev_delta_lo_hi) { check(bddmma_backward_mm(h_, omega, dev_delta_lo_hi, 1)); }
    void normalize_delta(REAL* dev_delta_lo_hi) const { check(bddmma_normalize_delta(h_, dev_delta_lo_hi, 1)); }
    void distribute_delta() { check(bddmma_distribute_delta(h_)); }

    // learned iterations (bdd_cuda_learned_mma.h: iterations; include/bdd_mma.h: bddmma_learned_iterations): device pointers, as the
    // reference's thrust::device_ptr arguments; dist_weights REAL[nr_layers], sol_avg REAL[nr_layers], the two lb averages REAL[nr_bdds]
    // (may be null when compute_history_for_itr = 0).  Returns the number of iterations run.
    // dev_omega_vec (REAL[nr_layers], same order; include/bdd_mma.h: bddmma_learned_iterations_omega_vec): one omega per layer in place of
    // omega, as the reference's omega_vec
    int iterations(const REAL* dev_dist_weights, const int num_itr, const REAL omega, const double improvement_slope = 1e-6,
                   REAL* dev_sol_avg = nullptr, REAL* dev_lb_first_diff_avg = nullptr, REAL* dev_lb_second_diff_avg = nullptr,
                   const int compute_history_for_itr = 0, const REAL history_avg_beta = 0.9, const REAL* dev_omega_vec = nullptr)
    {
        uint64_t done = 0;
        if (dev_omega_vec) {
            check(bddmma_learned_iterations_omega_vec(h_, dev_dist_weights, 1, (uint64_t)std::max(num_itr, 0), dev_omega_vec, 1, improvement_slope,
                                                      dev_sol_avg, dev_lb_first_diff_avg, dev_lb_second_diff_avg,
                                                      (uint64_t)std::max(compute_history_for_itr, 0), history_avg_beta, 1, &done));
            return (int)done;
        }
        check(bddmma_learned_iterations(h_, dev_dist_weights, 1, (uint64_t)std::max(num_itr, 0), omega, improvement_slope, dev_sol_avg,
                                        dev_lb_first_diff_avg, dev_lb_second_diff_avg, (uint64_t)std::max(compute_history_for_itr, 0),
                                        history_avg_beta, 1, &done));
        return (int)done;
    }
    // host weights without a history (dist_weights.size() must be nr_layers())
    int iterations(const std::vector<REAL>& dist_weights, const int num_itr, const REAL omega, const double improvement_slope = 1e-6)
    {
        if (dist_weights.size() != nr_layers()) throw std::runtime_error("bdd_mma: dist_weights must hold nr_layers() values");
        uint64_t done = 0;
        check(bddmma_learned_iterations(h_, dist_weights.data(), 0, (uint64_t)std::max(num_itr, 0), omega, improvement_slope, nullptr, nullptr,
                                        nullptr, 0, 0.9, 0, &done));
        return (int)done;
    }
    // host weights with a history (dist_weights.size() must be nr_layers(); the outputs are resized when a history is asked for)
    int iterations(const std::vector<REAL>& dist_weights, const int num_itr, const REAL omega, const double improvement_slope,
                   std::vector<REAL>& sol_avg, std::vector<REAL>& lb_first_diff_avg, std::vector<REAL>& lb_second_diff_avg,
                   const int compute_history_for_itr = 0, const REAL history_avg_beta = 0.9)
    {
        if (dist_weights.size() != nr_layers()) throw std::runtime_error("bdd_mma: dist_weights must hold nr_layers() values");
        if (compute_history_for_itr > 0) {
            sol_avg.resize(nr_layers());
            lb_first_diff_avg.resize(nr_bdds());
            lb_second_diff_avg.resize(nr_bdds());
        }
        uint64_t done = 0;
        check(bddmma_learned_iterations(h_, dist_weights.data(), 0, (uint64_t)std::max(num_itr, 0), omega, improvement_slope, sol_avg.data(),
                                        lb_first_diff_avg.data(), lb_second_diff_avg.data(), (uint64_t)std::max(compute_history_for_itr, 0),
                                        history_avg_beta, 0, &done));
        return (int)done;
    }
    // the same with one omega per layer, last as in the reference (bdd_cuda_learned_mma.h: iterations(..., omega_vec); include/bdd_mma.h:
    // bddmma_learned_iterations_omega_vec): REAL[nr_layers] in the order of dist_weights; omega is then not used
    int iterations(const std::vector<REAL>& dist_weights, const int num_itr, const REAL omega, const double improvement_slope,
                   const std::vector<REAL>& omega_vec)
    {
        std::vector<REAL> none;
        return iterations(dist_weights, num_itr, omega, improvement_slope, none, none, none, 0, REAL(0.9), omega_vec);
    }
    int iterations(const std::vector<REAL>& dist_weights, const int num_itr, const REAL /*omega*/, const double improvement_slope,
                   std::vector<REAL>& sol_avg, std::vector<REAL>& lb_first_diff_avg, std::vector<REAL>& lb_second_diff_avg,
                   const int compute_history_for_itr, const REAL history_avg_beta, const std::vector<REAL>& omega_vec)
    {
        if (dist_weights.size() != nr_layers()) throw std::runtime_error("bdd_mma: dist_weights must hold nr_layers() values");
        if (omega_vec.size() != nr_layers()) throw std::runtime_error("bdd_mma: omega_vec must hold nr_layers() values");
        if (compute_history_for_itr > 0) {
            sol_avg.resize(nr_layers());
            lb_first_diff_avg.resize(nr_bdds());
            lb_second_diff_avg.resize(nr_bdds());
        }
        uint64_t done = 0;
        check(bddmma_learned_iterations_omega_vec(h_, dist_weights.data(), 0, (uint64_t)std::max(num_itr, 0), omega_vec.data(), 0, improvement_slope,
                                                  sol_avg.data(), lb_first_diff_avg.data(), lb_second_diff_avg.data(),
                                                  (uint64_t)std::max(compute_history_for_itr, 0), history_avg_beta, 0, &done));
        return (int)done;
    }
    // 1 / nr_bdds(variable) per layer, public layer order (the weights with which iterations(...) above is iteration())
    std::vector<REAL> isotropic_dist_weights()
    {
        std::vector<REAL> w(nr_layers());
        check(bddmma_isotropic_dist_weights(h_, w.data(), 0));
        return w;
    }
    void isotropic_dist_weights(REAL* dev_out) { check(bddmma_isotropic_dist_weights(h_, dev_out, 1)); }

    // ---- min-marginals [var][bdd] -> {mm0, mm1} (bdd_cuda_base.cu:751-786)
    std::vector<std::vector<std::array<double, 2>>> min_marginals()
    {
        const size_t L = nr_layers();
        std::vector<int32_t> var(L);
        std::vector<REAL> m0(L), m1(L);
        check(bddmma_min_marginals(h_, 1, var.data(), m0.data(), m1.data(), 0));
        std::vector<std::vector<std::array<double, 2>>> out(nr_variables());
        for (size_t k = 0; k < L; ++k) out[var[k]].push_back({double(m0[k]), double(m1[k])});
        return out;
    }
    // min_marginals_cuda(get_sorted), bdd_cuda_base.h:84 (bdd_cuda_base.cu:716-749): (primal variable, mm_lo, mm_hi) per dual variable — what
    // incremental_mm_agreement_rounding_cuda.cu:262-362 consumes; sorted by variable (then BDD) or in the solver's layer order.
    // Device buffers of nr_layers() entries each, owned by the caller ...
    void min_marginals_cuda(int32_t* dev_var, REAL* dev_mm_lo, REAL* dev_mm_hi, bool get_sorted = true)
    {
        check(bddmma_min_marginals(h_, get_sorted ? 1 : 0, dev_var, dev_mm_lo, dev_mm_hi, 1));
    }
    // ... or as host vectors
    std::tuple<std::vector<int>, std::vector<REAL>, std::vector<REAL>> min_marginals_cuda(bool get_sorted = true)
    {
        const size_t L = nr_layers();
        std::vector<int32_t> var(L);
        std::vector<REAL> m0(L), m1(L);
        check(bddmma_min_marginals(h_, get_sorted ? 1 : 0, var.data(), m0.data(), m1.data(), 0));
        return {std::vector<int>(var.begin(), var.end()), std::move(m0), std::move(m1)};
    }
    // sum_marginals_cuda(get_sorted, get_log_probs), bdd_cuda_base.h (bdd_cuda_base.cu:788-1025): (primal variable, sm_lo, sm_hi) per dual
    // variable — log of the summed exp(-cost) over the root-to-top paths through the layer's lo / hi arcs (get_log_probs = false: the sums).
    // Device buffers of nr_layers() entries each, owned by the caller (dev_var may be null) ...
    void sum_marginals_cuda(int32_t* dev_var, REAL* dev_sm_lo, REAL* dev_sm_hi, bool get_sorted = true, bool get_log_probs = true)
    {
        check(bddmma_sum_marginals(h_, get_sorted ? 1 : 0, get_log_probs ? 1 : 0, dev_var, dev_sm_lo, dev_sm_hi, 1));
    }
    // ... or as host vectors
    std::tuple<std::vector<int>, std::vector<REAL>, std::vector<REAL>> sum_marginals_cuda(bool get_sorted = true, bool get_log_probs = true)
    {
        const size_t L = nr_layers();
        std::vector<int32_t> var(L);
        std::vector<REAL> m0(L), m1(L);
        check(bddmma_sum_marginals(h_, get_sorted ? 1 : 0, get_log_probs ? 1 : 0, var.data(), m0.data(), m1.data(), 0));
        return {std::vector<int>(var.begin(), var.end()), std::move(m0), std::move(m1)};
    }
    // sum_marginals(get_log_probs) (bdd_cuda_base.cu:1066-1100): [variable][bdd] -> {sm_lo, sm_hi}, indexed like min_marginals()
    std::vector<std::vector<std::array<double, 2>>> sum_marginals(bool get_log_probs = true)
    {
        const size_t L = nr_layers();
        std::vector<int32_t> var(L);
        std::vector<REAL> m0(L), m1(L);
        check(bddmma_sum_marginals(h_, 1, get_log_probs ? 1 : 0, var.data(), m0.data(), m1.data(), 0));
        std::vector<std::vector<std::array<double, 2>>> out(nr_variables());
        for (size_t k = 0; k < L; ++k) out[var[k]].push_back({double(m0[k]), double(m1[k])});
        return out;
    }
    // smooth_solution_cuda(ptr) (bdd_cuda_base.cu:1050-1064): exp(sm_hi) / (exp(sm_lo) + exp(sm_hi)) per layer into a device buffer of
    // nr_layers() entries, the solver's layer order
    void smooth_solution_cuda(REAL* dev_smooth_sol) { check(bddmma_smooth_solution(h_, dev_smooth_sol, 1)); }
    std::vector<REAL> smooth_solution()   // the same as a host vector
    {
        std::vector<REAL> out(nr_layers());
        check(bddmma_smooth_solution(h_, out.data(), 0));
        return out;
    }
    // ---- the single-shot backward operators of bdd_cuda_learned_mma<REAL> (bdd_cuda_learned_mma.h:82-110); device pointers of nr_layers()
    // entries in the solver's layer order unless stated, owned by the caller; state contracts in include/bdd_mma.h (bddmma_grad_*)
    // grad_mm_diff_all_hops(incoming_grad_mm, grad_lo_cost_out, grad_hi_cost_out) (bdd_cuda_learned_mma.cu:623-1023)
    void grad_mm_diff_all_hops(const REAL* dev_grad_mm, REAL* dev_grad_lo_out, REAL* dev_grad_hi_out)
    {
        check(bddmma_grad_min_marginal_diff(h_, dev_grad_mm, dev_grad_lo_out, dev_grad_hi_out, 1));
    }
    // grad_lower_bound_per_bdd(grad_lb_per_bdd [nr_bdds()], grad_lo_cost_out, grad_hi_cost_out, account_for_constant) (:387-416); smooth: the
    // gradient of the smooth lower bound (grad_smooth_lower_bound_per_bdd of the reference's Python module)
    void grad_lower_bound_per_bdd(const REAL* dev_grad_lb_per_bdd, REAL* dev_grad_lo_out, REAL* dev_grad_hi_out, bool smooth = false)
    {
        check(bddmma_grad_lower_bound_per_bdd(h_, dev_grad_lb_per_bdd, dev_grad_lo_out, dev_grad_hi_out, smooth ? 1 : 0, 1));
    }
    // grad_distribute_delta(grad_lo_cost, grad_hi_cost, grad_deferred_mm_diff_out) (:1025-1065): refers to the last distribute_delta()
    void grad_distribute_delta(const REAL* dev_grad_lo, const REAL* dev_grad_hi, REAL* dev_grad_deferred_mm_out)
    {
        check(bddmma_grad_distribute_delta(h_, dev_grad_lo, dev_grad_hi, dev_grad_deferred_mm_out, 1));
    }
    // grad_cost_perturbation(grad_lo_cost, grad_hi_cost, grad_lo_pert_out, grad_hi_pert_out) (:1067-1187): outputs of nr_variables() entries
    void grad_cost_perturbation(const REAL* dev_grad_lo, const REAL* dev_grad_hi, REAL* dev_grad_lo_pert_out, REAL* dev_grad_hi_pert_out)
    {
        check(bddmma_grad_cost_perturbation(h_, dev_grad_lo, dev_grad_hi, dev_grad_lo_pert_out, dev_grad_hi_pert_out, 1));
    }
    // grad_iterations(dist_weights, grad_lo_cost, grad_hi_cost, grad_mm, grad_dist_weights_out, grad_omega, omega_scalar, track_grad_after_itr,
    // track_grad_for_num_itr, num_caches, omega_vec) (:308-385): device arrays; grad_lo / grad_hi / grad_mm in-out, grad_omega of one entry
    // (nr_layers() with omega_vec).  Contract: bddmma_grad_learned_iterations.
    void grad_iterations(const REAL* dev_dist_weights, REAL* dev_grad_lo, REAL* dev_grad_hi, REAL* dev_grad_mm, REAL* dev_grad_dist_weights_out,
                         REAL* dev_grad_omega, REAL omega_scalar, int track_grad_after_itr, int track_grad_for_num_itr, int num_caches,
                         const REAL* dev_omega_vec = nullptr)
    {
        if (track_grad_after_itr < 0 || track_grad_for_num_itr < 0 || num_caches < 0) throw std::invalid_argument("grad_iterations: negative count");
        check(bddmma_grad_learned_iterations(h_, dev_dist_weights, 1, (double)omega_scalar, dev_omega_vec, 1, dev_grad_lo, dev_grad_hi, dev_grad_mm,
                                             dev_grad_dist_weights_out, dev_grad_omega, (uint64_t)track_grad_after_itr, (uint64_t)track_grad_for_num_itr,
                                             (uint64_t)num_caches, 1));
    }
    // the same four on host vectors: {grad_lo, grad_hi} / grad_deferred_mm / {grad_lo_pert, grad_hi_pert}
    std::pair<std::vector<REAL>, std::vector<REAL>> grad_mm_diff_all_hops(const std::vector<REAL>& grad_mm)
    {
        if (grad_mm.size() != nr_layers()) throw std::invalid_argument("grad_mm_diff_all_hops: grad_mm must have nr_layers() entries");
        std::vector<REAL> lo(nr_layers()), hi(nr_layers());
        check(bddmma_grad_min_marginal_diff(h_, grad_mm.data(), lo.data(), hi.data(), 0));
        return {std::move(lo), std::move(hi)};
    }
    std::pair<std::vector<REAL>, std::vector<REAL>> grad_lower_bound_per_bdd(const std::vector<REAL>& grad_lb_per_bdd, bool smooth = false)
    {
        if (grad_lb_per_bdd.size() != nr_bdds()) throw std::invalid_argument("grad_lower_bound_per_bdd: grad_lb_per_bdd must have nr_bdds() entries");
        std::vector<REAL> lo(nr_layers()), hi(nr_layers());
        check(bddmma_grad_lower_bound_per_bdd(h_, grad_lb_per_bdd.data(), lo.data(), hi.data(), smooth ? 1 : 0, 0));
        return {std::move(lo), std::move(hi)};
    }
    std::vector<REAL> grad_distribute_delta(const std::vector<REAL>& grad_lo, const std::vector<REAL>& grad_hi)
    {
        if (grad_lo.size() != nr_layers() || grad_hi.size() != nr_layers()) throw std::invalid_argument("grad_distribute_delta: nr_layers() entries each");
        std::vector<REAL> out(nr_layers());
        check(bddmma_grad_distribute_delta(h_, grad_lo.data(), grad_hi.data(), out.data(), 0));
        return out;
    }
    std::pair<std::vector<REAL>, std::vector<REAL>> grad_cost_perturbation(const std::vector<REAL>& grad_lo, const std::vector<REAL>& grad_hi)
    {
        if (grad_lo.size() != nr_layers() || grad_hi.size() != nr_layers()) throw std::invalid_argument("grad_cost_perturbation: nr_layers() entries each");
        std::vector<REAL> lo(nr_variables()), hi(nr_variables());
        check(bddmma_grad_cost_perturbation(h_, grad_lo.data(), grad_hi.data(), lo.data(), hi.data(), 0));
        return {std::move(lo), std::move(hi)};
    }
    // two_dim_variable_array<REAL> bdds_solution() (bdd_cuda_base.cu:1204-1233): [variable][bdd] -> 0 / 1, the argmin path of every BDD,
    // BDDs of a variable in ascending order (primal_variable_sorting_order_, :379-391); nested vectors instead of two_dim_variable_array
    std::vector<std::vector<REAL>> bdds_solution()
    {
        const size_t L = nr_layers(), V = nr_variables();
        std::vector<char> sorted(L);
        check(bddmma_bdds_solution(h_, 1, sorted.data(), 0));
        std::vector<int32_t> n(V);
        check(bddmma_num_bdds_per_var(h_, n.data()));
        std::vector<std::vector<REAL>> out(V);
        size_t k = 0;
        for (size_t v = 0; v < V; ++v) {
            out[v].resize((size_t)n[v]);
            for (int32_t b = 0; b < n[v]; ++b, ++k) out[v][(size_t)b] = REAL(sorted[k]);
        }
        return out;
    }
    std::vector<char> bdds_solution_vec_host()
    {
        std::vector<char> s(nr_layers());
        check(bddmma_bdds_solution(h_, 0, s.data(), 0));
        return s;
    }

    // ---- L-BFGS support on device vectors (lbfgs.h:22-27)
    void net_solver_costs(REAL* dev_out) const { check(bddmma_net_solver_costs(h_, dev_out, 1)); }
    void bdds_solution_vec(char* dev_out) { check(bddmma_bdds_solution(h_, 0, dev_out, 1)); }
    void make_dual_feasible(REAL* dev_g) const { check(bddmma_make_dual_feasible(h_, dev_g, 1)); }
    void gradient_step(const REAL* dev_g, double step_size) { check(bddmma_gradient_step(h_, dev_g, step_size, 1)); }

    // cereal save / load of the reference (bdd_cuda_base.h:167-170, bdd_cuda_base.cu:1486-1550; pickled by bdd_cuda_parallel_mma_py.cu:15-38):
    // the archive is a file; it holds the device layout and the costs, load() rebuilds nothing
    void save(const std::string& path) const { check(bddmma_save(h_, path.c_str())); }
    static bdd_hip_parallel_mma load(const std::string& path, int device = 0)
    {
        bddmma_solver* h = nullptr;
        const int rc = bddmma_load(&h, device, path.c_str());
        if (rc != BDDMMA_OK) throw std::runtime_error(std::string("bdd_hip_parallel_mma: ") + bddmma_last_error(nullptr));
        if (bddmma_precision(h) != precision) {
            bddmma_destroy(h);
            throw std::runtime_error("bdd_hip_parallel_mma: the checkpoint was written by a solver of the other precision");
        }
        bdd_hip_parallel_mma s;
        s.h_ = h;
        return s;
    }
    // Ordering against another stream of the solver's device (a hipStream_t as void*; nullptr: the default stream), without the host waiting:
    // stream_wait — the solver's later work starts after everything queued on `hip_stream` so far; stream_signal — the reverse
    // (bddmma_stream_wait / bddmma_stream_signal).  For device vectors that another stream writes, reads or frees.
    void stream_wait(void* hip_stream) { check(bddmma_stream_wait(h_, hip_stream)); }
    void stream_signal(void* hip_stream) { check(bddmma_stream_signal(h_, hip_stream)); }
    bddmma_solver* handle() { return h_; }

   private:
    std::vector<uint64_t> per_hop(int (*f)(const bddmma_solver*, uint64_t*)) const
    {
        std::vector<uint64_t> n(nr_hops());
        check(f(h_, n.data()));
        return n;
    }
    void check(int rc) const { check(rc, h_); }
    static void check(int rc, const bddmma_solver* h)
    {
        if (rc != BDDMMA_OK) throw std::runtime_error(std::string("bdd_hip_parallel_mma: ") + bddmma_last_error(h));
    }
    bddmma_solver* h_ = nullptr;
};

// Solvers whose instances fit one workgroup each (fused_small()), run together: one workgroup per member in one launch instead of one
// launch per solver (include/bdd_mma.h: bddmma_batch_*).  The solvers are borrowed: they must outlive the batch and stay usable on their
// own between its calls; a call behaves as if it had been made on each member in turn.
template <typename REAL>
class bdd_hip_batch {
   public:
    explicit bdd_hip_batch(const std::vector<std::reference_wrapper<bdd_hip_parallel_mma<REAL>>>& solvers)
    {
        std::vector<bddmma_solver*> h;
        for (bdd_hip_parallel_mma<REAL>& s : solvers) {
            h.push_back(s.handle());
            nv_.push_back(bddmma_nr_variables(s.handle()));
        }
        if (bddmma_batch_create(&b_, h.data(), h.size()) != BDDMMA_OK) throw std::runtime_error(std::string("bdd_hip_batch: ") + bddmma_batch_last_error(nullptr));
    }
    ~bdd_hip_batch() { bddmma_batch_destroy(b_); }
    bdd_hip_batch(const bdd_hip_batch&) = delete;
    bdd_hip_batch& operator=(const bdd_hip_batch&) = delete;
    size_t size() const { return bddmma_batch_size(b_); }
    void iterations(const size_t n, const REAL omega = 0.5) { check(bddmma_batch_iterations(b_, omega, n)); }
    // learned_iterations(w_i, num_itr, omega, improvement_slope = 0) of every member i, or with omega_vec non-null its omega_vec form: the
    // members' REAL[nr_layers] one behind the other in the members' order, host vectors or (the _dev form) device pointers.  Every member
    // must be fused_small_learned() (include/bdd_mma.h: bddmma_learned_iterations_batch).
    void learned_iterations(const std::vector<REAL>& dist_weights, const size_t num_itr, const REAL omega = 0.5, const std::vector<REAL>* omega_vec = nullptr)
    {
        check(bddmma_learned_iterations_batch(b_, dist_weights.data(), omega_vec ? omega_vec->data() : nullptr, omega, num_itr, 0));
    }
    void learned_iterations_dev(const REAL* dev_dist_weights, const size_t num_itr, const REAL omega = 0.5, const REAL* dev_omega_vec = nullptr)
    {
        check(bddmma_learned_iterations_batch(b_, dev_dist_weights, dev_omega_vec, omega, num_itr, 1));
    }
    // ... with the history of the last min(num_itr, compute_history_for_itr) iterations, computed inside the members' workgroups: sol_avg holds
    // the members' REAL[nr_layers], lb_first_diff_avg / lb_second_diff_avg the members' REAL[nr_bdds], one behind the other; updated in
    // place (the caller sizes them; an entry the history does not reach keeps its content).  Every member must be fused_small_history()
    // (include/bdd_mma.h: bddmma_learned_iterations_history_batch).
    void learned_iterations(const std::vector<REAL>& dist_weights, const size_t num_itr, const REAL omega, const std::vector<REAL>* omega_vec,
                            const size_t compute_history_for_itr, const REAL history_avg_beta, std::vector<REAL>& sol_avg, std::vector<REAL>& lb_first_diff_avg,
                            std::vector<REAL>& lb_second_diff_avg)
    {
        check(bddmma_learned_iterations_history_batch(b_, dist_weights.data(), omega_vec ? omega_vec->data() : nullptr, omega, num_itr, sol_avg.data(),
                                                      lb_first_diff_avg.data(), lb_second_diff_avg.data(), compute_history_for_itr, history_avg_beta, 0));
    }
    void learned_iterations_dev(const REAL* dev_dist_weights, const size_t num_itr, const REAL omega, const REAL* dev_omega_vec,
                                const size_t compute_history_for_itr, const REAL history_avg_beta, REAL* dev_sol_avg, REAL* dev_lb_first_diff_avg,
                                REAL* dev_lb_second_diff_avg)
    {
        check(bddmma_learned_iterations_history_batch(b_, dev_dist_weights, dev_omega_vec, omega, num_itr, dev_sol_avg, dev_lb_first_diff_avg,
                                                      dev_lb_second_diff_avg, compute_history_for_itr, history_avg_beta, 1));
    }
    // ... and with the stopping rule of the per-solver learned_iterations (improvement_slope > 0) inside the members' workgroups: returns the
    // members' counts of iterations run.  The history arrays may be null / empty with compute_history_for_itr == 0.  Every member must be
    // fused_small_stop() (include/bdd_mma.h: bddmma_learned_iterations_stop_batch).
    std::vector<size_t> learned_iterations_stopping(const std::vector<REAL>& dist_weights, const size_t num_itr, const REAL omega, const double improvement_slope,
                                                    const std::vector<REAL>* omega_vec = nullptr, const size_t compute_history_for_itr = 0,
                                                    const REAL history_avg_beta = 0.9, std::vector<REAL>* sol_avg = nullptr,
                                                    std::vector<REAL>* lb_first_diff_avg = nullptr, std::vector<REAL>* lb_second_diff_avg = nullptr)
    {
        std::vector<uint64_t> done(size());
        check(bddmma_learned_iterations_stop_batch(b_, dist_weights.data(), omega_vec ? omega_vec->data() : nullptr, omega, num_itr, improvement_slope,
                                                   sol_avg ? sol_avg->data() : nullptr, lb_first_diff_avg ? lb_first_diff_avg->data() : nullptr,
                                                   lb_second_diff_avg ? lb_second_diff_avg->data() : nullptr, compute_history_for_itr, history_avg_beta, 0,
                                                   done.data()));
        return std::vector<size_t>(done.begin(), done.end());
    }
    std::vector<size_t> learned_iterations_stopping_dev(const REAL* dev_dist_weights, const size_t num_itr, const REAL omega, const double improvement_slope,
                                                        const REAL* dev_omega_vec = nullptr, const size_t compute_history_for_itr = 0,
                                                        const REAL history_avg_beta = 0.9, REAL* dev_sol_avg = nullptr, REAL* dev_lb_first_diff_avg = nullptr,
                                                        REAL* dev_lb_second_diff_avg = nullptr)
    {
        std::vector<uint64_t> done(size());
        check(bddmma_learned_iterations_stop_batch(b_, dev_dist_weights, dev_omega_vec, omega, num_itr, improvement_slope, dev_sol_avg, dev_lb_first_diff_avg,
                                                   dev_lb_second_diff_avg, compute_history_for_itr, history_avg_beta, 1, done.data()));
        return std::vector<size_t>(done.begin(), done.end());
    }
    // grad_iterations(...) of every member with its part of every device array (bdd_hip_parallel_mma::grad_iterations; the members' arrays
    // one behind the other), one workgroup per member: dev_grad_omega has size() entries, the concatenated per-layer array with
    // dev_omega_vec.  Contract: bddmma_grad_learned_iterations_batch.
    void grad_iterations_dev(const REAL* dev_dist_weights, REAL* dev_grad_lo, REAL* dev_grad_hi, REAL* dev_grad_mm, REAL* dev_grad_dist_weights_out,
                             REAL* dev_grad_omega, REAL omega_scalar, int track_grad_after_itr, int track_grad_for_num_itr, int num_caches,
                             const REAL* dev_omega_vec = nullptr)
    {
        if (track_grad_after_itr < 0 || track_grad_for_num_itr < 0 || num_caches < 0) throw std::invalid_argument("grad_iterations: negative count");
        check(bddmma_grad_learned_iterations_batch(b_, dev_dist_weights, dev_omega_vec, (double)omega_scalar, dev_grad_lo, dev_grad_hi, dev_grad_mm,
                                                   dev_grad_dist_weights_out, dev_grad_omega, (uint64_t)track_grad_after_itr,
                                                   (uint64_t)track_grad_for_num_itr, (uint64_t)num_caches, 1));
    }
    // ... with every member's own two counts (size() entries each): the backward of learned_iterations_stopping_dev, whose members stop at
    // different iterations.  A member whose tracked count is 0 is left untouched.  Contract: bddmma_grad_learned_iterations_counts_batch.
    void grad_iterations_counts_dev(const REAL* dev_dist_weights, REAL* dev_grad_lo, REAL* dev_grad_hi, REAL* dev_grad_mm, REAL* dev_grad_dist_weights_out,
                                    REAL* dev_grad_omega, REAL omega_scalar, const std::vector<size_t>& track_grad_after_itr,
                                    const std::vector<size_t>& track_grad_for_num_itr, int num_caches, const REAL* dev_omega_vec = nullptr)
    {
        if (track_grad_after_itr.size() != size() || track_grad_for_num_itr.size() != size())
            throw std::invalid_argument("grad_iterations_counts: one count of each kind per member");
        if (num_caches < 0) throw std::invalid_argument("grad_iterations_counts: negative count");
        const std::vector<uint64_t> after(track_grad_after_itr.begin(), track_grad_after_itr.end()), tracked(track_grad_for_num_itr.begin(), track_grad_for_num_itr.end());
        check(bddmma_grad_learned_iterations_counts_batch(b_, dev_dist_weights, dev_omega_vec, (double)omega_scalar, dev_grad_lo, dev_grad_hi, dev_grad_mm,
                                                          dev_grad_dist_weights_out, dev_grad_omega, after.data(), tracked.data(), (uint64_t)num_caches, 1));
    }
    // set_solver_costs followed by backward_run / get_solver_costs of every member in one launch each, with the members' REAL[nr_layers]
    // one behind the other in the members' order.  Device pointers as in bdd_hip_parallel_mma (any of them may be null: that part is
    // skipped; the host does not wait), or host vectors (empty: skipped).  Contract: bddmma_set_solver_costs_batch / bddmma_get_solver_costs_batch.
    void set_solver_costs(const REAL* dev_lo, const REAL* dev_hi, const REAL* dev_deferred_mm_diff)
    {
        check(bddmma_set_solver_costs_batch(b_, dev_lo, dev_hi, dev_deferred_mm_diff, 1));
    }
    using SOLVER_COSTS_VECS = std::tuple<std::vector<REAL>, std::vector<REAL>, std::vector<REAL>>;
    void set_solver_costs(const SOLVER_COSTS_VECS& c)
    {
        auto p = [](const std::vector<REAL>& v) { return v.empty() ? nullptr : v.data(); };
        check(bddmma_set_solver_costs_batch(b_, p(std::get<0>(c)), p(std::get<1>(c)), p(std::get<2>(c)), 0));
    }
    void get_solver_costs(REAL* dev_lo, REAL* dev_hi, REAL* dev_deferred_mm_diff) const
    {
        check(bddmma_get_solver_costs_batch(b_, dev_lo, dev_hi, dev_deferred_mm_diff, 1));
    }
    SOLVER_COSTS_VECS get_solver_costs(const size_t total_layers) const
    {
        SOLVER_COSTS_VECS c{std::vector<REAL>(total_layers), std::vector<REAL>(total_layers), std::vector<REAL>(total_layers)};
        check(bddmma_get_solver_costs_batch(b_, std::get<0>(c).data(), std::get<1>(c).data(), std::get<2>(c).data(), 0));
        return c;
    }
    // lower_bound_per_bdd / grad_lower_bound_per_bdd (the arg-min path's, not the smooth one) / distribute_delta of every member in one launch
    // per kernel instantiation present: per-BDD arrays are the members' REAL[nr_bdds], layer arrays the members' REAL[nr_layers], one behind
    // the other in the members' order.  Device pointers (the host does not wait) or host vectors.  Contract:
    // bddmma_lower_bound_per_bdd_batch, bddmma_grad_lower_bound_per_bdd_batch, bddmma_distribute_delta_batch.
    void lower_bound_per_bdd(REAL* dev_lb_per_bdd) { check(bddmma_lower_bound_per_bdd_batch(b_, dev_lb_per_bdd, 1)); }
    std::vector<REAL> lower_bound_per_bdd_host(const size_t total_bdds)
    {
        std::vector<REAL> lb(total_bdds);
        check(bddmma_lower_bound_per_bdd_batch(b_, lb.data(), 0));
        return lb;
    }
    void grad_lower_bound_per_bdd(const REAL* dev_grad_lb_per_bdd, REAL* dev_grad_lo_out, REAL* dev_grad_hi_out)
    {
        check(bddmma_grad_lower_bound_per_bdd_batch(b_, dev_grad_lb_per_bdd, dev_grad_lo_out, dev_grad_hi_out, 1));
    }
    std::pair<std::vector<REAL>, std::vector<REAL>> grad_lower_bound_per_bdd(const std::vector<REAL>& grad_lb_per_bdd, const size_t total_layers)
    {
        std::vector<REAL> lo(total_layers), hi(total_layers);
        check(bddmma_grad_lower_bound_per_bdd_batch(b_, grad_lb_per_bdd.data(), lo.data(), hi.data(), 0));
        return {std::move(lo), std::move(hi)};
    }
    void distribute_delta() { check(bddmma_distribute_delta_batch(b_)); }
    // min_marginal_diff / grad_mm_diff_all_hops of every member, one workgroup per member: every array is the members' REAL[nr_layers], one
    // behind the other in the members' order.  Device pointers (the host does not wait) or host vectors.  Contract:
    // bddmma_min_marginal_diff_batch, bddmma_grad_min_marginal_diff_batch.
    void min_marginal_diff(REAL* dev_mm_diff) { check(bddmma_min_marginal_diff_batch(b_, dev_mm_diff, 1)); }
    std::vector<REAL> min_marginal_diff_host(const size_t total_layers)
    {
        std::vector<REAL> mm(total_layers);
        check(bddmma_min_marginal_diff_batch(b_, mm.data(), 0));
        return mm;
    }
    void grad_mm_diff_all_hops(const REAL* dev_grad_mm, REAL* dev_grad_lo_out, REAL* dev_grad_hi_out)
    {
        check(bddmma_grad_min_marginal_diff_batch(b_, dev_grad_mm, dev_grad_lo_out, dev_grad_hi_out, 1));
    }
    std::pair<std::vector<REAL>, std::vector<REAL>> grad_mm_diff_all_hops(const std::vector<REAL>& grad_mm)
    {
        std::vector<REAL> lo(grad_mm.size()), hi(grad_mm.size());
        check(bddmma_grad_min_marginal_diff_batch(b_, grad_mm.data(), lo.data(), hi.data(), 0));
        return {std::move(lo), std::move(hi)};
    }
    // sum_marginals_cuda (unsorted layer order, no variable output) / smooth_solution_per_bdd / grad_lower_bound_per_bdd(.., smooth = true)
    // of every member, one workgroup per member: layer arrays are the members' REAL[nr_layers], grad_lb_per_bdd the members' REAL[nr_bdds],
    // one behind the other in the members' order.  Device pointers (the host does not wait) or host vectors.  Contract:
    // bddmma_sum_marginals_batch, bddmma_smooth_solution_batch, bddmma_grad_smooth_lower_bound_per_bdd_batch.
    void sum_marginals_cuda(const bool get_log_probs, REAL* dev_sm_lo, REAL* dev_sm_hi)
    {
        check(bddmma_sum_marginals_batch(b_, get_log_probs ? 1 : 0, dev_sm_lo, dev_sm_hi, 1));
    }
    std::pair<std::vector<REAL>, std::vector<REAL>> sum_marginals_host(const bool get_log_probs, const size_t total_layers)
    {
        std::vector<REAL> lo(total_layers), hi(total_layers);
        check(bddmma_sum_marginals_batch(b_, get_log_probs ? 1 : 0, lo.data(), hi.data(), 0));
        return {std::move(lo), std::move(hi)};
    }
    void smooth_solution_per_bdd(REAL* dev_out) { check(bddmma_smooth_solution_batch(b_, dev_out, 1)); }
    std::vector<REAL> smooth_solution_per_bdd_host(const size_t total_layers)
    {
        std::vector<REAL> x(total_layers);
        check(bddmma_smooth_solution_batch(b_, x.data(), 0));
        return x;
    }
    void grad_smooth_lower_bound_per_bdd(const REAL* dev_grad_lb_per_bdd, REAL* dev_grad_lo_out, REAL* dev_grad_hi_out)
    {
        check(bddmma_grad_smooth_lower_bound_per_bdd_batch(b_, dev_grad_lb_per_bdd, dev_grad_lo_out, dev_grad_hi_out, 1));
    }
    std::pair<std::vector<REAL>, std::vector<REAL>> grad_smooth_lower_bound_per_bdd(const std::vector<REAL>& grad_lb_per_bdd, const size_t total_layers)
    {
        std::vector<REAL> lo(total_layers), hi(total_layers);
        check(bddmma_grad_smooth_lower_bound_per_bdd_batch(b_, grad_lb_per_bdd.data(), lo.data(), hi.data(), 0));
        return {std::move(lo), std::move(hi)};
    }
    // incremental_mm_agreement_rounding(...) of every member (not verbose), every round one workgroup per member: member i's solution, empty
    // where none was found.  rounds (may be null): the index of the round in which each member's agreement was seen, num_rounds where none
    // was.  Contract: bddmma_incremental_mm_agreement_rounding_batch.
    std::vector<std::vector<char>> incremental_mm_agreement_rounding(const double init_delta, const double delta_growth_rate, const size_t num_itr_lb,
                                                                      const size_t num_rounds = 500, const uint32_t seed = 0, std::vector<uint64_t>* rounds = nullptr)
    {
        size_t total = 0;
        for (const size_t v : nv_) total += v;
        std::vector<char> sol(total > 0 ? total : 1);
        std::vector<int> found(size());
        if (rounds) rounds->assign(size(), 0);
        check(bddmma_incremental_mm_agreement_rounding_batch(b_, init_delta, delta_growth_rate, num_itr_lb, num_rounds, seed, sol.data(), found.data(),
                                                             rounds ? rounds->data() : nullptr));
        std::vector<std::vector<char>> out(size());
        size_t at = 0;
        for (size_t i = 0; i < out.size(); ++i) {
            if (found[i]) out[i].assign(sol.begin() + at, sol.begin() + at + nv_[i]);
            at += nv_[i];
        }
        return out;
    }
    // bdds_solution_vec / update_costs / grad_cost_perturbation of every member in one launch each: layer arrays are the members'
    // [nr_layers], per-variable arrays the members' [nr_variables], one behind the other in the members' order.  Device pointers (the host
    // does not wait) or host vectors; a null (device) or empty (host) cost vector leaves that side of every member's costs as it is.
    // Contract: bddmma_bdds_solution_batch, bddmma_update_costs_batch, bddmma_grad_cost_perturbation_batch.
    void bdds_solution_vec(char* dev_out) { check(bddmma_bdds_solution_batch(b_, dev_out, 1)); }
    std::vector<char> bdds_solution_vec_host(const size_t total_layers)
    {
        std::vector<char> sol(total_layers > 0 ? total_layers : 1);
        check(bddmma_bdds_solution_batch(b_, sol.data(), 0));
        sol.resize(total_layers);
        return sol;
    }
    void update_costs(const REAL* dev_cost_delta_0, const REAL* dev_cost_delta_1)
    {
        check(bddmma_update_costs_batch(b_, dev_cost_delta_0, dev_cost_delta_1, sizeof(REAL) == 8 ? BDDMMA_F64 : BDDMMA_F32, 1));
    }
    template <typename COST>
    void update_costs(const std::vector<COST>& cost_delta_0, const std::vector<COST>& cost_delta_1)
    {
        static_assert(std::is_same<COST, float>::value || std::is_same<COST, double>::value, "update_costs: float or double vectors");
        size_t total = 0;
        for (const size_t v : nv_) total += v;
        if ((!cost_delta_0.empty() && cost_delta_0.size() != total) || (!cost_delta_1.empty() && cost_delta_1.size() != total))
            throw std::invalid_argument("bdd_hip_batch::update_costs: a vector holds the members' nr_variables() entries, or none");
        check(bddmma_update_costs_batch(b_, cost_delta_0.empty() ? nullptr : cost_delta_0.data(), cost_delta_1.empty() ? nullptr : cost_delta_1.data(),
                                        sizeof(COST) == 8 ? BDDMMA_F64 : BDDMMA_F32, 0));
    }
    void grad_cost_perturbation(const REAL* dev_grad_lo, const REAL* dev_grad_hi, REAL* dev_grad_lo_pert_out, REAL* dev_grad_hi_pert_out)
    {
        check(bddmma_grad_cost_perturbation_batch(b_, dev_grad_lo, dev_grad_hi, dev_grad_lo_pert_out, dev_grad_hi_pert_out, 1));
    }
    std::pair<std::vector<REAL>, std::vector<REAL>> grad_cost_perturbation(const std::vector<REAL>& grad_lo, const std::vector<REAL>& grad_hi)
    {
        if (grad_lo.size() != grad_hi.size()) throw std::invalid_argument("bdd_hip_batch::grad_cost_perturbation: the members' nr_layers() entries each");
        size_t total = 0;
        for (const size_t v : nv_) total += v;
        std::vector<REAL> lo(total > 0 ? total : 1), hi(total > 0 ? total : 1);
        check(bddmma_grad_cost_perturbation_batch(b_, grad_lo.data(), grad_hi.data(), lo.data(), hi.data(), 0));
        lo.resize(total);
        hi.resize(total);
        return {std::move(lo), std::move(hi)};
    }
    // stream_wait — the batch's later calls start after everything queued on `hip_stream` so far; stream_signal — the reverse
    // (bddmma_stream_wait_batch / bddmma_stream_signal_batch)
    void stream_wait(void* hip_stream) { check(bddmma_stream_wait_batch(b_, hip_stream)); }
    void stream_signal(void* hip_stream) { check(bddmma_stream_signal_batch(b_, hip_stream)); }
    std::vector<bddmma_run_result> run_solver(const size_t max_iter = 1000, const double tolerance = 1e-6, const double improvement_slope = 1e-9,
                                              const double time_limit = 3600.0)
    {
        std::vector<bddmma_run_result> res(size());
        check(bddmma_batch_run_solver(b_, max_iter, tolerance, improvement_slope, time_limit, res.data()));
        return res;
    }
    std::vector<double> lower_bounds()
    {
        std::vector<double> lb(size());
        check(bddmma_batch_lower_bounds(b_, lb.data()));
        return lb;
    }
    // ... into the caller's device array (double[size()]) on the batch's stream; the host does not wait (bddmma_lower_bound_batch)
    void lower_bounds(double* out_device) { check(bddmma_lower_bound_batch(b_, out_device, 1)); }
    bddmma_batch* handle() { return b_; }

   private:
    void check(int rc) const
    {
        if (rc != BDDMMA_OK) throw std::runtime_error(std::string("bdd_hip_batch: ") + bddmma_batch_last_error(b_));
    }
    bddmma_batch* b_ = nullptr;
    std::vector<size_t> nv_;   // the members' nr_variables()
};

// lbfgs<bdd_cuda_parallel_mma<REAL>, ...> (include/bdd_solver/lbfgs.h:35-111) over the HIP solver.
template <typename REAL>
class bdd_hip_lbfgs_mma {
   public:
    bdd_hip_lbfgs_mma(bdd_hip_parallel_mma<REAL>&& s, const bddmma_lbfgs_params* p = nullptr) : solver_(std::move(s))
    {
        if (bddmma_lbfgs_create(&l_, solver_.handle(), p) != BDDMMA_OK)
            throw std::runtime_error(std::string("bdd_hip_lbfgs_mma: ") + bddmma_last_error(solver_.handle()));
    }
    ~bdd_hip_lbfgs_mma() { bddmma_lbfgs_destroy(l_); }
    bdd_hip_lbfgs_mma(const bdd_hip_lbfgs_mma&) = delete;
    void iteration()
    {
        if (bddmma_lbfgs_iteration(l_) != BDDMMA_OK)
            throw std::runtime_error(std::string("bdd_hip_lbfgs_mma: ") + bddmma_last_error(solver_.handle()));
    }
    double lower_bound() { return solver_.lower_bound(); }
    bdd_hip_parallel_mma<REAL>& solver() { return solver_; }
    bddmma_lbfgs* lbfgs_handle() { return l_; }

   private:
    bdd_hip_parallel_mma<REAL> solver_;
    bddmma_lbfgs* l_ = nullptr;
};

// ---------------------------------------------------------------------------------------------------------
// The two CUDA-free façades the reference ships for embedding the GPU solver in other code
// (include/bdd_cuda.h:9-31 `bdd_cuda<REAL>`, include/bdd_lbfgs_cuda_mma.h:9-36 `bdd_lbfgs_cuda_mma<REAL>`; their
// implementations throw "not compiled with CUDA support" without CUDA, src/bdd_cuda.cpp:27,38).  Same public
// members, same argument meaning; move-only.  min_marginals() returns [variable][bdd] -> {mm0, mm1} as nested vectors
// (the reference's two_dim_variable_array has the same indexing).
template <typename REAL>
class bdd_hip {
   public:
    template <typename BDD_COLLECTION>
    explicit bdd_hip(const BDD_COLLECTION& bdd_col) : s_(bdd_col)
    {
    }
    template <typename BDD_COLLECTION, typename ITERATOR>
    bdd_hip(const BDD_COLLECTION& bdd_col, ITERATOR cost_begin, ITERATOR cost_end) : s_(bdd_col)
    {
        update_costs(cost_begin, cost_begin, cost_begin, cost_end);  // as bdd_cuda.h:36-41
    }
    bdd_hip(bdd_hip&&) = default;
    bdd_hip& operator=(bdd_hip&&) = default;

    template <typename ITERATOR>
    void update_costs(ITERATOR cost_lo_begin, ITERATOR cost_lo_end, ITERATOR cost_hi_begin, ITERATOR cost_hi_end)
    {
        s_.update_costs(std::vector<REAL>(cost_lo_begin, cost_lo_end), std::vector<REAL>(cost_hi_begin, cost_hi_end));
    }
    double lower_bound() { return s_.lower_bound(); }
    size_t nr_variables() const { return s_.nr_variables(); }
    std::vector<std::vector<std::array<double, 2>>> min_marginals() { return s_.min_marginals(); }
    void iteration() { s_.iteration(); }
    void backward_run() { s_.backward_run(); }
    // incremental_mm_agreement_rounding_cuda (incremental_mm_agreement_rounding_cuda.cu:333-372); empty: no solution found
    std::vector<char> incremental_mm_agreement_rounding(const double init_delta, const double delta_growth_rate, const int num_itr_lb,
                                                        const int num_rounds = 500)
    {
        return round(s_.handle(), nullptr, init_delta, delta_growth_rate, num_itr_lb, num_rounds);
    }
    bdd_hip_parallel_mma<REAL>& solver() { return s_; }

    static std::vector<char> round(bddmma_solver* h, bddmma_lbfgs* l, double init_delta, double growth, int num_itr_lb, int num_rounds)
    {
        std::vector<char> sol(bddmma_nr_variables(h), 0);
        int found = 0;
        if (bddmma_incremental_mm_agreement_rounding(h, l, init_delta, growth, (uint64_t)num_itr_lb, (uint64_t)num_rounds, 0, 0, sol.data(), &found) != BDDMMA_OK)
            throw std::runtime_error(std::string("incremental_mm_agreement_rounding: ") + bddmma_last_error(h));
        if (!found) sol.clear();
        return sol;
    }

   private:
    bdd_hip_parallel_mma<REAL> s_;
};

template <typename REAL>
class bdd_lbfgs_hip_mma {
   public:
    template <typename BDD_COLLECTION>
    bdd_lbfgs_hip_mma(const BDD_COLLECTION& bdd_col, const int history_size, const double init_step_size = 1e-6,
                      const double req_rel_lb_increase = 1e-6, const double step_size_decrease_factor = 0.8,
                      const double step_size_increase_factor = 1.1)
        : l_(bdd_hip_parallel_mma<REAL>(bdd_col), params(history_size, init_step_size, req_rel_lb_increase, step_size_decrease_factor, step_size_increase_factor))
    {
    }
    template <typename BDD_COLLECTION, typename ITERATOR>
    bdd_lbfgs_hip_mma(const BDD_COLLECTION& bdd_col, ITERATOR cost_begin, ITERATOR cost_end, const int history_size,
                      const double init_step_size = 1e-6, const double req_rel_lb_increase = 1e-6,
                      const double step_size_decrease_factor = 0.8, const double step_size_increase_factor = 1.1)
        : bdd_lbfgs_hip_mma(bdd_col, history_size, init_step_size, req_rel_lb_increase, step_size_decrease_factor, step_size_increase_factor)
    {
        update_costs(cost_begin, cost_begin, cost_begin, cost_end);  // as bdd_lbfgs_cuda_mma.h:41-52
    }
    template <typename ITERATOR>
    void update_costs(ITERATOR cost_lo_begin, ITERATOR cost_lo_end, ITERATOR cost_hi_begin, ITERATOR cost_hi_end)
    {
        const std::vector<REAL> lo(cost_lo_begin, cost_lo_end), hi(cost_hi_begin, cost_hi_end);
        constexpr int prec = std::is_same<REAL, double>::value ? BDDMMA_F64 : BDDMMA_F32;
        // lbfgs::update_costs also drops the history (lbfgs_impl.h:343-364)
        if (bddmma_lbfgs_update_costs(l_.lbfgs_handle(), lo.data(), lo.size(), hi.data(), hi.size(), prec, 0) != BDDMMA_OK)
            throw std::runtime_error(std::string("bdd_lbfgs_hip_mma: ") + bddmma_last_error(l_.solver().handle()));
    }
    double lower_bound() { return l_.lower_bound(); }
    size_t nr_variables() { return l_.solver().nr_variables(); }
    std::vector<std::vector<std::array<double, 2>>> min_marginals() { return l_.solver().min_marginals(); }
    void iteration() { l_.iteration(); }
    void backward_run() { l_.solver().backward_run(); }
    std::vector<char> incremental_mm_agreement_rounding(const double init_delta, const double delta_growth_rate, const int num_itr_lb,
                                                        const int num_rounds = 500)
    {
        return bdd_hip<REAL>::round(l_.solver().handle(), l_.lbfgs_handle(), init_delta, delta_growth_rate, num_itr_lb, num_rounds);
    }

   private:
    static const bddmma_lbfgs_params* params(int m, double s, double r, double d, double i)
    {
        static thread_local bddmma_lbfgs_params p;
        p = bddmma_lbfgs_params{m, s, r, d, i};
        return &p;
    }
    bdd_hip_lbfgs_mma<REAL> l_;
};

}  // namespace LPMP
