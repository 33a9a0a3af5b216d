/*
 * bdd_mma.h — C-ABI of the MI355X-native parallel deferred min-marginal-averaging
 * (MMA) solver over BDDs.
 *
 * This is the drop-in boundary for the reference's GPU relaxation solver
 * `LPMP::bdd_cuda_parallel_mma<REAL>` and its base `LPMP::bdd_cuda_base<REAL>`
 * (reference: include/bdd_solver/bdd_cuda_parallel_mma.h:7-52,
 * include/bdd_solver/bdd_cuda_base.h:58-229).  The reference has no FFI for this
 * path; the boundary is a compile-time "solver concept" selected by
 * `"relaxation solver": "cuda parallel mma"` (src/bdd_solver/bdd_solver.cpp:164-176).
 * Every entry point below names the reference member function it replaces.
 *
 * Conventions
 *  - Nothing but POD crosses the ABI.  All device memory is owned by the handle.
 *  - Every call returns BDDMMA_OK (0) or a negative error code; the message is
 *    available from bddmma_last_error().  No C++ exception crosses the ABI.
 *  - `precision` is BDDMMA_F32 or BDDMMA_F64; "REAL" below means that type.
 *    Buffers declared `void*` hold REAL elements of the handle's precision.
 *  - `on_device` != 0 means the buffer is a device pointer on the handle's GPU
 *    (the reference's thrust::device_vector overloads); 0 means host memory.
 *  - One handle per problem; handles are independent (own stream, own buffers)
 *    so one host thread/process per GPU is safe (reference: single stream,
 *    device 0 hard-coded, include/cuda_utils.h:111-114).  A device buffer written or read by another stream (a tensor of a
 *    framework that runs on a stream of its own) is not ordered against the handle's stream by itself: bddmma_stream_wait before the
 *    calls that read it and bddmma_stream_signal after the calls that read or write it order the two streams without the host
 *    waiting for either (or synchronise the device, as callers had to before these existed).
 *  - Layers: one layer per (BDD, variable) pair = one dual variable.  Terminal
 *    layers carry no information and are not exposed: nr_layers() equals the
 *    reference CPU solver's nr_layers() (bdd_parallel_mma_base.cpp:1398-1402),
 *    i.e. the reference GPU nr_layers() minus nr_bdds().  Per-layer vectors are
 *    in the solver's internal layer order; bddmma_layer_variables /
 *    bddmma_layer_bdds give the (variable, BDD) of every entry.
 */
#ifndef BDD_MMA_H
#define BDD_MMA_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BDDMMA_OK 0
#define BDDMMA_ERR_INVALID_ARGUMENT (-1)
#define BDDMMA_ERR_INVALID_BDD (-2)   /* not a QBDD / malformed collection */
#define BDDMMA_ERR_DEVICE (-3)        /* HIP runtime error */
#define BDDMMA_ERR_STATE (-4)         /* call not valid in current solver state */
#define BDDMMA_ERR_UNSUPPORTED (-5)
#define BDDMMA_ERR_IO (-6)

#define BDDMMA_F32 0
#define BDDMMA_F64 1

/* Bit-identical to BDD::bdd_instruction {size_t lo, hi, index}
 * (reference: include/bdd_collection/bdd_collection.h:14-36).  `lo`/`hi` are
 * ABSOLUTE indices into the instruction array; terminals have
 * index == BDDMMA_TOPSINK / BDDMMA_BOTSINK. */
typedef struct bddmma_instruction {
    uint64_t lo;
    uint64_t hi;
    uint64_t index;
} bddmma_instruction;

#define BDDMMA_TOPSINK UINT64_MAX
#define BDDMMA_BOTSINK (UINT64_MAX - 1)

typedef struct bddmma_solver bddmma_solver;

/* Tunables of the device layout (0 = default). */
typedef struct bddmma_options {
    uint32_t pack_width;       /* max #nodes of one hop inside a wave-sized BDD pack: 64, 128 (default) or 256 */
    uint32_t wide_pack_width;  /* max #nodes of one hop inside a workgroup-sized pack whose frontier lives in LDS (default 2048; <= 2048 for
                                  F64, <= 4096 for F32); BDDs with wider layers use the same kernels with the frontier in global memory */
    uint32_t deterministic;    /* 1: the per-variable delta sums in a fixed order — (variable, bdd), the CPU solver's — instead of LDS atomics:
                                  bit-reproducible; one launch like the default exchange, ~10 % slower than it at 10 M nodes */
    uint32_t vars_per_bin;     /* variables per exchange bin, <= 9728 (16 B of LDS accumulators each); default: ~V/256 rounded, 1024..9728 */
    uint32_t stage_cap;        /* max layers of one stage group of a narrow pack (default 640) */
    uint32_t waves_per_block;  /* narrow packs swept by one workgroup with cooperative staging: 1, 2, 4 or 8 (default 4) */
    uint32_t keep_bdd_order;   /* 1: keep the input order of the BDDs when forming packs (default: BDDs of equal shape are grouped, diamond-shaped
                                  BDDs of small shape classes — general linear rows — follow widest first; 2: grouped by shape only) */
    uint32_t resident_sweeps;  /* narrow packs copied to LDS up front and swept from there: 0 automatic (when every workgroup of a sweep can
                                  be in flight at once: small / medium instances), 1 off, 2 on whenever the packs fit */
    uint32_t exchange_by_variable;  /* 2: entry arrays ordered by (variable, bdd) — the per-variable delta reduction becomes one thread
                                  per variable over a contiguous run: deterministic, no LDS accumulators, a shorter exchange launch; but
                                  the sweeps' accesses to the entry arrays lose their locality (slower overall on every instance
                                  measured).  Default (0 / 1): binned order */
    uint32_t variant_flags;    /* TEST HOOKS, default 0.  Every bit forces a code path of the shipped library that the automatic rules choose on
                                  other shapes or sizes, so that the differential tests reach it on small instances; none changes results
                                  beyond floating-point summation order.  (The A/B-only switches of rounds 2-4 — bits 2-8 and 16 — are gone:
                                  the paths they selected were deleted or are selected by rule alone; those bits are ignored.)
                                  bit 0 / bit 1: narrow and wide backward / forward sweeps as two launches (rule: one launch, k_*_mixed, except
                                                 where the wide share is large)
                                  bit 9 / bit 10: make_dual_feasible of the L-BFGS direction through the staging tables / by gathers
                                                  (rule: staged from 500 000 layers on)
                                  bit 11: first-generation resident sweeps (rule: packs of 128 / 256 slots or layers wider than two nodes)
                                  bit 12: first-generation streaming solve sweeps (rule: packs that share no records; float above 16 M slots)
                                  bit 13: per-lane records for the streaming solve sweeps also where packs do not share them
                                  bit 14: staging transfers with 64-bit addresses (rule: arrays of 4 GiB and more)
                                  bit 15: the L-BFGS direction as its own pass (rule: wide packs present, or the projection by gathers)
                                  bit 17: `deterministic` exchanges by per-variable gathers, two launches (rule: bins that do not fit the
                                          one-launch schedule k_exchange_seg; same sums, same order: bit-equal results)
                                  bit 18: no third-generation streaming solve sweeps (a lane per layer; rule: packs of 128 slots with layers of
                                          <= 2 nodes and <= 64 layers per hop that share their records, up to 16 M slots): the second / first
                                          generation instead (bit 13 lifts the sharing and size conditions of the third generation too)
                                  bit 19: four launches per iteration also for instances that fit one workgroup (rule: whole iterations in one
                                          launch, k_iterate_small, for <= 16 narrow packs of 64 slots with layers of <= 2 nodes)
                                  bit 20: the streaming solve sweeps' instantiations that load potentials and staging tables non-temporally
                                          whatever the footprint (rule: arrays beyond 640 MiB; first generation, and second in double,
                                          packs of 128 slots, 4 / 8 per workgroup; the third generation's own: double beyond 640 MiB)
                                  bit 21: solve sweeps of iteration() keep F and T in memory (narrow3) (rule: float, third generation, packs that
                                          start from the resident headers and have <= 16 hops rebuild both potentials on chip inside
                                          bddmma_iteration / _iterations / _run_solver, k_fwd_narrow4 / k_bwd_narrow4; a test hook: same results)
                                  bits 22, 23: of those sweeps only the one that rebuilds T (22) / F (23) on chip, the other potential through
                                          memory (measurement hooks; built for 4 packs per workgroup and <= 10 hops, elsewhere as bit 21)
                                  bit 24: no lane-per-BDD sweeps: those sweeps walk their hops through LDS, k_fwd_narrow4 / k_bwd_narrow4
                                          (rule: where both potentials are on chip, capacity 10 or 12, and every structure template is
                                          lane-affine, csrc/layout.hpp: LaneCodes, the walks stay in registers, k_fwd_narrow5 /
                                          k_bwd_narrow5; a test hook: same results, bit for bit; bddmma_lane_sweeps reports the choice) */
    uint32_t pack_fill;        /* slots of a narrow pack's hop that further BDDs are packed into, in [2, pack_width] (default 0 = pack_width).
                                  Smaller values give more, emptier packs (more wavefronts for the same nodes); measured slower on every
                                  instance (NOTES.md section 6: the sweeps are bound by instructions issued, not by latency), kept for experiments */
    uint32_t pack_stagger;     /* narrow packs whose BDDs start at different hops ("staggered"): a BDD that no longer fits next to the ones
                                  of the open pack hop by hop is tried a few hops further down, where those have become narrow again — BDDs
                                  of general linear rows are narrow at both ends and wide in the middle, and side by side from hop 0 they
                                  fill ~30 % of a pack's lanes.  Value = most hops a pack may have; 0: automatic (on when the instance is
                                  large enough to keep ~2 700 packs of three BDD lengths), 1: off.  Applies to the wide packs too: a chained
                                  wide pack is one BDD wide (automatic while >= ~500 packs and enough wavefronts for the chip remain). */
} bddmma_options;

/* ---- construction ------------------------------------------------------- */

/* Replaces bdd_cuda_parallel_mma<REAL>(const BDD::bdd_collection&, const std::vector<double>& costs_hi)
 * (src/bdd_solver/bdd_cuda_parallel_mma.cu:7-17, bdd_cuda_base.cu:31-53).
 * `bdd_delims` has n_bdds+1 entries: BDD b occupies instr[bdd_delims[b] .. bdd_delims[b+1]),
 * nodes grouped by variable in BDD order, the two terminals last (either order).
 * Every BDD must be a reordered QBDD (bdd_cuda_base.cu:98-99).
 * costs_hi may be NULL (n_costs = 0): all costs zero. */
int bddmma_create(bddmma_solver** out, int precision, int device,
                  const bddmma_instruction* instr, const uint64_t* bdd_delims, uint64_t n_bdds,
                  const double* costs_hi, uint64_t n_costs, const bddmma_options* opts);
void bddmma_destroy(bddmma_solver* s);

/* Number of HIP devices visible to the process (0 when there is none / no driver).  One host thread per device, each with its own
 * handles, is the multi-GPU model: independent instances, no collective (reference: device 0 hard-coded, include/cuda_utils.h:111-114). */
int bddmma_device_count(void);
/* What the layout rules and the input stage ask the chip (hipDeviceProp of `device`): compute units, LDS bytes per compute unit, and
 * multiProcessorCount * maxThreadsPerMultiProcessor — the figure the reference's getMaximumOccupancy() derives its split length from
 * (src/bdd_conversion/bdd_preprocessor.cpp:21-30: cudaGetDeviceProperties, / 10 there).  Any out pointer may be NULL.
 * BDDMMA_ERR_DEVICE when there is no such device. */
int bddmma_device_chip(int device, uint32_t* n_cus, uint32_t* lds_bytes_per_cu, uint64_t* max_resident_threads);
/* Host threads one layout build (bddmma_create) may use: 0 = automatic (environment BDDMMA_THREADS, else min(cores, 32)).  A process that
 * builds one instance per GPU at the same time gives every build cores / #GPUs (the reference builds its layout on the device,
 * bdd_cuda_base.cu:146-391; here it is host work). */
int bddmma_set_layout_threads(int n);
/* The same limit for the builds started by the calling host thread only (0 = follow the process-wide setting).  One-solver-per-GPU host
 * threads (include/cuda_utils.h:111-114 of the reference knows one device; the batch farm here has a thread per device) set it for
 * themselves, so concurrent batches and the application's own process-wide value do not overwrite each other. */
int bddmma_set_thread_layout_threads(int n);
/* Error text of the last failed call on `s`; with s == NULL the last failed bddmma_create. */
const char* bddmma_last_error(const bddmma_solver* s);

/* ---- sizes (bdd_cuda_base.h:98-116) -------------------------------------- */
uint64_t bddmma_nr_variables(const bddmma_solver* s);
uint64_t bddmma_nr_bdds(const bddmma_solver* s);
uint64_t bddmma_nr_layers(const bddmma_solver* s);      /* non-terminal layers = #dual variables */
uint64_t bddmma_nr_bdd_nodes(const bddmma_solver* s);   /* incl. 2 terminals per BDD, as the reference counts */
uint64_t bddmma_nr_hops(const bddmma_solver* s);        /* length of the longest BDD */
uint64_t bddmma_nr_packs(const bddmma_solver* s);
/* Which kernels run the solve sweeps (forward_mm / backward_mm) of the narrow packs — chosen by rule at creation from the instance's shape and
 * size; diagnostics for benchmarks and for the tests that must know which path they compare with the oracle. */
enum {
    BDDMMA_SWEEPS_NONE = 0,        /* no narrow packs (wide / huge packs only) */
    BDDMMA_SWEEPS_MIXED = 1,       /* narrow and wide packs in one launch (k_fwd_mixed / k_bwd_mixed) */
    BDDMMA_SWEEPS_STREAMING1 = 2,  /* streaming, node words (k_fwd_narrow / k_bwd_narrow) */
    BDDMMA_SWEEPS_STREAMING2 = 3,  /* streaming, a 16-byte record per lane and hop (k_*_narrow2) */
    BDDMMA_SWEEPS_STREAMING3 = 4,  /* streaming, a lane per layer (k_*_narrow3) */
    BDDMMA_SWEEPS_RESIDENT1 = 5,   /* pack resident in LDS (k_*_res) */
    BDDMMA_SWEEPS_RESIDENT2 = 6    /* pack resident in LDS, records (k_*_res2) */
};
int bddmma_solve_sweep_kind(const bddmma_solver* s);
/* 1 when the instance fits one workgroup and bddmma_iterations / bddmma_run_solver run whole iterations inside one launch (sweeps, exchanges
 * and run_solver's tests with workgroup barriers in between, csrc/kernels/small.hpp; variant_flags bit 19 turns it off), else 0. */
int bddmma_fused_small(const bddmma_solver* s);
/* 1 when bddmma_learned_iterations / _omega_vec run whole learned iterations inside one launch too (k_learned_small): bddmma_fused_small
 * holds and the learned layout — the plain one plus an omega per layer — fits the CU's LDS as well.  With improvement_slope <= 0 the iterations that compute_history_for_itr does not reach then run fused; with a stopping rule
 * (improvement_slope > 0) every iteration of this call keeps the four launches (a batch: bddmma_learned_iterations_stop_batch).  variant_flags bit 19 turns it off together with bddmma_fused_small. */
int bddmma_fused_small_learned(const bddmma_solver* s);
/* 1 when bddmma_learned_iterations_history_batch can also run the history step of a tracked iteration (the per-BDD bounds, every BDD's
 * arg-min path and the moving averages) inside this solver's workgroup: bddmma_fused_small_learned holds and the solver has a thread per
 * BDD.  The step needs no LDS of its own — its marks live in entries that are dead between a backward sweep and the next exchange — so today
 * this is 1 wherever bddmma_fused_small_learned is. */
int bddmma_fused_small_history(const bddmma_solver* s);
/* 1 when bddmma_learned_iterations_stop_batch can run this solver's stopping rule (improvement_slope > 0) inside its workgroup too:
 * bddmma_fused_small_history holds and the rule's working values — a few words of static LDS beside the learned layout — fit the CU's LDS as
 * well. */
int bddmma_fused_small_stop(const bddmma_solver* s);
/* 1 when the narrow packs' solve sweeps run in the instantiation that loads what a sweep reads once (potentials, staging tables) non-temporally. */
int bddmma_nontemporal_loads(const bddmma_solver* s);
/* 1 when the solve sweeps of bddmma_iteration / _iterations / _run_solver rebuild the costs-from-root and costs-to-terminal on chip instead of
 * storing and reloading them (csrc/kernels/narrow4.hpp; variant_flags bit 21 turns it off).  bddmma_solve_sweep_kind stays STREAMING3. */
int bddmma_potentials_on_chip(const bddmma_solver* s);
/* The hop capacity of the kernels behind bddmma_potentials_on_chip, the smallest that holds the solver's longest pack: 0 (not on chip), 10 or
 * 12 (both potentials on chip: k_fwd_narrow4 with k_bwd_narrow4), 16 (the costs-from-root on chip, the costs-to-terminal through memory:
 * k_fwd_narrow3 with k_bwd_narrow4). */
int bddmma_onchip_hops(const bddmma_solver* s);
/* 1 when those sweeps keep a BDD's potentials in one lane's registers and walk the hops without LDS (csrc/kernels/narrow5.hpp: both
 * potentials on chip, capacity 10 or 12, every structure template lane-affine; variant_flags bit 24 turns it off), else 0; -1 without a
 * solver.  bddmma_onchip_hops, bddmma_potentials_on_chip and bddmma_solve_sweep_kind do not change with it. */
int bddmma_lane_sweeps(const bddmma_solver* s);
int bddmma_precision(const bddmma_solver* s);
int bddmma_device(const bddmma_solver* s);
/* nr_bdds(var): int32[nr_variables] (get_num_bdds_per_var, bdd_cuda_base.h:166) */
int bddmma_num_bdds_per_var(const bddmma_solver* s, int32_t* out);
/* (variable, bdd) of every layer in internal layer order (get_primal_variable_index / get_bdd_index) */
int bddmma_layer_variables(const bddmma_solver* s, int32_t* out);
int bddmma_layer_bdds(const bddmma_solver* s, int32_t* out);
/* nodes / layers per hop (get_cum_nr_bdd_nodes_per_hop_dist etc., non-cumulative, nr_hops entries) */
int bddmma_nodes_per_hop(const bddmma_solver* s, uint64_t* out);
int bddmma_layers_per_hop(const bddmma_solver* s, uint64_t* out);

/* ---- costs -------------------------------------------------------------- */
/* update_costs(cost_delta_0, cost_delta_1) (bdd_cuda_base.cu:476-558): cost[layer] += c[var]/nr_bdds(var).
 * n_lo / n_hi may be 0 (that side untouched) or <= nr_variables; layers of variables >= n are
 * SET to 0 as in the reference (bdd_cuda_base.cu:465-469).  elem_precision: type of lo/hi buffers. */
int bddmma_update_costs(bddmma_solver* s, const void* lo, uint64_t n_lo, const void* hi, uint64_t n_hi,
                        int elem_precision, int on_device);
/* set_cost(c, var) (bdd_cuda_base.cu:441-455): hi cost of all layers of `var` += c/nr_bdds(var). */
int bddmma_set_cost(bddmma_solver* s, double c, uint64_t var);
/* get_solver_costs / set_solver_costs (bdd_cuda_base.cu:1308-1344): REAL[nr_layers] each. */
int bddmma_get_solver_costs(const bddmma_solver* s, void* lo, void* hi, void* deferred_mm_diff, int on_device);
int bddmma_set_solver_costs(bddmma_solver* s, const void* lo, const void* hi, const void* deferred_mm_diff, int on_device);
/* compute_primal_objective_vec (bdd_cuda_base.cu:1352-1362): out[var] = sum over layers of var (hi - lo). */
int bddmma_primal_objective_vec(bddmma_solver* s, void* out, int on_device);

/* ---- plain sweeps ------------------------------------------------------- */
int bddmma_forward_run(bddmma_solver* s);   /* bdd_cuda_base.cu:588-612 */
int bddmma_backward_run(bddmma_solver* s);  /* bdd_cuda_base.cu:669-713 (without path costs) */
/* lower_bound() (bdd_cuda_base.cu:1243-1251): sum of root costs-from-terminal, accumulated in double. */
int bddmma_lower_bound(bddmma_solver* s, double* lb);
/* lower_bound_per_bdd (bdd_cuda_base.cu:1253-1259): REAL[nr_bdds], indexed by BDD number. */
int bddmma_lower_bound_per_bdd(bddmma_solver* s, void* out, int on_device);

/* ---- parallel MMA (bdd_cuda_parallel_mma.cu) ------------------------------ */
/* iteration(omega) (:142-153): forward_mm, normalize_delta, backward_mm, normalize_delta on the
 * solver's own deferred delta. Asynchronous: returns once queued on the handle's stream. */
int bddmma_iteration(bddmma_solver* s, double omega);
/* n iterations back to back without host synchronisation. */
int bddmma_iterations(bddmma_solver* s, double omega, uint64_t n);
/* forward_mm(omega, delta_lo_hi) / backward_mm (:207-257, :301-346): delta is REAL[2*nr_variables],
 * interleaved {lo,hi}; read as the values to add, overwritten with the un-normalised sums. */
int bddmma_forward_mm(bddmma_solver* s, double omega, void* delta_lo_hi, int on_device);
int bddmma_backward_mm(bddmma_solver* s, double omega, void* delta_lo_hi, int on_device);
/* normalize_delta (:410-430): delta[i] /= nr_bdds(i/2). */
int bddmma_normalize_delta(const bddmma_solver* s, void* delta_lo_hi, int on_device);
/* distribute_delta() (bdd_cuda_base.cu:1396-1436). */
int bddmma_distribute_delta(bddmma_solver* s);
/* the solver's deferred delta_lo_hi_ (REAL[2*nr_variables]) */
int bddmma_get_delta(const bddmma_solver* s, void* out, int on_device);
int bddmma_set_delta(bddmma_solver* s, const void* in, int on_device);

/* ---- learned iterations (bdd_cuda_learned_mma<REAL>, src/bdd_solver/bdd_cuda_learned_mma.cu:9-262; Python binding
 * bdd_cuda_learned_mma_py.cu:300-326,580-600) -----------------------------------------------------------------------------
 * bddmma_learned_iterations = iterations(dist_weights, num_itr, omega, improvement_slope, sol_avg, lb_first_diff_avg, lb_second_diff_avg,
 * compute_history_for_itr, history_avg_beta) (:184-270) with a scalar omega (per-layer omega_vec: bddmma_learned_iterations_omega_vec).  Every pass (forward, then backward) starts from
 * the sums of the deferred min-marginal differences per variable, Slo[v] = sum max(-mm, 0), Shi[v] = sum max(mm, 0) — NOT divided by
 * nr_bdds(v) — and adds alpha[l] * S[v(l)] to layer l: lo' = lo + min(mm, 0) + alpha * Slo, hi' = hi + min(-mm, 0) + alpha * Shi (:37,:42).
 * The product is formed in REAL from the sum rounded to REAL.  With alpha[l] = 1 / nr_bdds(v(l)) (bddmma_isotropic_dist_weights) this is
 * bddmma_iteration up to that rounding.
 *   dist_weights   REAL[nr_layers] in the public layer order (bddmma_get_solver_costs, bddmma_bdds_solution(sorted = 0),
 *                  bddmma_layer_variables), host or device (weights_on_device).  A negative or non-finite weight gives
 *                  BDDMMA_ERR_INVALID_ARGUMENT and leaves the solver untouched.  sum over the layers of a variable = 1 is NOT enforced:
 *                  only with it is the bound a valid bound of the original problem (costs are then a reparametrisation of it).
 *   improvement_slope  > 0: lower_bound() after every iteration (one host round trip each); stop when |lb_prev - lb_post| <
 *                  improvement_slope * initial_lb_change and the history is complete (:261-266).  initial_lb_change = |lb before - lb after
 *                  the first iteration| of the first call on this solver that runs an iteration (set once per solver, :263,
 *                  bdd_cuda_learned_mma.h:111-116).  <= 0: all num_itr iterations, no host synchronisation between them.
 *   compute_history_for_itr > 0: over the last that many iterations (and every iteration after convergence) sol_avg REAL[nr_layers]
 *                  becomes an exponential moving average (factor history_avg_beta) of bdds_solution (public layer order, 0 / 1),
 *                  lb_first_diff_avg REAL[nr_bdds] of the change of lower_bound_per_bdd, lb_second_diff_avg REAL[nr_bdds] of its second
 *                  difference; the first value of each is copied in, not averaged (:211-254).  An output the history does not reach keeps
 *                  its content.  Host or device (outputs_on_device); ignored when compute_history_for_itr = 0 (may be null then).
 *   itr_done       the number of iterations run (the reference returns the loop index at the break, one less when it stops early).
 * State contract (the reference leaves it open):
 *   entry  the first pass's delta is derived from the solver's deferred differences with the given weights; a pending isotropic delta
 *          (bddmma_get_delta), which is derived from the same differences, is ignored;
 *   exit   the deferred differences are the last backward pass's, and the per-variable delta and its per-layer broadcast are what the
 *          isotropic exchange of them gives — the state bddmma_iteration leaves.  So bddmma_get_delta, bddmma_distribute_delta,
 *          bddmma_iteration(s), bddmma_run_solver, bddmma_min_marginals and bddmma_save work unchanged afterwards, and learned iterations
 *          with isotropic weights (n) followed by bddmma_iterations (m) equal bddmma_iterations (n + m).
 * An L-BFGS wrapper attached to the handle (bddmma_lbfgs_create without bddmma_lbfgs_destroy yet) makes the call return BDDMMA_ERR_STATE:
 * its history would describe costs that the iterations have moved.  Synchronous when improvement_slope > 0, a history is written to the
 * host or the initial change is still unset; otherwise returns once queued. */
int bddmma_learned_iterations(bddmma_solver* s, const void* dist_weights, int weights_on_device, uint64_t num_itr, double omega,
                              double improvement_slope, void* sol_avg, void* lb_first_diff_avg, void* lb_second_diff_avg,
                              uint64_t compute_history_for_itr, double history_avg_beta, int outputs_on_device, uint64_t* itr_done);
/* bddmma_learned_iterations with one omega per layer (omega_vec of iterations(..., omega_vec), bdd_cuda_learned_mma.cu:184-270 with
 * bdd_cuda_parallel_mma.cu:45-57,117-128): the deferred difference of layer l is omega_vec[l] * (m1 - m0) — one product in REAL, the
 * scalar call's arithmetic — in place of omega * (m1 - m0).  An omega_vec that holds omega everywhere gives the scalar call's results bit
 * for bit.
 *   omega_vec      REAL[nr_layers] in the public layer order (that of dist_weights), host or device (omega_vec_on_device).  Null, or a
 *                  negative or non-finite value, gives BDDMMA_ERR_INVALID_ARGUMENT and leaves the solver untouched.
 * Every other argument, the stopping rule, the history, the state contract on exit and the refusal while an L-BFGS wrapper is attached are
 * those of bddmma_learned_iterations. */
int bddmma_learned_iterations_omega_vec(bddmma_solver* s, const void* dist_weights, int weights_on_device, uint64_t num_itr, const void* omega_vec,
                                        int omega_vec_on_device, double improvement_slope, void* sol_avg, void* lb_first_diff_avg,
                                        void* lb_second_diff_avg, uint64_t compute_history_for_itr, double history_avg_beta, int outputs_on_device,
                                        uint64_t* itr_done);
/* REAL[nr_layers], public layer order: 1 / nr_bdds(variable of the layer) in REAL — the weights with which learned iterations are the
 * plain ones (the isotropic alpha of the learned solver's Python side). */
int bddmma_isotropic_dist_weights(bddmma_solver* s, void* out, int on_device);

/* ---- min-marginals and per-BDD solutions -------------------------------- */
/* min_marginals_cuda(get_sorted) (bdd_cuda_base.cu:716-749): var int32[nr_layers], mm0/mm1 REAL[nr_layers].
 * sorted != 0: ordered by (variable, bdd) as primal_variable_sorting_order_ (bdd_cuda_base.cu:379-391). */
int bddmma_min_marginals(bddmma_solver* s, int sorted, int32_t* var, void* mm0, void* mm1, int on_device);
/* mm1 - mm0 per layer, internal layer order, REAL[nr_layers] (compute_and_set_min_marginal_diff of the reference's Python module,
 * src/bdd_solver/bdd_cuda_parallel_mma_py.cu:56-72: min_marginals_cuda(false) followed by thrust::minus into the caller's buffer). */
int bddmma_min_marginal_diff(bddmma_solver* s, void* out, int on_device);
/* sum_marginals_cuda(get_sorted, get_log_probs) (bdd_cuda_base<REAL>::sum_marginals_cuda, bdd_cuda_base.cu:788-1025): with the current arc
 * costs (deferred differences NOT applied, as in the reference), per non-terminal layer l of BDD b
 *   sm0[l] = log sum over the root -> top paths P of b that take a lo arc in layer l of exp(-cost(P)),   sm1[l]: the same with a hi arc,
 * computed in the log domain throughout (costs of a few hundred are fine in float).  log_probs = 0: exp of both.  A side no such path
 * takes is -inf (probability 0); the reference's -1e30 sentinel ends as about -1e30 there.  var int32[nr_layers] (may be NULL), sm0 / sm1
 * REAL[nr_layers] (NULL: BDDMMA_ERR_INVALID_ARGUMENT, solver untouched); orders and on_device as bddmma_min_marginals.
 * One forward and one backward launch per pack family (csrc/kernels/summarg.hpp); every sum in a fixed order: repeated calls agree bit for bit.
 * State contract: the call overwrites the stored costs from root and to terminal with log-partition values, so it ends with both sweep
 * states invalid and the cached lower bound dropped (the reference flushes both, :1008-1011) — the next entry point that needs them
 * recomputes them from the costs.  Arc costs, deferred differences, delta and therefore the result of every other entry point called
 * afterwards are unchanged, also with an L-BFGS wrapper attached and between two bddmma_learned_iterations calls. */
int bddmma_sum_marginals(bddmma_solver* s, int sorted, int log_probs, int32_t* var, void* sm0, void* sm1, int on_device);
/* smooth_solution_cuda (bdd_cuda_base<REAL>::smooth_solution_cuda, bdd_cuda_base.cu:1027-1064; smooth_solution_per_bdd of the learned
 * solver): out[l] = exp(sm1) / (exp(sm0) + exp(sm1)) of the log sum-marginals, evaluated as ComputeSmoothSolution does (both shifted by
 * their maximum); REAL[nr_layers] in internal layer order (the reference also writes 0 for terminal layers, which are not stored here).
 * 0.5 where no path crosses the layer.  NULL: BDDMMA_ERR_INVALID_ARGUMENT, solver untouched.  State contract: bddmma_sum_marginals. */
int bddmma_smooth_solution(bddmma_solver* s, void* out, int on_device);
/* bdds_solution_vec() (bdd_cuda_base.cu:1139-1202): char[nr_layers] argmin path per BDD, internal
 * layer order (sorted = 0) or (variable,bdd) order (sorted = 1, as bdds_solution(), :1204-1233). */
int bddmma_bdds_solution(bddmma_solver* s, int sorted, char* sol, int on_device);

/* ---- single-shot backward operators (bdd_cuda_learned_mma.h:82-110) ------ */
/* Transpose-Jacobian products with respect to the arc costs.  Every layer-sized array is REAL[nr_layers] in the public layer order (that of
 * bddmma_get_solver_costs, bddmma_min_marginal_diff and bddmma_bdds_solution(sorted = 0)), on the host or the device (on_device, one flag
 * for all arrays of a call); inputs and outputs must not overlap.  A null pointer or a non-finite incoming gradient gives
 * BDDMMA_ERR_INVALID_ARGUMENT and leaves the solver untouched.  No entry point changes arc costs, deferred differences or delta; all of
 * them work with an L-BFGS wrapper attached.  Backpropagation through the learned iterations: bddmma_grad_learned_iterations below. */
/* grad_mm_diff_all_hops (bdd_cuda_learned_mma.cu:623-1023; grad_all_min_marginal_differences of the reference's Python module): the
 * transpose-Jacobian product of bddmma_min_marginal_diff with respect to the current lo / hi arc costs, deferred differences NOT applied
 * (as in the forward call).  With F the cost from the root, T the cost to the terminal and, per layer l and arc a,
 * m_a[l] = min over the nodes u of l of F[u] + c_a[l] + T[child_a(u)], the result is
 *   grad_lo / grad_hi = sum over l of grad_mm[l] * (chi(P_hi(l)) - chi(P_lo(l))),
 * P_a(l) a minimum-cost root -> top path that takes arc a in layer l, chi its indicator over (layer, arc).  An arc no finite path takes
 * contributes nothing.
 * Tie rule: where a minimum is attained more than once the result is one valid subgradient, chosen by a fixed rule — lowest slot first
 * among a layer's nodes (slot order is the node order of the BDD's layer in the layout), first in parent table order among the parents of
 * a node (parents by slot, lo arc before hi arc), lo before hi between a node's two arcs.  The reference resolves ties by a race; agreement
 * with it at ties is not a goal.  Every sum has a fixed order and nothing is accumulated atomically: two calls agree bit for bit.
 * One launch per direction and pack family (csrc/kernels/gradmm.hpp).
 * State contract: reads the stored costs from root and to terminal of the plain sweeps and recomputes whichever is invalid (also right
 * after bddmma_sum_marginals, which overwrites both); both are valid on return.  Nothing else changes. */
int bddmma_grad_min_marginal_diff(bddmma_solver* s, const void* grad_mm, void* grad_lo_out, void* grad_hi_out, int on_device);
/* grad_lower_bound_per_bdd (bdd_cuda_learned_mma.cu:387-416; grad_lower_bound_per_bdd and grad_smooth_lower_bound_per_bdd of the Python
 * module): grad_hi[l] = x[l] * grad_lb_per_bdd[bdd(l)], grad_lo[l] = (1 - x[l]) * grad_lb_per_bdd[bdd(l)]; grad_lb_per_bdd is
 * REAL[nr_bdds] in the order of bddmma_lower_bound_per_bdd.  smooth = 0: x is bddmma_bdds_solution (0 / 1), the gradient of the per-BDD
 * lower bound; state contract of bddmma_bdds_solution.  smooth != 0: x is bddmma_smooth_solution, the gradient of
 * -log sum over paths of exp(-cost) per BDD; state contract of bddmma_sum_marginals. */
int bddmma_grad_lower_bound_per_bdd(bddmma_solver* s, const void* grad_lb_per_bdd, void* grad_lo_out, void* grad_hi_out, int smooth, int on_device);
/* grad_distribute_delta (bdd_cuda_learned_mma.cu:1025-1065): the backward of bddmma_distribute_delta with respect to the deferred
 * differences it applied: out[l] = grad_hi[l] where that difference was > 0, else -grad_lo[l].  grad_lo / grad_hi pass through to the
 * arc costs unchanged (identity Jacobian) and are not written.  The reference reads the deferred differences in place and so needs them
 * preserved by the caller; here bddmma_distribute_delta clears them and keeps a copy of what it applied, which this call reads: it
 * refers to the LAST bddmma_distribute_delta on this handle, whatever has run since, and returns BDDMMA_ERR_STATE when there was none
 * (a handle restored from a checkpoint included).  Cost of that copy, paid by every caller of bddmma_distribute_delta: REAL[nr_layers] of
 * device memory from the first such call on (counted by bddmma_device_bytes) and one device-to-device copy of it per call;
 * bddmma_distribute_delta is not part of an iteration. */
int bddmma_grad_distribute_delta(bddmma_solver* s, const void* grad_lo, const void* grad_hi, void* grad_deferred_mm_out, int on_device);
/* grad_cost_perturbation (bdd_cuda_learned_mma.cu:1067-1187): the backward of bddmma_update_costs' isotropic distribution: outputs
 * REAL[nr_variables], out[v] = (sum over the layers of v of grad[l]) / nr_bdds(v), summed in the order of the variable's layers by BDD.
 * Reads no solver state besides the layout. */
int bddmma_grad_cost_perturbation(bddmma_solver* s, const void* grad_lo, const void* grad_hi, void* grad_lo_pert_out, void* grad_hi_pert_out, int on_device);

/* grad_iterations (bdd_cuda_learned_mma.cu:308-385 with :418-621): the exact transpose-Jacobian product of track_grad_for_num_itr learned
 * iterations (bddmma_learned_iterations / _omega_vec with improvement_slope = 0 and no history), run after track_grad_after_itr untracked
 * ones, at the arg-mins those iterations took.  One iteration maps (lo, hi, d) — arc costs and deferred differences per layer — to new ones:
 * T = cost to terminal of (lo, hi); a forward pass root -> terminal with, per layer l, m_a[l] = min over its nodes u of F[u] + c_a[l] +
 * T[child_a(u)], mm[l] = omega_l (m_hi - m_lo) (0 unless both are finite), lo'[l] = lo[l] + min(mm, 0) + w[l] S_lo[v(l)],
 * hi'[l] = hi[l] + min(-mm, 0) + w[l] S_hi[v(l)], S the per-variable sums of max(-d, 0) / max(d, 0), F grown from the new costs; then a
 * backward pass terminal -> root, the same with that F, the forward pass's mm as d, and T rebuilt from the new costs as it rises.
 *   dist_weights, omega, omega_vec   those of the forward call (omega_vec null: the scalar omega; otherwise REAL[nr_layers] and omega is ignored)
 *   grad_lo, grad_hi, grad_mm        REAL[nr_layers], in-out: on entry the loss gradient with respect to the arc costs and deferred differences
 *                                    AFTER the tracked iterations, on return with respect to those BEFORE the first tracked iteration (after
 *                                    the untracked ones)
 *   grad_dist_weights_out            REAL[nr_layers], overwritten
 *   grad_omega_out                   REAL[1] (scalar omega: the per-layer values summed in double in a fixed order) or REAL[nr_layers]
 *   num_caches                       up to max(num_caches, 1) inputs of tracked iterations are kept on the device at the reference's interval
 *                                    rule (bdd_cuda_learned_mma.h:12-23); the others are replayed from the nearest one.  The caches (3 REAL per
 *                                    layer each) and the call's other arrays are allocated on first use and counted by bddmma_device_bytes.
 * Layer arrays are in the public layer order; on_device is one flag for the five gradient arrays.
 * The reverse of a pass uses the potentials F and T the pass itself read (the reference replays the pass and takes its arg-mins against the
 * potentials of the UPDATED costs, :542-545 and :592-595; agreement with it there is not a goal, agreement with finite differences of
 * bddmma_learned_iterations is).  Tie rules as bddmma_grad_min_marginal_diff; the dual update's rule at mm = 0 is the reference's (>= 0: the hi
 * side, :439-442), as is that of the consumed differences (:512-516).  One launch per pass and pack family (csrc/kernels/graditer.hpp), no
 * atomics in the reverse sweeps.
 * State contract: on entry the solver holds the state from which the forward call started.  On return the arc costs, the deferred
 * differences and delta are the entry values bit for bit; both sweep states are invalid (recomputed by whoever needs them).  Refusals, each
 * leaving the solver untouched: BDDMMA_ERR_STATE while an L-BFGS wrapper is attached or run_solver is queueing iterations;
 * BDDMMA_ERR_INVALID_ARGUMENT for a null pointer (omega_vec excepted), a non-finite incoming gradient, a negative or non-finite weight or
 * omega; BDDMMA_ERR_UNSUPPORTED where a wide pack's arrays (8 REAL + 12 bytes per slot) do not fit the LDS.
 * track_grad_for_num_itr = 0: no iteration runs, the in-out arrays are unchanged, both outputs are zero-filled.
 * The result does not depend on num_caches.  With the deterministic exchange (bddmma_options.deterministic) two calls, and calls with any two
 * num_caches, agree bit for bit; with the default LDS-atomic exchange the replayed iterations may differ in the last bits of a variable's sum
 * from call to call, and so may the result. */
int bddmma_grad_learned_iterations(bddmma_solver* s, const void* dist_weights, int weights_on_device, double omega, const void* omega_vec,
                                   int omega_vec_on_device, void* grad_lo, void* grad_hi, void* grad_mm, void* grad_dist_weights_out, void* grad_omega_out,
                                   uint64_t track_grad_after_itr, uint64_t track_grad_for_num_itr, uint64_t num_caches, int on_device);

/* ---- L-BFGS support (lbfgs.h:22-27) --------------------------------------- */
/* net_solver_costs() (bdd_cuda_parallel_mma.cu:432-463): hi - lo + deferred mm diff, REAL[nr_layers]. */
int bddmma_net_solver_costs(const bddmma_solver* s, void* out, int on_device);
/* make_dual_feasible(g) (bdd_cuda_base.cu:1261-1303): g[layer] -= mean over layers of the same variable. */
int bddmma_make_dual_feasible(const bddmma_solver* s, void* g, int on_device);
/* gradient_step(g, step) (bdd_cuda_parallel_mma.h:62-77): hi += step * g. */
int bddmma_gradient_step(bddmma_solver* s, const void* g, double step_size, int on_device);

/* L-BFGS outer solver wrapping a handle (lbfgs.h:35-111, lbfgs_impl.h). */
typedef struct bddmma_lbfgs bddmma_lbfgs;
typedef struct bddmma_lbfgs_params {
    int32_t history_size;                   /* "history size", default 5 */
    double init_step_size;                  /* "initial step size", default 1e-6 */
    double req_rel_lb_increase;             /* "required relative lb increase", default 1e-6 */
    double step_size_decrease_factor;       /* default 0.8 */
    double step_size_increase_factor;       /* default 1.1 */
} bddmma_lbfgs_params;
int bddmma_lbfgs_create(bddmma_lbfgs** out, bddmma_solver* s, const bddmma_lbfgs_params* p);
void bddmma_lbfgs_destroy(bddmma_lbfgs* l);
int bddmma_lbfgs_iteration(bddmma_lbfgs* l);       /* lbfgs::iteration(), lbfgs_impl.h:137-157 */
int bddmma_lbfgs_update_costs(bddmma_lbfgs* l, const void* lo, uint64_t n_lo, const void* hi, uint64_t n_hi,
                              int elem_precision, int on_device);  /* lbfgs_impl.h:353-364: also drops history */
int bddmma_lbfgs_flush(bddmma_lbfgs* l);           /* flush_lbfgs_states(), lbfgs_impl.h:318-326 */
/* What the state machine did in the last bddmma_lbfgs_iteration (the reference only logs these; exposed so that the
 * parity tests can compare the decision sequence with the CPU restatement oracle/lbfgs_oracle.py). */
typedef struct bddmma_lbfgs_state {
    double step_size;                 /* lbfgs::step_size after the last iteration */
    double last_applied_step;         /* step left applied by search_step_size_and_apply (0: none / rolled back) */
    uint64_t mma_iterations;          /* lbfgs::mma_iterations */
    uint64_t lbfgs_iterations;        /* lbfgs::lbfgs_iterations */
    int32_t history_entries;          /* history.size() */
    int32_t num_unsuccessful_updates; /* num_unsuccessful_lbfgs_updates_ */
    int32_t last_kind;                /* choose_solver() of the last iteration: 0 mma, 1 lbfgs */
    int32_t last_trials;              /* gradient steps taken by the last step-size search */
} bddmma_lbfgs_state;
int bddmma_lbfgs_get_state(const bddmma_lbfgs* l, bddmma_lbfgs_state* out);

/* ---- run_solver (include/run_solver_util.h:10-77) -------------------------
 * Same criteria, same order, same result as the reference's loop (iteration(); lower_bound(); time limit, minimum improvement,
 * improvement slope, infeasibility).  For the plain solver (lbfgs_or_null == NULL) the three tests on the bound run on the device,
 * in the launch that ends each iteration; the host keeps a few iterations queued and never synchronises inside the loop, and the
 * launches queued behind the stopping iteration return without doing anything — the solver is left in exactly the state after the
 * iteration that met the criterion.  The wall-clock limit is tested on the host after every iteration it sees complete. */
typedef struct bddmma_run_result {
    uint64_t iterations;
    double lb_initial;
    double lb_final;
    double seconds;
    int32_t stop_reason; /* 0 max iter, 1 time limit, 2 min improvement, 3 improvement slope, 4 infeasible */
} bddmma_run_result;
int bddmma_run_solver(bddmma_solver* s, bddmma_lbfgs* lbfgs_or_null, uint64_t max_iter, double tolerance,
                      double improvement_slope, double time_limit, int verbose, bddmma_run_result* res);
/* The same loop literally as the reference writes it — iteration(); lower_bound() with a host round trip; the tests on the host — for the
 * plain solver too (with an L-BFGS wrapper both entry points run this loop).  Same iteration count, same state, same bound. */
int bddmma_run_solver_host_loop(bddmma_solver* s, bddmma_lbfgs* lbfgs_or_null, uint64_t max_iter, double tolerance,
                                double improvement_slope, double time_limit, int verbose, bddmma_run_result* res);

/* ---- batches of one-workgroup instances ------------------------------------
 * Callers with instances that fit one workgroup (bddmma_fused_small == 1) usually have many of them.  A batch runs its members'
 * iterations concurrently, one workgroup per member in one launch per kernel instantiation present, instead of one launch of one
 * workgroup per handle.  The members are BORROWED: the batch never owns or destroys them, they stay usable on their own between the
 * batch's calls, and every member must outlive the batch — destroying a member before its batch is the caller's error (only
 * bddmma_batch_destroy and bddmma_batch_size may be called on such a batch).
 * Ordering: a batch call behaves as if the same call had been made on each member in turn.  It is ordered after everything already
 * queued on every member's stream, and everything queued on a member afterwards is ordered after it (events between the batch's
 * stream and the members' streams; the host does not synchronise).  Results are bit-equal to the per-member calls.
 * bddmma_batch_create: BDDMMA_ERR_INVALID_ARGUMENT for a null pointer, n == 0 or a handle listed twice; BDDMMA_ERR_UNSUPPORTED for a
 * member that is not bddmma_fused_small or that differs from member 0 in precision or device; BDDMMA_ERR_STATE for a member with an
 * L-BFGS wrapper attached or profiling on.  All of these are decided before any device call; bddmma_batch_last_error(NULL) names the
 * member index and the reason.
 * Every other call re-checks the members' state before it launches anything: when a member has since got an L-BFGS wrapper (attached
 * now or earlier: its backward sweeps then write x per layer), has profiling on or is inside bddmma_run_solver, the call returns
 * BDDMMA_ERR_STATE and every member is left untouched. */
typedef struct bddmma_batch bddmma_batch;
int bddmma_batch_create(bddmma_batch** out, bddmma_solver* const* members, uint64_t n);
void bddmma_batch_destroy(bddmma_batch* b);
/* error text of the last failed call on the batch; b == NULL: of the last failed bddmma_batch_create of this thread */
const char* bddmma_batch_last_error(const bddmma_batch* b);
uint64_t bddmma_batch_size(const bddmma_batch* b);
/* bddmma_iterations(member, omega, n) for every member */
int bddmma_batch_iterations(bddmma_batch* b, double omega, uint64_t n);
/* bddmma_learned_iterations(member i, w_i, .., num_itr, omega, 0.0, NULL, NULL, NULL, 0, 0.0, .., NULL) for every member i — or, with
 * omega_vec non-null, bddmma_learned_iterations_omega_vec with member i's part of it: one workgroup per member, one launch per kernel
 * instantiation present, results bit-equal to those calls (each member's set-once initial bound change included).
 * dist_weights, and omega_vec when given: the members' REAL[nr_layers] in the public layer order, one behind the other in the members'
 * order at bddmma_batch_create; both on the host or both on the device (on_device).  One kernel checks and loads all of them.
 * Refusals, each before any member's costs, deferred differences, delta or initial change is touched, bddmma_batch_last_error naming
 * the member: BDDMMA_ERR_STATE as for every batch call; BDDMMA_ERR_UNSUPPORTED for a member whose bddmma_fused_small_learned is 0;
 * BDDMMA_ERR_INVALID_ARGUMENT for a negative or non-finite value (naming the array too).  num_itr == 0 does nothing.  With device
 * inputs the host waits only for the check of the values and, where a member's initial change is still unset, for its two bounds.
 * (Named after bddmma_learned_iterations, which it is for every member; the bddmma_batch_ prefix is kept for the batch object's own calls.) */
int bddmma_learned_iterations_batch(bddmma_batch* b, const void* dist_weights, const void* omega_vec /* or NULL */, double omega,
                                    uint64_t num_itr, int on_device);
/* bddmma_learned_iterations_batch with the history of bddmma_learned_iterations: for every member i,
 * bddmma_learned_iterations(member i, w_i, .., num_itr, omega, 0.0, its part of sol_avg / lb_first_diff_avg / lb_second_diff_avg,
 * compute_history_for_itr, history_avg_beta, .., NULL) — or its omega_vec form.  The last min(num_itr, compute_history_for_itr) iterations
 * are tracked; the history step of a tracked iteration — the per-BDD bounds, the arg-min path of every BDD and the three moving averages —
 * runs inside the member's workgroup behind the iteration's backward sweep (csrc/kernels/small.hpp, HISTORY), where the per-member call
 * makes about fifteen launches per tracked iteration.  The iterations in front of the tracked ones run through the launches of
 * bddmma_learned_iterations_batch.
 * compute_history_for_itr == 0 IS bddmma_learned_iterations_batch; the three arrays may be NULL then.
 * Arrays: dist_weights / omega_vec as there.  sol_avg: the members' REAL[nr_layers] in the public layer order, one behind the other in
 * the members' order; lb_first_diff_avg / lb_second_diff_avg: the members' REAL[nr_bdds] in the order of bddmma_lower_bound_per_bdd, one
 * behind the other.  An entry the history does not reach keeps its content (compute_history_for_itr == 1 leaves both per-BDD arrays alone,
 * == 2 the second).  on_device is one flag for all arrays.  Host outputs pass through one staging buffer the batch owns with one host
 * synchronisation; device outputs are written in the order of the batch's stream.
 * Results: in float every result is bit-equal to the per-member call; in double bit-equal wherever no variable sits in more than two
 * BDDs, elsewhere within the summation order of the exchange (sol_avg holds 0 / 1 decisions: it differs only where two path costs tie to
 * within that rounding).  Every call starts its history afresh, as the per-member call does.
 * Everything bddmma_learned_iterations_batch promises holds: its refusals, its ordering, the checks of the weights and of omega, the
 * members' set-once initial bound change.  Added refusals: BDDMMA_ERR_INVALID_ARGUMENT for a NULL history array with
 * compute_history_for_itr > 0; BDDMMA_ERR_UNSUPPORTED, naming the member, where bddmma_fused_small_history is 0.  Every refusal is decided
 * before any member or output is touched. */
int bddmma_learned_iterations_history_batch(bddmma_batch* b, const void* dist_weights, const void* omega_vec /* or NULL */, double omega,
                                            uint64_t num_itr, void* sol_avg, void* lb_first_diff_avg, void* lb_second_diff_avg,
                                            uint64_t compute_history_for_itr, double history_avg_beta, int on_device);
/* bddmma_learned_iterations_history_batch with the stopping rule of bddmma_learned_iterations: for every member i,
 * bddmma_learned_iterations(member i, w_i, .., num_itr, omega, improvement_slope, its part of the three history arrays,
 * compute_history_for_itr, history_avg_beta, .., &iterations_done[i]) — or its omega_vec form.  iterations_done: host, uint64_t[bddmma_batch_size],
 * member i's count of iterations run in entry i.
 * The rule runs inside the member's workgroup behind every iteration (csrc/kernels/small.hpp, STOP): the bound is reduced in the shape of
 * bddmma_lower_bound, so it is that call's value bit for bit, and one lane applies the lines of the per-member loop in double — the set-once
 * initial change taken at the call's iteration 0 where it is unset; converged once the bound's change falls below improvement_slope times
 * it; stop when converged and the history has made compute_history_for_itr steps.  An iteration is tracked when it is one of the last
 * compute_history_for_itr of num_itr or an earlier iteration's test has set converged, so the tracked window is not known when a launch
 * starts.  A member that stops leaves through the exit exchange, as the per-member loop does; the call's launches — chunks of 32 iterations,
 * queued without waiting — return at once for it afterwards, and its state stays what its own last launch left.  The host waits once per
 * call, for the members' counts (with any host outputs), next to the wait for the check of the values; the first iteration needs no
 * launch of its own in this form, as the initial change is taken in the workgroup.
 * improvement_slope <= 0 or NaN never stops: that call IS bddmma_learned_iterations_history_batch, and every count is num_itr.
 * Results: as bddmma_learned_iterations_history_batch states them, counts included — in float, and in double wherever no variable sits in more
 * than two BDDs, every member's count, state, outputs and initial change are the per-member call's bit for bit; elsewhere in double a
 * decision that is borderline within the exchange's summation order may fall differently.
 * Everything bddmma_learned_iterations_history_batch promises holds: its refusals, its ordering, the check of the values in one launch, the
 * outputs' "an entry the history does not reach keeps its content", the set-once initial change.  Added refusals:
 * BDDMMA_ERR_INVALID_ARGUMENT for iterations_done == NULL; with improvement_slope > 0, BDDMMA_ERR_UNSUPPORTED, naming the member, where
 * bddmma_fused_small_stop is 0.  Every refusal is decided before any member, output or initial change is touched. */
int bddmma_learned_iterations_stop_batch(bddmma_batch* b, const void* dist_weights, const void* omega_vec /* or NULL */, double omega,
                                         uint64_t num_itr, double improvement_slope, void* sol_avg, void* lb_first_diff_avg,
                                         void* lb_second_diff_avg, uint64_t compute_history_for_itr, double history_avg_beta, int on_device,
                                         uint64_t* iterations_done /* host, [bddmma_batch_size] */);
/* bddmma_grad_learned_iterations(member i, its part of every array, ..) for every member i, with the same two iteration counts for all
 * members: ONE workgroup per member runs the whole call in one launch per kernel instantiation present — the tracked iterations once,
 * recording what their reverse reads, then the reverse (kernels/gradsmall.hpp) — where the per-member call issues about 25 launches and
 * copies per tracked iteration and synchronises the host once per member.
 * Arrays: every layer array is the members' REAL[nr_layers] in the public layer order, one behind the other in the members' order at
 * bddmma_batch_create.  grad_lo / grad_hi / grad_mm are in-out, grad_dist_weights_out is written.  grad_omega_out is
 * REAL[bddmma_batch_size] with a scalar omega — member i's own sum in entry i — and the concatenated per-layer array with omega_vec.
 * on_device is one flag for all arrays, as in bddmma_learned_iterations_batch.
 * Results: in float every result is bit-equal to the per-member call.  In double they are bit-equal wherever no variable sits in more than
 * two BDDs, and elsewhere within the summation order of the tracked iterations' exchange — the statement made above for the fused forward
 * iterations, whose kernel runs them here.
 * State contract: that of the per-member call.  On return every member's arc costs, deferred differences and delta are the entry values
 * bit for bit, and both sweep states are invalid.
 * Refusals, each decided before any member's state is touched, bddmma_batch_last_error naming the member and, for a bad value, the array:
 * BDDMMA_ERR_STATE as for every batch call; BDDMMA_ERR_UNSUPPORTED for a member whose bddmma_fused_small_learned is 0;
 * BDDMMA_ERR_INVALID_ARGUMENT for a null pointer (omega_vec excepted), a non-finite incoming gradient, or a negative or non-finite weight
 * or omega.  One launch checks all arrays; the member named is the first with an offending value, the array the first of its arrays in the
 * per-member call's order of checks (omega_vec, dist_weights, grad_lo, grad_hi, grad_mm).
 * track_grad_for_num_itr == 0: the in-out arrays stay unchanged, both outputs are zero-filled.
 * num_caches is accepted and does not change the result, as in the per-member contract; this form does not replay at all: it records every
 * tracked iteration's inputs once, 6 nr_layers + 2 slots values per member and tracked iteration, in a workspace the batch owns.  The
 * workspace is allocated before any member is touched (a failure leaves every member untouched), grows only when a call tracks more
 * iterations than any call before it, and is freed by bddmma_batch_destroy.
 * Ordering: that of the other batch calls; the host waits only for the one read of the argument check (and, with host arrays, for the
 * results). */
int bddmma_grad_learned_iterations_batch(bddmma_batch* b, const void* dist_weights, const void* omega_vec /* or NULL */, double omega,
                                         void* grad_lo, void* grad_hi, void* grad_mm, void* grad_dist_weights_out, void* grad_omega_out,
                                         uint64_t track_grad_after_itr, uint64_t track_grad_for_num_itr, uint64_t num_caches, int on_device);
/* bddmma_grad_learned_iterations(member i, its part of every array, .., track_grad_after_itr[i], track_grad_for_num_itr[i], ..) for every
 * member i: bddmma_grad_learned_iterations_batch with every member's own two counts — what the backward of
 * bddmma_learned_iterations_stop_batch needs, whose members stop at different iterations.  Still one workgroup per member and one launch
 * per kernel instantiation present for the call itself; the untracked iterations in front run in launches of up to 2^14 iterations, in
 * which a member that has run its own count returns at once.  The two count arrays are copied to the device once per call.
 * Arrays, grad_omega_out, on_device, results, state contract, ordering and workspace: as bddmma_grad_learned_iterations_batch states them,
 * for the members whose tracked count is above 0.  The workspace is sized for the largest tracked count of the call and grows only when
 * that exceeds every earlier call's, through either entry point.
 * A member with track_grad_for_num_itr[i] == 0 is left untouched, as its per-member call leaves it: no iteration runs for it (its
 * untracked count is not looked at), its arc costs, deferred differences and delta stay as they are, neither sweep state nor its cached
 * bound is invalidated, its parts of grad_lo / grad_hi / grad_mm are unchanged, its part of grad_dist_weights_out and its entry (with
 * omega_vec: its part) of grad_omega_out are zero.  Its arguments are checked like every member's.  All tracked counts 0: no member is
 * touched.
 * Refusals: those of bddmma_grad_learned_iterations_batch with its messages and its order of checks, and BDDMMA_ERR_INVALID_ARGUMENT for
 * a NULL count array, for a tracked count above 0xFFFFFFFF and, where the tracked count is above 0, for an untracked count above
 * 0xFFFFFFFF — bddmma_batch_last_error naming the first such member.  Each is decided before any member's state or any output is touched.
 * Every kernel instantiation of this call is built, so no member that bddmma_grad_learned_iterations_batch takes is refused here.
 * num_caches is accepted and ignored, as there. */
int bddmma_grad_learned_iterations_counts_batch(bddmma_batch* b, const void* dist_weights, const void* omega_vec /* or NULL */, double omega,
                                                void* grad_lo, void* grad_hi, void* grad_mm, void* grad_dist_weights_out, void* grad_omega_out,
                                                const uint64_t* track_grad_after_itr /* host, [bddmma_batch_size] */,
                                                const uint64_t* track_grad_for_num_itr /* host, [bddmma_batch_size] */, uint64_t num_caches,
                                                int on_device);
/* bddmma_set_solver_costs(member i, its part of lo / hi / mm, ..) followed by bddmma_backward_run(member i) for every member i: one
 * workgroup per member scatters the member's values and runs its plain backward sweep out of LDS, one launch per wave count present —
 * where the per-member call is three copies, three kernels and a host synchronisation, and leaves the costs-to-terminal stale, so that
 * the next batch call had to launch a backward sweep per member first.
 * Arrays: the members' REAL[nr_layers] in the public layer order, one behind the other in the members' order at bddmma_batch_create,
 * all on the host or all on the device (on_device).  Each of the three may be NULL: that part of the members' state is left as it is.
 * All three NULL: BDDMMA_OK, nothing is done.  No value is checked, as bddmma_set_solver_costs checks none.
 * State afterwards: that of the two per-member calls — arc costs, deferred differences, costs-to-terminal and the bound's partial sums
 * bit-equal to theirs, the backward state valid, the forward state invalid; delta and the costs-from-root are untouched.
 * Ordering: that of the other batch calls.  With device arrays the host does not wait at all; host arrays pass through one staging
 * buffer the batch owns (allocated before any member is touched, freed by bddmma_batch_destroy) with one host synchronisation.
 * Refusals: b == NULL is BDDMMA_ERR_INVALID_ARGUMENT; BDDMMA_ERR_STATE as for every batch call, every member left untouched.
 * (Named after the per-member calls, as bddmma_learned_iterations_batch is; likewise the three entries below.) */
int bddmma_set_solver_costs_batch(bddmma_batch* b, const void* lo /* or NULL */, const void* hi /* or NULL */, const void* mm /* or NULL */,
                                  int on_device);
/* bddmma_get_solver_costs(member i, its part of lo / hi / mm, ..) for every member i in one launch: the same array layout, the same
 * refusals, NULL outputs are skipped, results bit-equal to the per-member calls.  Device outputs are written in the order of the
 * batch's stream and the host does not wait (bddmma_stream_signal_batch orders a reader's stream behind them); host outputs pass
 * through the staging buffer with one host synchronisation.  No member's state changes. */
int bddmma_get_solver_costs_batch(bddmma_batch* b, void* lo /* or NULL */, void* hi /* or NULL */, void* mm /* or NULL */, int on_device);
/* bddmma_stream_wait / bddmma_stream_signal for the batch's own stream, on which every batch call runs: whatever a batch call queues
 * after bddmma_stream_wait_batch starts after everything queued on `hip_stream` so far; whatever is queued on `hip_stream` after
 * bddmma_stream_signal_batch starts after everything the batch's calls have queued so far.  One event the batch owns (timing disabled,
 * created on first use); neither waits on the host.  A caller whose work between the two is batch calls only needs this one pair instead
 * of a pair per member: every batch call orders itself against the members' streams. */
int bddmma_stream_wait_batch(bddmma_batch* b, void* hip_stream);
int bddmma_stream_signal_batch(bddmma_batch* b, void* hip_stream);
/* The tail of a training step's loss for every member at once (kernels/batchbound.hpp); named after the per-member calls they are.
 * Arrays: per-BDD arrays are the members' REAL[nr_bdds] in the order of bddmma_lower_bound_per_bdd, one behind the other in the members'
 * order at bddmma_batch_create; layer arrays are the members' REAL[nr_layers] in the public layer order, concatenated the same way.  One
 * on_device flag covers all arrays of a call.  Host arrays pass through a staging buffer the batch owns with one host synchronisation;
 * device arrays are written in the order of the batch's stream and the host does not wait (the gradient's argument check reads one
 * word back, once).  Results are bit-equal to the per-member calls in float and in double.
 * Refusals, each decided before any member or output is touched: b == NULL or a null array is BDDMMA_ERR_INVALID_ARGUMENT;
 * BDDMMA_ERR_STATE as for every batch call; whatever has to be allocated is allocated before any member is touched.
 *
 * bddmma_lower_bound_per_bdd_batch: bddmma_lower_bound_per_bdd(member i, its part of out, ..) for every member i in one launch.  Members
 * whose costs-to-terminal are stale get their own backward sweep first; afterwards the backward state is valid and nothing else has changed. */
int bddmma_lower_bound_per_bdd_batch(bddmma_batch* b, void* out, int on_device);
/* bddmma_grad_lower_bound_per_bdd(member i, its parts, smooth = 0, ..) for every member i: one workgroup per member, a wave per pack, runs
 * the arg-min path of every BDD out of LDS and writes grad_hi = x * g, grad_lo = (1 - x) * g per layer, g the BDD's entry of
 * grad_lb_per_bdd; one launch per wave count present.  A value of grad_lb_per_bdd that is not finite: BDDMMA_ERR_INVALID_ARGUMENT,
 * bddmma_batch_last_error naming the first offending member, the outputs untouched (one check launch covers all members).
 * State: as bddmma_lower_bound_per_bdd_batch — arc costs, deferred differences and delta are unchanged, and every getter returns
 * afterwards what it returns after the per-member call. */
int bddmma_grad_lower_bound_per_bdd_batch(bddmma_batch* b, const void* grad_lb_per_bdd, void* grad_lo_out, void* grad_hi_out, int on_device);
/* bddmma_distribute_delta(member i) for every member i in one launch.  Per member exactly the state that call leaves: the deferred
 * differences applied to the arc costs and cleared, a copy of them kept for a later bddmma_grad_distribute_delta(member i, ..), delta
 * zero, both sweep states invalid. */
int bddmma_distribute_delta_batch(bddmma_batch* b);
/* The min-marginal differences of every member and their gradient (kernels/batchmm.hpp), one launch per wave count present each: one
 * workgroup per member, a wave per pack.  Arrays, the on_device flag, host staging, device ordering and the refusals are those of the
 * three entry points above; results are bit-equal to the per-member calls in float and in double.
 *
 * bddmma_min_marginal_diff_batch: bddmma_min_marginal_diff(member i, its part of out, ..) for every member i.  Deferred differences are
 * not applied.  Members whose costs-to-terminal are stale get their own backward sweep first; the launch recomputes every member's
 * costs-from-root by a plain forward pass and stores them, so both sweep states are valid afterwards, as after the per-member call;
 * arc costs, deferred differences and delta are unchanged. */
int bddmma_min_marginal_diff_batch(bddmma_batch* b, void* out, int on_device);
/* bddmma_grad_min_marginal_diff(member i, its parts, ..) for every member i: the forward pass, then the two sweeps of that call on the
 * wave's pack (the same routing steps and layer folds, so the same tie rule and the same bits).  A value of grad_mm that is not finite:
 * BDDMMA_ERR_INVALID_ARGUMENT, bddmma_batch_last_error naming the first offending member and grad_mm, the outputs untouched (host
 * values are checked on the host, device values by one check launch for all members).  State: as bddmma_min_marginal_diff_batch. */
int bddmma_grad_min_marginal_diff_batch(bddmma_batch* b, const void* grad_mm, void* grad_lo_out, void* grad_hi_out, int on_device);
/* The log-sum-exp family of every member (kernels/batchsm.hpp), one launch per wave count present each: one workgroup per member, a wave
 * per pack, running the two sweeps of bddmma_sum_marginals on the wave's pack and the call's per-layer expression behind them.  Arrays,
 * the on_device flag, host staging, device ordering and the refusals are those of the entry points above; every output pointer is
 * required.  Layer arrays are in the unsorted layer order only (bddmma_get_primal_variable_index gives the variables); results are
 * bit-equal to the per-member calls in float and in double.  No costs-to-terminal are needed, so no member runs a sweep of its own first.
 * State of every member afterwards, as after the per-member calls: the stored costs-from-root and costs-to-terminal hold log-partition
 * values and both sweep states and the cached bound are invalid (the next call that needs them recomputes them); arc costs, deferred
 * differences and delta are unchanged.
 *
 * bddmma_sum_marginals_batch: bddmma_sum_marginals(member i, sorted 0, log_probs, NULL, its parts of sm0 and sm1, ..) for every member i. */
int bddmma_sum_marginals_batch(bddmma_batch* b, int log_probs, void* sm0, void* sm1, int on_device);
/* bddmma_smooth_solution(member i, its part of out, ..) for every member i: 0.5 on a layer no root-to-top path crosses. */
int bddmma_smooth_solution_batch(bddmma_batch* b, void* out, int on_device);
/* bddmma_grad_lower_bound_per_bdd(member i, its parts, smooth 1, ..) for every member i; grad_lb_per_bdd: the members' REAL[nr_bdds] one
 * behind the other.  A value of it that is not finite: BDDMMA_ERR_INVALID_ARGUMENT, bddmma_batch_last_error naming the first offending
 * member and grad_lb_per_bdd, members and outputs untouched (host values are checked on the host, device values by one check launch for
 * all members). */
int bddmma_grad_smooth_lower_bound_per_bdd_batch(bddmma_batch* b, const void* grad_lb_per_bdd, void* grad_lo_out, void* grad_hi_out, int on_device);
/* bddmma_run_solver(member, NULL, max_iter, tolerance, improvement_slope, time_limit, 0, &res[i]) for every member i: each member's tests
 * run inside its workgroup against its own control block and each stops on its own criterion; the host relaunches chunks of iterations
 * until every member has stopped or reached max_iter.  res (bddmma_batch_size entries, may be NULL): member i's iterations, bounds and
 * stop reason; `seconds` is the batch's wall time for all members.  The time limit is one clock for the whole batch. */
int bddmma_batch_run_solver(bddmma_batch* b, uint64_t max_iter, double tolerance, double improvement_slope, double time_limit,
                            bddmma_run_result* res);
/* bddmma_batch_iterations bracketed by hipEvents on the batch's stream, from its first launch to its last; *ms = elapsed device time.
 * Waits for the launches (the measurement counterpart of bddmma_time_iterations). */
int bddmma_batch_time_iterations(bddmma_batch* b, double omega, uint64_t n, double* ms);
/* bddmma_lower_bound_batch(b, out, 0) without the BDDMMA_ERR_STATE refusals of the members' states (the name of the first batch calls, kept) */
int bddmma_batch_lower_bounds(bddmma_batch* b, double* out);
/* bddmma_lower_bound(member i, &out[i]) for every member i, in one launch per wave count present (kernels/batchlb.hpp: one workgroup per
 * member, a wave per pack): a member whose costs-to-terminal are stale runs the plain backward sweep bddmma_lower_bound would run first
 * inside its workgroup, and wave 0 sums the member's partial sums in that call's order, so out[i] is bit-equal to it in float and in
 * double.  out: double[bddmma_batch_size] in the members' order at bddmma_batch_create.
 * on_device 0: out is a host array; the results arrive in a pinned buffer the batch owns and the host waits once.  Every member's cached
 * bound is set, as bddmma_lower_bound sets it.
 * on_device 1: out is a device array written on the batch's stream; the host does not wait and no member's cached bound is set.  The
 * ordering is that of the batch entry points above: the launch runs behind everything queued on every member's stream, and every
 * member's stream waits for it.
 * State of every member afterwards: its costs-to-terminal are valid (a later call runs no sweep for them).
 * Refusals, decided before any member or output is touched: b == NULL or out == NULL is BDDMMA_ERR_INVALID_ARGUMENT; BDDMMA_ERR_STATE as for
 * every batch call (an L-BFGS wrapper, profiling, a member inside run_solver; bddmma_batch_last_error names the member). */
int bddmma_lower_bound_batch(bddmma_batch* b, double* out, int on_device);

/* ---- primal rounding (src/bdd_solver/incremental_mm_agreement_rounding_cuda.cu:333-372) ------------------
 * incremental_mm_agreement_rounding_cuda(s, init_delta, delta_growth_rate, num_itr_lb, verbose, num_rounds):
 * perturbs the costs towards the sign of the min-marginal differences until they agree in every BDD.
 * sol: char[nr_variables]; *found = 1 if a solution was reconstructed.  The solver's costs stay perturbed
 * afterwards, as in the reference (bdd_solver.cpp:368 "TODO: reset solver state"). */
int bddmma_incremental_mm_agreement_rounding(bddmma_solver* s, bddmma_lbfgs* lbfgs_or_null, double init_delta,
                                             double delta_growth_rate, uint64_t num_itr_lb, uint64_t num_rounds,
                                             uint32_t seed, int verbose, char* sol, int* found);

/* One round of perturb_primal_costs (incremental_mm_agreement_rounding_cuda.cu:262-331): distribute_delta, min-marginals,
 * per-variable sign agreement (:29-65,76-108), sums (:110-134) and the perturbation {delta,0} / {0,delta} / random
 * (:136-205), then update_costs — through the L-BFGS wrapper (which drops its history, lbfgs_impl.h:343-364) when
 * `lbfgs_or_null` is given.  counts = #one, #zero, #equal, #inconsistent.  When all variables are `one` or `zero` the
 * solution is written to sol (char[nr_variables]) and the costs are left alone.  cost_delta_0 / cost_delta_1 (REAL[nr_variables],
 * host, may be NULL) receive the perturbation that was applied.  The random draws of the `equal` / `inconsistent` types
 * come from a counter-based hash of (variable, round, seed) instead of thrust::default_random_engine. */
int bddmma_perturb_primal_costs(bddmma_solver* s, bddmma_lbfgs* lbfgs_or_null, double cur_delta, uint32_t round_index, uint32_t seed,
                                uint32_t counts[4], char* sol, void* cost_delta_0, void* cost_delta_1);

/* Both for a batch (kernels/batchround.hpp: one workgroup per member, one launch per round and wave count present).  All arrays are on
 * the host.  sol, cost_delta_0 and cost_delta_1 are the members' nr_variables entries one behind the other in the members' order, counts
 * four per member, found / rounds one per member.  A call equals the per-member call — bddmma_perturb_primal_costs(member i, NULL, ..)
 * resp. bddmma_incremental_mm_agreement_rounding(member i, NULL, .., seed, 0, ..) — on every member, bit for bit in float and in
 * double: the outputs and every member's state afterwards.  A member's part of sol is written only where its min-marginals agreed, as
 * the per-member call writes it.  There is no L-BFGS form and no `verbose`.
 * Refusals, all decided before any member or output is touched: a null batch or a required null array (counts, sol; sol, found):
 * BDDMMA_ERR_INVALID_ARGUMENT; init_delta <= 0 or delta_growth_rate <= 0: BDDMMA_ERR_INVALID_ARGUMENT; BDDMMA_ERR_STATE as for every
 * batch call (an L-BFGS wrapper, profiling, a member inside run_solver; bddmma_batch_last_error names the member).
 *
 * bddmma_perturb_primal_costs_batch: one round on every member; cost_delta_0 / cost_delta_1 may be NULL. */
int bddmma_perturb_primal_costs_batch(bddmma_batch* b, double cur_delta, uint32_t round_index, uint32_t seed, uint32_t* counts, char* sol, void* cost_delta_0,
                                      void* cost_delta_1);
/* The loop for all members at once: the initial distribute_delta, then per round cur_delta = min(cur_delta * delta_growth_rate, 1e6), the
 * round over the members still looking and bddmma_batch_run_solver(num_itr_lb, 1e-7, 0.0001, no time limit) over the same.  A member
 * whose min-marginals agree is not touched again: its state is what its own call returns with.  found[i]: 0 or 1; rounds (may be NULL):
 * rounds[i] = the index of the round in which member i's agreement was seen, num_rounds where none was. */
int bddmma_incremental_mm_agreement_rounding_batch(bddmma_batch* b, double init_delta, double delta_growth_rate, uint64_t num_itr_lb, uint64_t num_rounds,
                                                   uint32_t seed, char* sol, int* found, uint64_t* rounds);

/* Per-BDD solutions, cost updates and the gradient of a cost perturbation for a batch (kernels/batchsol.hpp), one launch each; named
 * after the per-member calls they are.  Layer arrays are the members' [nr_layers] in the public layer order, per-variable arrays the
 * members' [nr_variables], each one behind the other in the members' order at bddmma_batch_create.  The on_device flag, host staging
 * (one buffer the batch owns, one host synchronisation), device ordering (the batch's stream; with device arrays the host does not wait,
 * except for the one word the gradient's argument check reads back) and the refusals are those of the batch entry points above: b == NULL
 * or a required null array is BDDMMA_ERR_INVALID_ARGUMENT, BDDMMA_ERR_STATE as for every batch call, each decided before any member or
 * output is touched and after whatever has to be allocated has been allocated.  Results and every member's state afterwards are
 * bit-equal to the per-member calls in float and in double.
 *
 * bddmma_bdds_solution_batch: bddmma_bdds_solution(member i, sorted 0, its part of sol, ..) for every member i: one workgroup per member,
 * a wave per pack, runs the arg-min path of every BDD out of LDS (the path pass of bddmma_grad_lower_bound_per_bdd_batch, so the same
 * tie rule) and writes the decision of every layer as a char, 0 where no node of the layer is on the path; one launch per wave count
 * present.  sol: char per layer; there is no sorted form.  Members whose costs-to-terminal are stale get their own backward sweep first;
 * afterwards the backward state is valid, the forward state what it was, and nothing else has changed. */
int bddmma_bdds_solution_batch(bddmma_batch* b, char* sol, int on_device);
/* bddmma_update_costs(member i, its part of lo, nr_variables(i), its part of hi, nr_variables(i), elem_precision, on_device) for every
 * member i in one launch: every layer of a variable gets lo[variable] / nr_bdds(variable) resp. hi[..], quotient and sum in double and
 * rounded once, as that call forms them.  lo / hi: full-length per-variable arrays of elem_precision (BDDMMA_F32 / BDDMMA_F64); either may
 * be NULL and that side is then untouched on every member; both NULL: BDDMMA_OK, nothing is done.  No value is checked, as
 * bddmma_update_costs checks none.  State afterwards, per member, that of the per-member call: both sweep states invalid and the cached
 * bound dropped; deferred differences and delta are untouched.  There is no L-BFGS form. */
int bddmma_update_costs_batch(bddmma_batch* b, const void* lo /* or NULL */, const void* hi /* or NULL */, int elem_precision, int on_device);
/* bddmma_grad_cost_perturbation(member i, its parts, ..) for every member i in one launch: per variable the sum of grad_lo resp. grad_hi
 * over its layers, in the order of the member's variable -> layer table, divided by max(nr_bdds, 1).  grad_lo / grad_hi: REAL per layer,
 * read where the caller has them; the outputs: REAL per variable.  A value of grad_lo or grad_hi that is not finite:
 * BDDMMA_ERR_INVALID_ARGUMENT, bddmma_batch_last_error naming the first offending member and, of its arrays, the first in the per-member
 * call's order (grad_lo, then grad_hi), the outputs untouched (host values are checked on the host, device values by one check launch
 * for all members).  No member's state is read beyond its layout, and none changes. */
int bddmma_grad_cost_perturbation_batch(bddmma_batch* b, const void* grad_lo, const void* grad_hi, void* grad_lo_pert_out, void* grad_hi_pert_out,
                                        int on_device);

/* ---- checkpoint (bdd_cuda_base.cu:1486-1550) ------------------------------ */
int bddmma_save(const bddmma_solver* s, const char* path);
int bddmma_load(bddmma_solver** out, int device, const char* path);

/* ---- ordering against other streams ---------------------------------------
 * bddmma_stream_wait: whatever is queued on the handle's stream after this call starts after everything queued on `hip_stream` (a
 * hipStream_t of the handle's device; NULL: the default stream) so far.  bddmma_stream_signal: the reverse — whatever is queued on
 * `hip_stream` after the call starts after everything queued on the handle's stream so far.  Both are an event record followed by a
 * stream wait on an event the handle owns (timing disabled, created on first use): neither waits on the host, and neither changes how
 * streams or queues are set up.  Call wait before handing the handle device buffers that `hip_stream` still writes, and signal before
 * `hip_stream` reads what the handle wrote or reuses memory the handle read.  A HIP failure returns BDDMMA_ERR_DEVICE. */
int bddmma_stream_wait(bddmma_solver* s, void* hip_stream);
int bddmma_stream_signal(bddmma_solver* s, void* hip_stream);

/* ---- measurement ---------------------------------------------------------- */
int bddmma_synchronize(bddmma_solver* s);
/* Kernel classes timed with hipEvents on the handle's stream when profiling is on. */
#define BDDMMA_K_FORWARD_MM 0
#define BDDMMA_K_BACKWARD_MM 1
#define BDDMMA_K_FINISH_DELTA 2
#define BDDMMA_K_OTHER 3
#define BDDMMA_K_COUNT 4
typedef struct bddmma_profile {
    uint64_t launches[BDDMMA_K_COUNT];
    double total_ms[BDDMMA_K_COUNT];
} bddmma_profile;
/* on = 0: off; on = n > 0: record events for every n-th iteration() (an event pair per launch costs ~4 us of
 * stream time, so n = 1 slows a 10.5 M-node iteration by ~14 %).  Resets the counters. */
int bddmma_set_profiling(bddmma_solver* s, int on);
int bddmma_get_profile(bddmma_solver* s, bddmma_profile* out);  /* synchronises */
/* Run n iterations bracketed by hipEvents on the handle's stream; *ms = elapsed device time. */
int bddmma_time_iterations(bddmma_solver* s, double omega, uint64_t n, double* ms);
/* Time `reps` back-to-back launches of one kernel class with hipEvents on the handle's stream
 * (kernel-level benchmarking; leaves the sweep state invalid).  kind: 0 forward_run sweep, 1 backward_run
 * sweep, 2 forward_mm sweep, 3 backward_mm sweep, 4 exchange reduce, 5 exchange broadcast, 8 / 9 forward / backward sum-marginal
 * sweep (bddmma_sum_marginals), 10 / 11 / 12 the root -> terminal / terminal -> root / both gradient sweeps (bddmma_grad_min_marginal_diff),
 * 13 - 17 the launch groups of one reversed learned iteration (bddmma_grad_learned_iterations with one tracked iteration, zero incoming
 * gradients and isotropic weights; the state is the entry state on return): 13 the reverse of the backward pass, 14 the reverse of the
 * forward pass, 15 the final sweep through T, 16 the copies and memsets that keep what the reverse reads, 17 its six elementwise launches;
 * 6 STREAM triad
 * a = b + s*c over three temporary arrays of BDDMMA_TRIAD_BYTES each (3 * BDDMMA_TRIAD_BYTES of HBM traffic
 * per launch), 7 STREAM copy a = b (2 * BDDMMA_TRIAD_BYTES per launch): the measured bandwidth ceilings of the
 * box the roofline is quoted next to. */
#define BDDMMA_TRIAD_BYTES (1ull << 30)
int bddmma_time_kernel(bddmma_solver* s, int kind, uint64_t reps, double* ms);
/* HBM bytes of the arrays the handle holds (its working set), and the bytes it has allocated for them: the
 * arrays are carved out of few large allocations, so allocated >= held (what a farm of many small solvers
 * must budget with). */
uint64_t bddmma_device_bytes(const bddmma_solver* s);
uint64_t bddmma_device_allocated_bytes(const bddmma_solver* s);

/* ---- host-only layout inspection (no GPU needed; used by the CPU test-suite) ------------- */
typedef struct bddmma_layout bddmma_layout;
int bddmma_layout_create(bddmma_layout** out, const bddmma_instruction* instr, const uint64_t* bdd_delims,
                         uint64_t n_bdds, const bddmma_options* opts);
/* The same for values of real_size bytes (4 / 8) on a chip with n_cus compute units and lds_bytes_per_cu of LDS each (0: MI355X, what
 * bddmma_layout_create assumes): the layout bddmma_create builds on such a device (bddmma_device_chip), e.g. a CPX / DPX partition. */
int bddmma_layout_create_for_chip(bddmma_layout** out, const bddmma_instruction* instr, const uint64_t* bdd_delims,
                                  uint64_t n_bdds, const bddmma_options* opts, int real_size, uint32_t n_cus, uint32_t lds_bytes_per_cu);
void bddmma_layout_destroy(bddmma_layout* l);
/* what / which: the codes listed in csrc/capi.cpp.  From 100 on they address the arrays of the checkpoint format by their id (csrc/layout.hpp:
 * LAY_*, ids 1-39): bddmma_layout_size(l, 100 + id) is the array's element count and bddmma_layout_copy(l, 100 + id, out) copies it
 * (element sizes as the format stores them: 8 bytes for ids 3, 36, 37; 1 for 13, 17, 21; 2 for 23, 33, 38, 39; 4 for the rest). */
uint64_t bddmma_layout_size(const bddmma_layout* l, int what);
int bddmma_layout_copy(const bddmma_layout* l, int which, void* out);
/* The per-lane records of the second-generation resident sweeps (derived data, csrc/layout.hpp: Res2Records) for values of real_size
 * bytes: info[0] = usable, [1] = number of 32-bit words (4 per record), [2] / [3] = the slot / layer capacity of a wave's LDS region the
 * offsets assume, [4] = hops of the longest pack.  words (info[1] entries) and rec_off (one per narrow pack) may be NULL to query sizes. */
int bddmma_layout_res2_records(const bddmma_layout* l, int real_size, uint32_t* info, uint32_t* words, uint32_t* rec_off);
/* The same for the records of the second-generation streaming sweeps (csrc/layout.hpp: StreamRecords): info[0] = usable, [1] = words. */
int bddmma_layout_stream_records(const bddmma_layout* l, int real_size, uint32_t* info, uint32_t* words, uint32_t* rec_off);
/* ... and the per-layer records of the third-generation streaming sweeps (csrc/layout.hpp: LayerRecords; 64 records of 4 words per hop):
 * info[0] = usable (packs of 128 slots, layers of <= 2 nodes, <= 64 layers per hop, no staggered packs), [1] = number of 32-bit words. */
int bddmma_layout_layer_records(const bddmma_layout* l, int real_size, uint32_t* info, uint32_t* words, uint32_t* rec_off);
/* ... and the lane codes of the lane-per-BDD solve sweeps, derived from those records (csrc/layout.hpp: LaneCodes; 64 lanes of 4 words per
 * structure template): info[0] = usable (every template lane-affine, <= 12 hops), [1] = number of 32-bit words, [2] = every template
 * lane-affine whatever its length.  code_off (one per narrow pack): the first lane record of the pack's template. */
int bddmma_layout_lane_codes(const bddmma_layout* l, int real_size, uint32_t* info, uint32_t* words, uint32_t* code_off);
/* The schedule of the atomic-free exchange (csrc/layout.hpp: SegExchange) for workgroups of `threads` and values of real_size bytes:
 * info[0] = usable, [1] = 32-bit words of `bin` (4 per bin), [2] = 16-bit words of `perm`, [3] = 32-bit words of `thr` (2 per bin and
 * thread), [4] / [5] / [6] = entries / slots / groups of the largest bin.  The arrays may be NULL to query sizes. */
int bddmma_layout_seg_exchange(const bddmma_layout* l, int threads, int real_size, uint32_t* info, uint32_t* bin, uint16_t* perm, uint32_t* thr);

#ifdef __cplusplus
}
#endif
#endif /* BDD_MMA_H */
