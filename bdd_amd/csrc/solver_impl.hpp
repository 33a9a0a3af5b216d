// solver_impl.hpp — the solver object behind the C-ABI (include/bdd_mma.h): template SolverT<REAL>, instantiated once per precision in its
// own translation unit (solver_f32.hip / solver_f64.hip, so that the two compile side by side; solver_base.hip has the precision-free part).
// gfx950 only; there is no CPU fallback: every compute entry point fails with BDDMMA_ERR_DEVICE when no HIP device is usable.
//
// Mirrors LPMP::bdd_cuda_parallel_mma<REAL> / bdd_cuda_base<REAL>
// (reference: src/bdd_solver/bdd_cuda_parallel_mma.cu, src/bdd_solver/bdd_cuda_base.cu).
#pragma once
#include <hip/hip_runtime.h>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <memory>
#include <string>
#include <thread>
#include <type_traits>
#include <vector>
#include "../../include/bdd_mma.h"
#include "kernels.hpp"
#include "layout.hpp"
#include "solver.hpp"

namespace bddmma {

// one step of a host spin-wait (the polled bounds, run_solver's reader): the core's pause / yield hint
static inline void cpu_relax()
{
#if defined(__x86_64__) || defined(__i386__)
    __asm__ __volatile__("pause");
#elif defined(__aarch64__)
    __asm__ __volatile__("yield");
#else
    std::this_thread::yield();
#endif
}


#define HIPCHK(expr)                                                                                   \
    do {                                                                                               \
        hipError_t e_ = (expr);                                                                        \
        if (e_ != hipSuccess) {                                                                        \
            err = std::string(#expr) + ": " + hipGetErrorString(e_);                                   \
            return BDDMMA_ERR_DEVICE;                                                                  \
        }                                                                                              \
    } while (0)

static inline uint32_t cdiv(uint64_t a, uint32_t b) { return (uint32_t)((a + b - 1) / b); }

// A run-time value as a compile-time constant: f(std::integral_constant<int, V>) for the candidate V that equals v, for the LAST candidate
// where none does (pack_width 64 / 128 / anything else, wpb 1 / 2 / 4 / anything else, ...: the kernels' instantiations).
template <int V0, int... Vs, class F>
decltype(auto) pick(uint32_t v, F&& f)
{
    if constexpr (sizeof...(Vs) == 0) return f(std::integral_constant<int, V0>{});
    else return v == (uint32_t)V0 ? f(std::integral_constant<int, V0>{}) : pick<Vs...>(v, static_cast<F&&>(f));
}

// A pull sweep (kernels/pull.hpp), described once: its kernel for the narrow, the wide and the huge packs (one function type: the leading
// arguments of every pull kernel, then the sweep's own TAIL), the bytes of a pack's arrays by value size and pack width (the dynamic LDS
// of the narrow and wide launches) and the huge packs' global scratch of that shape.  SolverT::launch_pull launches it.
template <typename REAL, typename... TAIL>
struct PullSweep {
    using Fn = void (*)(DevPtrs<REAL>, PackDev, const uint32_t*, const uint32_t*, uint32_t, unsigned char*, TAIL...);
    Fn narrow, wide, huge;
    size_t (*bytes)(size_t, uint32_t);
    unsigned char* scratch;
};

// ---------------------------------------------------------------------------------------------
// accumulator type of the exchange kernel's LDS tile (kernels.hpp: k_exchange_reduce); experiments: -DBDDMMA_EX_ACC=REAL
#ifndef BDDMMA_EX_ACC
#define BDDMMA_EX_ACC double
#endif
template <typename REAL> struct GradSmallItem;   // kernels/gradsmall.hpp
template <typename REAL> struct GradSmallIO;
template <typename REAL> struct SmallHistItem;   // kernels/smallhist.hpp
template <typename REAL> struct SmallStopItem;   // kernels/smallstop.hpp
template <typename REAL>
struct SolverT final : SolverBase {
    // device buffers
    uint32_t* d_nwords = nullptr;       // distinct pack word sequences (layout.hpp: narrow_words_unique)
    uint32_t* d_pack_word_off = nullptr;
    uint32_t n_nwords = 0;
    uint64_t* d_wwords = nullptr;
    REAL *d_F = nullptr, *d_T = nullptr, *d_lohi = nullptr;  // d_lohi: {lo, hi} per layer, interleaved
    REAL* d_lo = nullptr;  // = d_lohi     (stride 2)
    REAL* d_hi = nullptr;  // = d_lohi + 1 (stride 2)
    int32_t *d_var = nullptr, *d_bdd = nullptr, *d_nbdds = nullptr;
    uint32_t *d_var_ptr = nullptr, *d_var_layers = nullptr, *d_root_slot = nullptr;
    REAL* d_delta_var = nullptr;    // 2V: the solver's deferred delta_lo_hi_ (normalised), per variable; rebuilt lazily, see delta_var_valid
    bool delta_var_valid = true;    // false after an exchange that only wrote the broadcast pairs (d_delta_lay)
    REAL* d_delta_lay = nullptr;    // 2L: the same, broadcast to binned entry order (what the sweeps read)
    REAL* d_mm_binned = nullptr;    // L : deferred min-marginal differences in binned entry order
    REAL *d_delta_c = nullptr, *d_delta_lay_c = nullptr;  // scratch for the explicit forward_mm/backward_mm API
    // learned iterations (learned_iterations): the distribution weights in binned entry order, and the history's scratch — allocated on the
    // first call that needs them (dalloc: carved from the arena's rest or a further chunk; not part of the arena's size estimate in init)
    REAL* d_alpha_ent = nullptr;
    REAL* d_omega_lay = nullptr;   // omega_vec in layer order (the order of d_lohi): what the sweeps' OV instantiation reads
    REAL* d_hist = nullptr;        // last_sol [L], three per-BDD bounds [3 B], the change [B] and the previous change [B]
    REAL* d_hist_out = nullptr;    // device copies of the caller's host outputs: sol_avg [L], lb_first_diff_avg [B], lb_second_diff_avg [B]
    uint16_t* d_bvar = nullptr;
    uint32_t *d_evar = nullptr, *d_lpos = nullptr, *d_vpos = nullptr, *d_bin_ptr = nullptr;
    uint32_t *d_pack_group_ptr = nullptr, *d_grp_layer_off = nullptr, *d_grp_hop_end = nullptr;
    uint32_t *d_quad_round_ptr = nullptr, *d_cs_ptr = nullptr, *d_cs_entry = nullptr;
    uint16_t* d_cs_slot = nullptr;
    uint32_t wpb = 1;
    bool entry_by_var = false;  // entries ordered by (variable, bdd): exchange = k_exchange_byvar
    bool exch_small = false, exch_medium = false;
    // exchange as a fixed schedule (kernels.hpp: k_exchange_seg; layout.hpp: SegExchange) where every bin fits it
    bool use_seg = false;
    uint32_t *d_seg_bin = nullptr, *d_seg_thr = nullptr;
    uint16_t* d_seg_perm = nullptr;
    uint32_t seg_lds = 0, seg_tile_off = 0, seg_cnt_off = 0, seg_groups = 0;
    bool big = false;  // some array reaches 4 GiB (or variant_flags bit 14, for the tests): kernels.hpp DevPtrs::big
    uint32_t opts_variant = 0;  // bddmma_options.variant_flags (A/B switches of kernel variants)
    uint32_t n_cus = 256, lds_cu = 160 * 1024;  // hipDeviceProp of `device` (init)
    bool narrow_seg = false;  // some narrow pack has layers wider than two nodes: seg_min2 goes through LDS and needs scratch
    uint32_t vars_per_bin = 0, n_bins = 0, stage_cap = 0, stage_lds = 0, exch_lds = 0, n_narrow_layers = 0;
    double *d_lb_partial = nullptr, *d_lb = nullptr;
    double* h_lb = nullptr;  // pinned, device-visible: the reduce kernel writes the bound straight into host memory
    // h_lb[0]: lower_bound(); h_lb[1], h_lb[2]: the slots of lower_bound_enqueue; each with a sequence word the reduce kernel writes behind
    // the value, polled by the host (wait_bound)
    uint64_t *h_lb_seq = nullptr, *d_lb_seq = nullptr;
    uint64_t lb_seq_next = 0, lb_seq_expect[3] = {0, 0, 0};
    // the bound is a function of the costs-to-terminal, which only launch_bwd() writes: a second lower_bound() without a backward
    // sweep in between (L-BFGS reads the bound at the end of an iteration and again before its step search) costs nothing
    bool lb_cached = false;
    double lb_cache = 0.0;
    bool lb_slot_known[2] = {false, false}, lb_slot_enqueued[2] = {false, false};  // lower_bound_enqueue / _fetch: h_lb[1], h_lb[2]
    double lb_slot_value[2] = {0.0, 0.0};
    uint64_t lb_gen = 0, lb_slot_gen[2] = {0, 0};       // lb_gen counts the backward launches: a fetched slot of the current generation is the cached bound
    // device-resident run_solver (kernels.hpp: run_ctl_step)
    RunCtl* d_run_ctl = nullptr;
    RunHost *h_run = nullptr, *d_run_host = nullptr;  // pinned + its device address
    const uint32_t* run_stop = nullptr;               // &d_run_ctl->stop while run_plain() queues iterations, nullptr otherwise
    uint32_t run_iter = 0;                            // index of the iteration being queued by run_plain() (kernels.hpp: DevPtrs::run_iter)
    RunGate gate() const { return RunGate{run_stop, run_iter}; }
    RunStep run_step{};                               // {partials, count, ctl, host}: what the launch that ends an iteration gets
    REAL* d_x_layer = nullptr;    // net_solver_costs x = (hi - lo) + deferred mm in layer order, written by the backward solve sweeps once an L-BFGS wrapper uses them
    bool x_layer_valid = false;   // true after a backward solve sweep, false after anything else that writes arc costs or deferred values
    // every call that changes arc costs other than through a solve sweep: both sweep states and the x view are stale, and an L-BFGS wrapper's
    // pending bound is no longer "the bound of the current costs" (SolverBase::cost_epoch)
    void costs_changed()
    {
        fwd_valid = bwd_valid = lb_valid = x_layer_valid = false;
        ++cost_epoch;
    }
    CostQuot* d_cost_q = nullptr;      // update_costs: per-variable quotients (kernels.hpp: k_cost_quotients)
    uint8_t* d_cost_flags = nullptr;
    uint32_t* d_counts = nullptr;
    REAL *d_tmp0 = nullptr, *d_tmp1 = nullptr;        // per-layer scratch (min-marginals, sorted outputs)
    char* d_sol = nullptr;
    struct PackBufs {
        uint32_t *pack_hop_ptr = nullptr, *hop_node_off = nullptr, *hop_layer_off = nullptr;
        uint8_t* pack_steps = nullptr;
        uint16_t* hop_root = nullptr;  // narrow and wide packs (layout.hpp: PackSet::hop_root)
        uint32_t n_packs = 0;
    } nb_, wb_, hb_;  // narrow, wide, huge packs
    uint32_t wide_lds = 0, wide_threads = 256, wide_npt = 1;
    bool n3_nt = false;  // third-generation sweeps: the instantiation with non-temporal loads (double beyond the Infinity Cache's reach)
    bool beyond_cache = false;  // the arrays exceed what the Infinity Cache helps with (640 MiB)
    bool n12_nt = false;  // ... and of the first- (float) / second-generation (double) sweeps that run beyond 16 M slots: packs of 128 slots, 4 / 8 per workgroup
    uint32_t nt_potentials = 0;  // PackDev::nt_potentials (kernels.hpp: hop_store): double, footprint several times the Infinity Cache
    bool mixed = false;      // narrow (streaming) and wide solve sweeps in one launch (kernels.hpp: k_fwd_mixed / k_bwd_mixed)
    // Measured on the knapsack benchmark (3 604 narrow + 389 wide packs): backward 44.7 -> 37.4 us in one launch.  The forward sweeps
    // did not gain at first (56.1 -> 58.6 us: both kinds were bound by same-address LDS pushes into the sink entries); with those
    // pushes gone the one launch wins there too: 32.7 -> 26.3 us (float), 37.3 -> 30.2 us (double), 14.5 k -> 16.1 k it/s.
    bool mixed_fwd = true;   // variant_flags bit 1: forward narrow / wide solve sweeps as two launches
    uint32_t mixed_npt = 1, mixed_lds = 0;
    // (Running the wide launch on a second stream next to the narrow one was measured and dropped: the event fork / join costs ~10 us
    // per pass on this platform, more than the overlap returns — knapsack benchmark 8 990 -> 8 261 it/s.)
    // resident sweeps of the narrow packs (kernels.hpp: k_fwd_res / k_bwd_res)
    uint32_t *d_pack_hdr = nullptr, *d_quad_hdr = nullptr;
    bool use_res = false;
    uint32_t res_ns = 0, res_nl = 0, res_lds = 0;
    // second generation (kernels.hpp: k_fwd_res2 / k_bwd_res2): per-lane records of ready-made LDS offsets, derived from the layout here
    bool use_res2 = false;
    uint32_t *d_res2_rec = nullptr, *d_res2_rec_off = nullptr;
    uint32_t res2_n_words = 0, res2_lds = 0, res2_ns = 0, res2_nl = 0;
    // streaming solve sweeps on per-lane records (kernels.hpp: k_fwd_narrow2 / k_bwd_narrow2)
    bool use_narrow2 = false, narrow_gen = false;  // narrow_gen: layers wider than two nodes or staggered packs -> the kernels' general form
    uint32_t *d_srec = nullptr, *d_srec_off = nullptr;
    // the streaming sweeps of the narrow packs start from the resident headers where those hold (one stage group per pack, one round per quad, no
    // staggered packs; layout.hpp: struct Resident) — variant_flags bit 16: from the hop / group / round tables as before
    bool res_hdr_ok = false;
    const uint32_t* n2_hdr_pack() const { return res_hdr_ok ? d_pack_hdr : nullptr; }
    const uint32_t* n2_hdr_quad() const { return res_hdr_ok ? d_quad_hdr : nullptr; }
    uint32_t srec_words = 0;
    // instances that fit one workgroup: whole iterations in one launch (kernels/small.hpp: k_iterate_small)
    bool small_ok = false, small_rl = false;
    int small_nw = 1;
    uint32_t small_lds = 0;
    SmallDev small{};
    uint32_t* d_small_lds = nullptr;
    // learned iterations inside one launch (kernels/small.hpp: k_learned_small): the plain layout (records in LDS or not on this form's own
    // budget) + omega per layer.  The kernels live in solver_sl_f32.hip / _f64.hip: sl_prepare() resolves this
    // solver's and raises its dynamic-LDS limit on the first call that launches it.
    bool small_ln_ok = false, small_ln_rl = false, sl_ready = false;
    bool small_stop_ok = false;   // ... and the stopping rule (kernels/small.hpp: STOP): SMALL_STOP_LDS bytes of static LDS beside the learned form's
    bool small_hist_ok = false;   // the learned form with its history step (kernels/small.hpp: HISTORY); no LDS beyond the learned form's
    uint32_t small_ln_lds = 0;
    SmallDev small_ln{};
    SmallLearn<REAL> small_ln_arg{};
    // streaming solve sweeps, third generation: a lane per layer (kernels/narrow3.hpp: k_fwd_narrow3 / k_bwd_narrow3)
    bool use_narrow3 = false;
    // ... and inside iteration() with the potentials on chip (kernels/narrow4.hpp): 0, or the kernels' hop capacity (10 / 16)
    int onchip_hc = 0;
    uint32_t onchip_mode = 0;
    uint32_t *d_lrec = nullptr, *d_lrec_off = nullptr;
    uint32_t lrec_words = 0;
    // ... and in registers alone, a lane per BDD (kernels/narrow5.hpp): the lane codes of layout.hpp: LaneCodes in place of the records
    bool lane5 = false;
    uint32_t *d_lcode = nullptr, *d_lcode_off = nullptr;
    uint32_t lcode_words = 0;
    uint32_t huge_pack_width = 0;
    unsigned char* d_huge_scratch = nullptr;  // frontier arrays of the huge packs (global memory instead of LDS)

    std::vector<void*> allocs;

    ~SolverT() override
    {
        if (device >= 0) (void)hipSetDevice(device);
        for (void* p : allocs) (void)hipFree(p);
        if (h_lb) (void)hipHostFree(h_lb);
        if (h_lb_seq) (void)hipHostFree(h_lb_seq);
        if (h_run) (void)hipHostFree(h_run);
        if (d_run_ctl) (void)hipFree(d_run_ctl);
        for (auto& e : ev_pool) {
            (void)hipEventDestroy(e.first);
            (void)hipEventDestroy(e.second);
        }
        if (ev_t0) (void)hipEventDestroy(ev_t0);
        if (ev_t1) (void)hipEventDestroy(ev_t1);
        if (ev_order) (void)hipEventDestroy(ev_order);
        if (stream) (void)hipStreamDestroy(stream);
    }

    // Arena: the solver's arrays are carved out of few large allocations instead of one hipMalloc each (see arena_chunk below).
    struct Arena { char* base = nullptr; uint64_t size = 0, used = 0; };
    std::vector<Arena> arenas;
    uint64_t arena_chunk = 0;   // bytes per arena allocation (0: one hipMalloc per array, as before round 5)
    uint64_t arena_skew = 0;    // extra bytes between consecutive arrays
    template <typename T>
    int dalloc(T** p, uint64_t n)
    {
        // + 1 KiB: the resident sweeps copy in whole 1 KiB pieces and may read up to 1008 bytes past a pack's range (kernels.hpp: wave_copy_to_lds)
        const uint64_t bytes = std::max<uint64_t>(n, 1) * sizeof(T) + 1024;
        if (arena_chunk == 0) {
            HIPCHK(hipMalloc((void**)p, bytes));
            allocs.push_back(*p);
            dev_bytes += bytes;
            dev_alloc_bytes += bytes;
            return BDDMMA_OK;
        }
        const uint64_t need = (bytes + 4095) / 4096 * 4096 + arena_skew;
        if (arenas.empty() || arenas.back().used + need > arenas.back().size) {
            Arena a;
            a.size = std::max(arenas.empty() ? arena_chunk : std::min<uint64_t>(arena_chunk, 64ull << 20), need);   // what comes after the first chunk is small
            HIPCHK(hipMalloc((void**)&a.base, a.size));
            allocs.push_back(a.base);
            arenas.push_back(a);
            dev_alloc_bytes += a.size;
        }
        Arena& a = arenas.back();
        *p = reinterpret_cast<T*>(a.base + a.used);
        a.used += need;
        dev_bytes += bytes;
        return BDDMMA_OK;
    }
    struct DevField { const void* ptr = nullptr; uint64_t count = 0; };
    DevField dev_fields[LAYOUT_ARRAY_IDS];  // layout array id (layout.hpp: visit_layout_arrays) -> where it lives on the device
    template <typename T>
    int upload(T** p, const std::vector<T>& h, int id = 0)
    {
        int rc = dalloc(p, h.size());
        if (rc) return rc;
        if (!h.empty()) HIPCHK(hipMemcpyAsync(*p, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice, stream));
        if (id) dev_fields[id] = DevField{*p, h.size()};
        return BDDMMA_OK;
    }
    int download_layout(HostLayout& H) override
    {
        HIPCHK(hipSetDevice(device));
        H = HostLayout();
        set_layout_scalars(H, lay_scalars);
        hipError_t e = hipSuccess;
        visit_layout_arrays(H, [&](int id, auto& vec) {
            using T = typename std::remove_reference_t<decltype(vec)>::value_type;
            if (id == LAY_NODES_PER_HOP) { vec.assign(nodes_per_hop.begin(), nodes_per_hop.end()); return; }
            if (id == LAY_LAYERS_PER_HOP) { vec.assign(layers_per_hop.begin(), layers_per_hop.end()); return; }
            const DevField& f = dev_fields[id];
            vec.resize(f.count);
            if (f.count && e == hipSuccess) e = hipMemcpyAsync(vec.data(), f.ptr, f.count * sizeof(T), hipMemcpyDeviceToHost, stream);
        });
        if (e == hipSuccess) e = hipStreamSynchronize(stream);
        HIPCHK(e);
        return BDDMMA_OK;
    }
    int upload_packs(PackBufs& b, const PackSet& ps, int id0)
    {
        b.n_packs = ps.n_packs();
        int rc;
        if ((rc = upload(&b.pack_hop_ptr, ps.pack_hop_ptr, id0))) return rc;
        if ((rc = upload(&b.hop_node_off, ps.hop_node_off, id0 + LAY_SET_HOP_NODE_OFF))) return rc;
        if ((rc = upload(&b.hop_layer_off, ps.hop_layer_off, id0 + LAY_SET_HOP_LAYER_OFF))) return rc;
        if ((rc = upload(&b.pack_steps, ps.pack_steps, id0 + LAY_SET_PACK_STEPS))) return rc;
        return BDDMMA_OK;
    }

    int init_from_layout(const HostLayout& L, const bddmma_options* opts) override { return init(L, opts); }
    int init(const HostLayout& L, const bddmma_options* opts)
    {
        HIPCHK(hipSetDevice(device));
        {
            ChipInfo chip;
            std::string e;
            if (query_chip(device, &chip, e)) { err = e; return BDDMMA_ERR_DEVICE; }
            n_cus = chip.n_cus;
            lds_cu = chip.lds_bytes;
        }
        HIPCHK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
        HIPCHK(hipEventCreate(&ev_t0));
        HIPCHK(hipEventCreate(&ev_t1));
        n_vars = L.n_vars; n_bdds = L.n_bdds; n_layers = L.n_layers; n_hops = L.n_hops;
        n_input_nodes = L.n_input_nodes; n_slots = L.n_slots; pack_width = L.pack_width;
        wide_pack_width = L.wide_pack_width;
        nodes_per_hop = L.nodes_per_hop; layers_per_hop = L.layers_per_hop;
        h_nbdds = L.num_bdds_per_var; h_var_ptr = L.var_ptr;
        h_layer_var = L.layer_var; h_layer_bdd = L.layer_bdd;
        lay_scalars = layout_scalars(L);
        if (opts) saved_opts = *opts;
        deterministic = opts && opts->deterministic;
        {
            // Placement (round 5, tools/placement_probe.py, profiles/r05_placement.txt).  With one hipMalloc per array the iteration rate of
            // the SAME instance depends on where the arrays happened to land: the 10.5 M-node float instance runs at 8 810, 8 200, 7 500 or
            // 6 960 it/s from one solver object to the next in one process (stable for the life of an object; the sweeps alone always take
            // 38.7 / 39.8 us, inside the iteration loop 41 ... 57 us: what varies is how much of the 465 MB working set the 256 MiB Infinity
            // Cache keeps between launches) — the "noisy boxes" of rounds 3-4.  Carved out of ONE allocation, 4 KiB-aligned back to back,
            // the arrays gave 8 800-8 840 it/s in 40 of 40 solver objects on three boxes (a deliberate 1 MiB + 64 KiB between arrays: 8 000
            // in 10 of 10).  Beyond the cache's reach the contiguous placement is the consistently SLOWER one (21 M nodes 3 580 against
            // 3 590-3 800, 42 M 1 650 against 1 640-1 840 it/s), so the arena is used while the solver's arrays are expected to stay below
            // ~640 MiB; 1 M / 4.2 M nodes and double at 4.2 M: no difference.
            const uint64_t est = (uint64_t)n_slots * 2 * sizeof(REAL) + (uint64_t)n_layers * (5 * sizeof(REAL) + 24) + (uint64_t)n_vars * 24 +
                                 L.narrow_words_unique.size() * 4 + L.wide_words.size() * 8;
            // ~1.6 x: measured 1.45 x on the headline instance.  Small instances get a small chunk (rounded up to 2 MiB; it was floored at
            // 32 MiB through round 5: a farm of per-subproblem solvers then held 32 MiB each while bddmma_device_bytes reported ~1 MB).
            const uint64_t want = est + est / 2 + est / 8 + std::min<uint64_t>(16ull << 20, est / 2 + (1ull << 20));
            if (want <= (640ull << 20)) arena_chunk = (want + (2ull << 20) - 1) / (2ull << 20) * (2ull << 20);
#ifdef BDDMMA_EXPERIMENTAL  // make EXPERIMENTAL=1: BDDMMA_EXP_ARENA="<chunk MiB>,<bytes between arrays>" (0: one hipMalloc per array) — tools/exp_r05_aa.sh ... _ad.sh
            if (const char* ar = std::getenv("BDDMMA_EXP_ARENA")) {
                unsigned long long mib = 0, skew = 0;
                if (std::sscanf(ar, "%llu,%llu", &mib, &skew) >= 1) { arena_chunk = mib << 20; arena_skew = skew; }
            }
#endif
        }
        // Arrays of 4 GiB and more (>= 512 M slots or 256 M layers in double; the reference indexes nodes with int: 2^31).  The narrow sweeps
        // and the exchange address F / T / {lo, hi} and the entry arrays relative to their pack / bin (HopWindow, exchange_reduce_body) and
        // stage with 64-bit addresses then (DevPtrs::big); what still carries absolute 32-bit byte offsets is refused for such instances
        // below: wide and huge packs, the deterministic and by-variable exchanges, resident sweeps (small instances anyway), the L-BFGS
        // wrapper's vector passes.
        big = (uint64_t)n_slots * sizeof(REAL) >= 0xFFFF0000ull || 2ull * n_layers * sizeof(REAL) >= 0xFFFF0000ull || (opts && (opts->variant_flags & 0x4000u));
        if ((uint64_t)n_slots * sizeof(REAL) >= 0xFFFF0000ull || 2ull * n_layers * sizeof(REAL) >= 0xFFFF0000ull) {
            if (L.wide.n_packs() || L.huge.n_packs() || deterministic || L.ex.entry_by_var) {
                err = "instance too large for the 32-bit buffer offsets of this configuration: " + std::to_string(n_slots) + " node slots, " +
                      std::to_string(n_layers) + " layers of " + std::to_string(sizeof(REAL)) +
                      "-byte values (arrays of 4 GiB and more are supported for narrow packs with the binned exchange)";
                return BDDMMA_ERR_UNSUPPORTED;
            }
        }
        int rc;
        if ((rc = upload(&d_nwords, L.narrow_words_unique, LAY_NARROW_WORDS))) return rc;
        n_nwords = (uint32_t)L.narrow_words_unique.size();
        if ((rc = upload(&d_pack_word_off, L.narrow_word_off, LAY_NARROW_WORD_OFF))) return rc;
        if ((rc = upload(&d_wwords, L.wide_words, LAY_WIDE_WORDS))) return rc;
        if ((rc = upload(&d_var, L.layer_var, LAY_LAYER_VAR))) return rc;
        if ((rc = upload(&d_bdd, L.layer_bdd, LAY_LAYER_BDD))) return rc;
        if ((rc = upload(&d_nbdds, L.num_bdds_per_var, LAY_NUM_BDDS_PER_VAR))) return rc;
        if ((rc = upload(&d_var_ptr, L.var_ptr, LAY_VAR_PTR))) return rc;
        if ((rc = upload(&d_var_layers, L.var_layers, LAY_VAR_LAYERS))) return rc;
        if ((rc = upload(&d_root_slot, L.bdd_root_slot, LAY_BDD_ROOT_SLOT))) return rc;
        if ((rc = upload_packs(nb_, L.narrow, LAY_NARROW_PACK_HOP_PTR))) return rc;
        if (L.narrow.hop_root.size() + 1 != L.narrow.hop_node_off.size() && !L.narrow.hop_node_off.empty()) {
            err = "narrow hop_root table does not match the hop records";
            return BDDMMA_ERR_INVALID_ARGUMENT;
        }
        if ((rc = upload(&nb_.hop_root, L.narrow.hop_root, LAY_NARROW_HOP_ROOT))) return rc;
        if ((rc = upload_packs(wb_, L.wide, LAY_WIDE_PACK_HOP_PTR))) return rc;
        if (L.wide.hop_root.size() + 1 != L.wide.hop_node_off.size() && !L.wide.hop_node_off.empty()) {
            err = "wide hop_root table does not match the hop records";
            return BDDMMA_ERR_INVALID_ARGUMENT;
        }
        if ((rc = upload(&wb_.hop_root, L.wide.hop_root, LAY_WIDE_HOP_ROOT))) return rc;
        if ((rc = upload_packs(hb_, L.huge, LAY_HUGE_PACK_HOP_PTR))) return rc;
        huge_pack_width = L.huge_pack_width;
        if (hb_.n_packs && (rc = dalloc(&d_huge_scratch, (size_t)hb_.n_packs * wide_lds_bytes(sizeof(REAL), huge_pack_width, true)))) return rc;
        wide_slot_base = L.narrow_slots;
        if ((rc = dalloc(&d_F, n_slots))) return rc;
        if ((rc = dalloc(&d_T, n_slots))) return rc;
        if ((rc = dalloc(&d_lohi, 2 * n_layers + 2))) return rc;
        d_lo = d_lohi;
        d_hi = d_lohi + 1;
        if ((rc = dalloc(&d_mm_binned, n_layers))) return rc;
        if ((rc = dalloc(&d_delta_lay, 2 * n_layers))) return rc;
        if ((rc = dalloc(&d_delta_lay_c, 2 * n_layers))) return rc;
        if ((rc = upload(&d_evar, L.ex.evar, LAY_EVAR))) return rc;
        if ((rc = upload(&d_bvar, L.ex.bvar, LAY_BVAR))) return rc;
        if ((rc = upload(&d_lpos, L.ex.lpos, LAY_LPOS))) return rc;
        if ((rc = upload(&d_vpos, L.ex.vpos, LAY_VPOS))) return rc;
        if ((rc = upload(&d_bin_ptr, L.ex.bin_ptr, LAY_BIN_PTR))) return rc;
        if ((rc = upload(&d_pack_group_ptr, L.ex.pack_group_ptr, LAY_PACK_GROUP_PTR))) return rc;
        if ((rc = upload(&d_grp_layer_off, L.ex.grp_layer_off, LAY_GRP_LAYER_OFF))) return rc;
        if ((rc = upload(&d_grp_hop_end, L.ex.grp_hop_end, LAY_GRP_HOP_END))) return rc;
        if ((rc = upload(&d_quad_round_ptr, L.ex.quad_round_ptr, LAY_QUAD_ROUND_PTR))) return rc;
        if ((rc = upload(&d_cs_ptr, L.ex.cs_ptr, LAY_CS_PTR))) return rc;
        if ((rc = upload(&d_cs_entry, L.ex.cs_entry, LAY_CS_ENTRY))) return rc;
        if ((rc = upload(&d_cs_slot, L.ex.cs_slot, LAY_CS_SLOT))) return rc;
        wpb = L.ex.waves_per_block;
        entry_by_var = L.ex.entry_by_var;
        {   // balance of the narrow packs' hop counts over contiguous eighths of the pack sequence (see xcd_chunk)
            const uint32_t P = L.narrow.n_packs();
            if (P >= 64) {
                uint64_t part[8] = {0, 0, 0, 0, 0, 0, 0, 0}, total = 0;
                const uint32_t per = (P + 7) / 8;
                for (uint32_t p = 0; p < P; ++p) {
                    const uint32_t h = L.narrow.pack_hop_ptr[p + 1] - L.narrow.pack_hop_ptr[p];
                    part[std::min<uint32_t>(7, p / per)] += h;
                    total += h;
                }
                uint64_t mx = 0;
                for (uint64_t v : part) mx = std::max(mx, v);
                if (mx * 8 * 10 > total * 11) xcd_chunk_auto = 32;
            }
        }
        for (uint8_t st : L.narrow.pack_steps) narrow_seg = narrow_seg || st >= 2;
        vars_per_bin = L.ex.vars_per_bin; n_bins = L.ex.n_bins; stage_cap = L.ex.stage_cap;
        n_narrow_layers = L.ex.grp_layer_off.empty() ? 0 : L.ex.grp_layer_off.back();
        stage_lds = L.ex.waves_per_block * stage_cap * 2 * (uint32_t)sizeof(REAL);
        exch_lds = vars_per_bin * 2 * (uint32_t)sizeof(double);  // accumulators are double for both precisions
        // LDS of a narrow solve workgroup: the dynamic staging area + the kernel's static arrays (frontier F x2 and T per wave, the hop
        // offset windows) — k_fwd_narrow is the larger of the two.  Above the 64 KiB a launch gets by default the kernels need the
        // attribute (pack_width 256, double, 4 waves per block is ~67 KiB; raise_lds_limits at the end of init); above what a
        // CU has the options are refused here, not at the first sweep.
        const uint32_t narrow_static = L.ex.waves_per_block * (3 * (pack_width + 2) * (uint32_t)sizeof(REAL) + 2 * 64 * 4 + 2) + seg_bytes(L.ex.waves_per_block);
        if (exch_lds > lds_cu - 1024 || stage_lds + narrow_static > lds_cu - 1024) {
            err = "vars_per_bin / stage_cap / waves_per_block need more LDS than a CU has (" + std::to_string(stage_lds + narrow_static) + " B per sweep workgroup)";
            return BDDMMA_ERR_INVALID_ARGUMENT;
        }
        if ((rc = dalloc(&d_tmp0, n_layers))) return rc;
        if ((rc = dalloc(&d_tmp1, n_layers))) return rc;
        if ((rc = dalloc(&d_sol, n_layers))) return rc;
        if ((rc = dalloc(&d_delta_var, 2 * n_vars))) return rc;
        if ((rc = dalloc(&d_delta_c, 2 * n_vars))) return rc;
        if ((rc = dalloc(&d_lb_partial, nb_.n_packs + wb_.n_packs + hb_.n_packs))) return rc;
        HIPCHK(hipHostMalloc((void**)&h_lb, 3 * sizeof(double), hipHostMallocMapped | hipHostMallocCoherent));
        HIPCHK(hipHostGetDevicePointer((void**)&d_lb, h_lb, 0));
        HIPCHK(hipHostMalloc((void**)&h_lb_seq, 3 * sizeof(uint64_t), hipHostMallocMapped | hipHostMallocCoherent));
        HIPCHK(hipHostGetDevicePointer((void**)&d_lb_seq, h_lb_seq, 0));
        std::memset((void*)h_lb_seq, 0, 3 * sizeof(uint64_t));
        if ((rc = dalloc(&d_counts, 8))) return rc;   // 4: rounding_round; LOAD_MAX_ARRAYS: gr_load_device
        HIPCHK(hipMemsetAsync(d_F, 0, n_slots * sizeof(REAL), stream));
        HIPCHK(hipMemsetAsync(d_T, 0, n_slots * sizeof(REAL), stream));
        HIPCHK(hipMemsetAsync(d_lohi, 0, 2 * n_layers * sizeof(REAL), stream));
        HIPCHK(hipMemsetAsync(d_mm_binned, 0, n_layers * sizeof(REAL), stream));  // bdd_cuda_base.cu:45
        for (REAL* p : {d_delta_var, d_delta_c}) HIPCHK(hipMemsetAsync(p, 0, 2 * n_vars * sizeof(REAL), stream));
        for (REAL* p : {d_delta_lay, d_delta_lay_c}) HIPCHK(hipMemsetAsync(p, 0, 2 * n_layers * sizeof(REAL), stream));
        opts_variant = opts ? opts->variant_flags : 0u;
        mixed_fwd = (opts_variant & 2u) == 0;
        // measured in double: 7.1 M nodes (490 MB resident) lose 12 % with non-temporal potentials, 10.5 M (720 MB) gain 4 %
        beyond_cache = dev_bytes > (640ull << 20);   // array bytes (the working set), not arena capacity
        nt_potentials = (sizeof(REAL) == 8 && beyond_cache) ? 1u : 0u;
        exch_small = vars_per_bin <= EXS_MAX_VARS_PER_BIN;  // 256-thread workgroups (kernels.hpp: EXS_*)
        exch_medium = !exch_small && vars_per_bin <= EXM_MAX_VARS_PER_BIN;  // 512-thread workgroups (EXM_*)
        // `deterministic`: the scheduled reduction (kernels.hpp: k_exchange_seg; no atomics, fixed order) where every bin fits its tables
        // and the LDS — runs of <= 32 entries per thread, differences + pairs + counts of a bin in LDS —, else (or with variant_flags
        // bit 17) the per-variable gathers k_delta_gather + k_exchange_bcast.  Both sum in (variable, bdd) order: bit-equal results.
        if (deterministic && !entry_by_var && !big && !(opts_variant & 0x20000u)) {
            const uint32_t T = exch_small ? EXS_THREADS : exch_medium ? EXM_THREADS : EX_THREADS;
            SegExchange SE;
            build_seg_exchange(L, T, (uint32_t)sizeof(REAL), SE);
            constexpr uint32_t VEC = 16 / sizeof(REAL);
            if (SE.ok && SE.max_groups <= 4 && SE.max_entries <= (uint64_t)SEG_MAXL * T * VEC) {
                const uint32_t Z = (SE.max_entries + VEC - 1) / VEC * VEC;
                seg_tile_off = ((Z + 1) * (uint32_t)sizeof(REAL) + 15u) & ~15u;
                seg_cnt_off = seg_tile_off + SE.max_slots * 2u * (uint32_t)sizeof(REAL);
                seg_lds = (seg_cnt_off + SE.max_slots * 2u + 15u) & ~15u;
                if (seg_lds + 1024 <= lds_cu) {
                    if ((rc = upload(&d_seg_bin, SE.bin))) return rc;
                    if ((rc = upload(&d_seg_perm, SE.perm))) return rc;
                    if ((rc = upload(&d_seg_thr, SE.thr))) return rc;
                    use_seg = true;
                    seg_groups = SE.max_groups;
                }
            }
        }
        // resident sweeps: chosen when every narrow pack fits its wave's LDS slice and the instance is small enough that the streaming
        // kernels are latency-bound (few waves per SIMD); resident_sweeps = 1 turns them off, = 2 forces them on
        if ((rc = upload(&d_pack_hdr, L.res.pack_hdr, LAY_PACK_HDR))) return rc;
        if ((rc = upload(&d_quad_hdr, L.res.quad_hdr, LAY_QUAD_HDR))) return rc;
        res_hdr_ok = L.res.ok && nb_.n_packs > 0;
        if (nb_.n_packs && L.res.ok) {
            res_ns = (L.res.max_slots + 255) / 256 * 256;
            res_nl = (L.res.max_layers + 127) / 128 * 128;
            res_lds = wpb * stage_cap * 2 * (uint32_t)sizeof(REAL) + wpb * res_wave_bytes(sizeof(REAL), res_ns, res_nl);
            const uint32_t static_lds = wpb * (2 * (pack_width + 2) * (uint32_t)sizeof(REAL) + 512) + seg_bytes(wpb);
            const uint32_t mode = opts ? opts->resident_sweeps : 0;
            const bool fits = res_lds + static_lds <= lds_cu - 512;
            // automatic choice: small instances only — fewer than 3 waves per SIMD (2880 packs: with the round-2 kernels the resident sweeps
            // win by 3-6 % from 1 900 to 2 800 packs and lose 10 % at 3 125), all workgroups in flight at once with their LDS slices.  Measured (float, sweep fwd / bwd in us, streaming vs resident): 1 M nodes (1563 packs) 12.1 / 12.2 vs 11.4 / 10.5;
            // 2 M 18.5 / 19.1 vs 20.5 / 19.7; 4 M 27.3 / 25.5 vs 41.8 / 39.0; 10.5 M 50 / 45 vs 108 / 98 — with more waves per SIMD the
            // streaming kernels hide their latency and the resident ones only lose occupancy to their LDS footprint.
            const uint64_t wgs_per_cu = fits ? (lds_cu) / (res_lds + static_lds) : 0;
            const bool all_in_flight = (uint64_t)nb_.n_packs * 256 <= 2880ull * n_cus && (uint64_t)cdiv(nb_.n_packs, wpb) <= (uint64_t)n_cus * std::min<uint64_t>(wgs_per_cu, 2048 / (64 * wpb));
            use_res = fits && mode != 1 && (mode == 2 || all_in_flight) && !big;
            // Second generation (kernels.hpp: k_fwd_res2 / k_bwd_res2), packs of 64 slots with layers of <= 2 nodes: its LDS regions are sized in
            // whole 1 KiB pieces of REAL values (no node words in LDS).  Chosen, like the first, while the packs are (nearly) all in flight at
            // once.  Measured on random set cover (tools/sweep_res2.sh, profiles/r04_res2_sweep.txt), float, it/s streaming -> resident: 1.05 M
            // nodes (1 563 packs) 28.1 k -> 35.0 k, 1.6 M 21.4 k -> 26.1 k, 2.1 M 19.0 k -> 19.9 k, 3.1 M (4 688 packs, 1.4 x what the CUs' LDS holds
            // at once) 16.3 k -> 16.7 k, 4.2 M (128-slot streaming packs) 14.5 k -> 13.4 k; double gains only with every pack in flight.
            // variant_flags bit 11: first generation only.
            if (pack_width == 64 && !narrow_seg && mode != 1 && !big && !(opts && (opts->variant_flags & 0x800u))) {
                res2_ns = res2_slot_capacity((uint32_t)sizeof(REAL), L.res.max_slots);
                res2_nl = res2_layer_capacity((uint32_t)sizeof(REAL), L.res.max_layers);
                res2_lds = wpb * stage_cap * 2 * (uint32_t)sizeof(REAL) + wpb * res2_wave_bytes(sizeof(REAL), res2_ns, res2_nl);
                const uint64_t wgs2 = res2_lds + 256 <= lds_cu ? std::min<uint64_t>((lds_cu) / (res2_lds + 256), 2048 / (64 * wpb)) : 0;
                const uint64_t in_flight = (uint64_t)n_cus * wgs2 * wpb;  // packs the chip holds at once
                const bool auto_ok = sizeof(REAL) == 4 ? (uint64_t)nb_.n_packs * 100 <= in_flight * 145 : (uint64_t)nb_.n_packs <= in_flight;
                if (wgs2 && (mode == 2 || auto_ok)) {
                    Res2Records R2;
                    build_res2_records(L, sizeof(REAL), res2_ns, res2_nl, R2);
                    if (R2.ok && R2.rec.size() * sizeof(uint32_t) < (1ull << 31)) {
                        if ((rc = upload(&d_res2_rec, R2.rec))) return rc;
                        if ((rc = upload(&d_res2_rec_off, R2.rec_off))) return rc;
                        res2_n_words = (uint32_t)R2.rec.size();
                        use_res2 = use_res = true;
                    }
                }
            }
        }
        // streaming solve sweeps, second generation (kernels.hpp: k_fwd_narrow2 / k_bwd_narrow2): every narrow pack; the general form (GEN) where
        // layers are wider than two nodes or packs are staggered.  variant_flags bit 12: first generation; bit 13: records also where they are not
        // shared (the differential tests run the general form on random instances that way)
        uint32_t narrow2_static = 0;
        LaneCodes lane_codes;  // of the third generation's records, where those are built (float)
        if (nb_.n_packs && !use_res && !wb_.n_packs && !(opts && (opts->variant_flags & 0x1000u))) {
            StreamRecords SR;
            build_stream_records(L, sizeof(REAL), SR);
            narrow2_static = L.ex.waves_per_block * ((2 * pack_width + 2 + pack_width + 2) * (uint32_t)sizeof(REAL) + 3 * 64 * 4 + 64);
            // ... where the records are shared by the packs of a structure template (every row of a constraint family): 16 bytes per lane and hop
            // that are not shared cost more bandwidth than the instructions they save (general linear rows: k_fwd_mixed).  Limit: the records
            // hold at most a quarter of what the potentials of the narrow packs do.
            // ... and, in float, while the instance is small enough for the caches to help (tools/kbench.py, same-box A/B first / second
            // generation, it/s): 10.5 M nodes 8 190 / 8 540, 21 M 3 520 / 3 495, 42 M 1 605 / 1 596, 105 M 642 / 618 — once the sweeps run at
            // the HBM rate the instructions saved buy nothing and the records' L2 traffic costs a little; double: 4 273 / 4 353 and 339 / 357.
            const bool forced = opts && (opts->variant_flags & 0x2000u);
            const bool shared = forced || (SR.rec.size() * sizeof(uint32_t) <= (uint64_t)L.narrow_slots * sizeof(REAL) / 2 &&
                                           (sizeof(REAL) == 8 || n_slots <= 16'000'000ull));
            if (SR.ok && shared && stage_lds + narrow2_static + seg_bytes(L.ex.waves_per_block) <= 64 * 1024) {
                if ((rc = upload(&d_srec, SR.rec))) return rc;
                if ((rc = upload(&d_srec_off, SR.rec_off))) return rc;
                srec_words = (uint32_t)SR.rec.size();
                use_narrow2 = true;
                narrow_gen = narrow_seg;
                for (uint16_t r : L.narrow.hop_root) narrow_gen = narrow_gen || r != NO_ROOT;
            }
        }
        // streaming solve sweeps, third generation (kernels/narrow3.hpp): a lane per LAYER — packs of 128 slots whose layers have <= 2 nodes and whose
        // hops have <= 64 layers, no staggered packs, records shared like the second generation's.  At every size: what it saves — issue slots and bytes through the CU's vector-memory path — is what
        // bounds the sweeps with or without the caches' help (profiles/r05_hbm_only.txt).  variant_flags bit 18: second / first generation instead.
        if (nb_.n_packs && !use_res && !wb_.n_packs && !hb_.n_packs && !narrow_seg && pack_width == 128 && (L.ex.waves_per_block == 4 || L.ex.waves_per_block == 8) &&
            !(opts && (opts->variant_flags & 0x41000u))) {
            LayerRecords LR;
            build_layer_records(L, sizeof(REAL), LR);
            if constexpr (sizeof(REAL) == 4) build_lane_codes(L, sizeof(REAL), LR, lane_codes);
            const uint32_t n3_static = L.ex.waves_per_block * (4 * (128 + 128) * (uint32_t)sizeof(REAL) + 3 * 64 * 4);
            const bool forced = opts && (opts->variant_flags & 0x2000u);
            // ... and while the instance is small enough for the Infinity Cache to matter (same-box A/B against what the rules chose before,
            // tools/ab_n3.sh, it/s float / double: 4.2 M nodes 16 150 / 11 660 against 15 380 / 10 770; 10.5 M 8 850 / 4 390 against 8 530 /
            // 4 290; 21 M 3 480 / 1 838 against 3 555 / 1 879; 42 M 1 604 / 888 against 1 638 / 913): beyond, a shorter hop loop only
            // lengthens the staging phase of the same waves (profiles/r05_hbm_only.txt) and the eight-pack first / second generation stay ahead
            const bool shared = forced || (LR.rec.size() * sizeof(uint32_t) <= (uint64_t)L.narrow_slots * sizeof(REAL) / 2 && n_slots <= 16'000'000ull);
            if (LR.ok && shared && stage_lds + n3_static <= lds_cu - 1024) {
                if ((rc = upload(&d_lrec, LR.rec))) return rc;
                if ((rc = upload(&d_lrec_off, LR.rec_off))) return rc;
                lrec_words = (uint32_t)LR.rec.size();
                use_narrow3 = true;
                // double, footprint beyond the Infinity Cache's reach (the condition of the non-temporal stores): the instantiation that LOADS what a
                // sweep reads once — potentials, staging tables — non-temporally (profiles/r05_placement.txt #7: 10.5 M nodes +3.5 %)
                n3_nt = sizeof(REAL) == 8 && nt_potentials != 0;
            }
        }
        // First / second (double only) generation where the third stops — beyond 16 M slots, i.e. beyond the Infinity Cache's reach: the same
        // policy, the instantiation that loads potentials and staging tables non-temporally (round 5's build knobs BDDMMA_LD_POT_AUX / _TAB_AUX as a
        // template parameter; profiles/r06_nt_loads.txt, alternating with the library before, it/s: float 21 M nodes 3 705 / 3 837 -> 3 823 / 4 006,
        // 42 M 1 689 / 1 808 -> 1 836 / 1 891, 105 M 669 / 652 -> 671 / 661; double 21 M 1 938 / 2 090 -> 1 996 / 2 150, 42 M and 105 M +0-1 %).
        // Packs of 128 slots, 4 / 8 per workgroup, layers of at most two nodes, no staggered packs: what instances of that size have (the other
        // instantiations are not built).  variant_flags bit 20: whatever the footprint (the tests' way to these kernels).
        if (nb_.n_packs && !use_res && !use_narrow3 && !wb_.n_packs && !hb_.n_packs && !narrow_seg && !narrow_gen && pack_width == 128 &&
            (L.ex.waves_per_block == 4 || L.ex.waves_per_block == 8) && (beyond_cache || (opts && (opts->variant_flags & 0x100000u))))
#ifndef BDDMMA_EXP_NO_N12_NT   // A/B builds (tools/build_variant.sh)
            n12_nt = !use_narrow2 || sizeof(REAL) == 8;
#else
            n12_nt = false;
#endif
        nt_loads = n3_nt || n12_nt;
        // The solve sweeps of iteration() with F and T rebuilt in registers (kernels/narrow4.hpp): third-generation packs that start from the
        // resident headers and have at most 16 hops, float (the double form spills).  The smallest capacity that holds the longest pack
        // (bddmma_onchip_hops): 10 or 12 hops with both potentials on chip, 16 with F alone (the forward form spills beyond 12).
        // variant_flags bit 21: off (the tests' twin); bits 22 / 23: only T / only F on chip, where that pair is built (4 packs, 10 hops).
        if constexpr (sizeof(REAL) == 4) {
            if (use_narrow3 && res_hdr_ok && !n3_nt && !(opts && (opts->variant_flags & 0x200000u))) {
                uint32_t max_hops = 0;
                for (uint32_t p = 0; p < nb_.n_packs; ++p) max_hops = std::max(max_hops, L.res.pack_hdr[8 * (size_t)p + 5] & 0xFFFFu);
                onchip_hc = max_hops <= 10 ? 10 : max_hops <= 12 ? 12 : max_hops <= 16 ? 16 : 0;  // 10, 12: both on chip; 16: F only (mode 3)
                const uint32_t part = opts ? (opts->variant_flags >> 22) & 3u : 0u;
                if (onchip_hc == 16) onchip_mode = 3;
                if (part == 1 || part == 2) {
                    if (onchip_hc == 10 && wpb == 4) onchip_mode = part;
                    else onchip_hc = 0;
                }
                pot_on_chip = onchip_hc != 0;
                onchip_hops = onchip_hc;
                // ... walked in registers, a lane per BDD (kernels/narrow5.hpp), where both potentials are on chip and every structure
                // template is lane-affine (layout.hpp: LaneCodes; packs of BDDs ordered longest first).  variant_flags bit 24: the LDS walks.
                if ((onchip_hc == 10 || onchip_hc == 12) && onchip_mode == 0 && lane_codes.ok && !(opts && (opts->variant_flags & 0x1000000u))) {
                    if ((rc = upload(&d_lcode, lane_codes.words))) return rc;
                    if ((rc = upload(&d_lcode_off, lane_codes.code_off))) return rc;
                    lcode_words = (uint32_t)lane_codes.words.size();
                    lane5 = lane_sweeps = true;
                }
            }
        }
        if (wb_.n_packs) {
            // one workgroup per wide pack, thread t owns the nodes t + i * wide_threads of a hop (kernels.hpp: k_fwd_wide2)
            // two nodes of a hop per thread: half the wavefronts at the hop's two barriers and two independent chains per lane.  Wide-only
            // instance (25 000 rows of 18 variables, 15 M nodes): packs of 512 / 1024 slots with one node per thread 1 823 / 1 662 it/s, with
            // two 2 158 / 2 205, with four (1024 slots) 1 936
            wide_threads = std::min<uint32_t>(1024, std::max<uint32_t>(64, ((wide_pack_width + 1) / 2 + 63) / 64 * 64));
            wide_npt = (wide_pack_width + wide_threads - 1) / wide_threads;
            wide_npt = wide_npt <= 1 ? 1 : (wide_npt <= 2 ? 2 : 4);
            wide_lds = (uint32_t)wide2_lds_bytes(sizeof(REAL), wide_pack_width, true);
            if (wide_lds > lds_cu || wide_pack_width > 4096) {
                err = "wide_pack_width " + std::to_string(wide_pack_width) + " needs " + std::to_string(wide_lds) + " B of LDS (> 160 KiB)";
                return BDDMMA_ERR_UNSUPPORTED;
            }
        }
        // one launch for narrow + wide solve sweeps when the wide packs fit the narrow workgroup size (<= 4 nodes per thread) and their
        // LDS frontier does not cost the narrow workgroups their occupancy
        if (wb_.n_packs && nb_.n_packs && !use_res && !(opts && (opts->variant_flags & 1u))) {
            const uint32_t threads = 64 * wpb;
            const uint32_t npt = (wide_pack_width + threads - 1) / threads;
            const uint32_t narrow_dyn = stage_lds + seg_bytes(wpb);
            // (no launch attribute is set for the mixed kernels: static + dynamic LDS has to stay within the default 64 KiB)
            if (npt <= 4 && wide_lds <= narrow_dyn + 16 * 1024 && std::max(narrow_dyn, wide_lds) + narrow_static <= 64 * 1024) {
                mixed = true;
                mixed_npt = npt <= 1 ? 1 : (npt <= 2 ? 2 : 4);
                mixed_lds = std::max(narrow_dyn, wide_lds);
            }
        }
        // Whole iterations in one launch (kernels/small.hpp) where every pack fits one workgroup: the second-generation resident records (their
        // conditions: 64-slot packs, layers of <= 2 nodes, one stage group per pack and one staging round per quad), narrow packs only, the LDS-atomic
        // exchange's arithmetic (not the deterministic / by-variable orders), all of it within the CU's LDS.  variant_flags bit 19: off.
        if (use_res2 && res_hdr_ok && nb_.n_packs <= SMALL_MAX_PACKS && !wb_.n_packs && !hb_.n_packs && !deterministic && !entry_by_var && !big &&
            L.var_ptr.size() == n_vars + 1 && L.ex.vpos.size() == n_layers && !(opts && (opts->variant_flags & 0x80000u))) {
            const uint32_t np = nb_.n_packs;
            std::vector<uint32_t> lds_off(n_layers);
            uint32_t max_hops = 0;
            bool ok = true;
            for (uint32_t k = 0; k < (uint32_t)n_layers && ok; ++k) {
                const uint32_t l = L.var_layers[k];
                uint32_t p = 0;   // the pack whose layer range holds l (pack_hdr: [2] first layer, [3] layers)
                while (p < np && !(l >= L.res.pack_hdr[8 * (size_t)p + 2] && l < L.res.pack_hdr[8 * (size_t)p + 2] + L.res.pack_hdr[8 * (size_t)p + 3])) ++p;
                if (p == np || l - L.res.pack_hdr[8 * (size_t)p + 2] >= res2_nl) { ok = false; break; }
                lds_off[k] = (p * small_stage_stride(res2_nl) + (l - L.res.pack_hdr[8 * (size_t)p + 2])) * 2u * (uint32_t)sizeof(REAL);
            }
            for (uint32_t p = 0; p < np; ++p) max_hops = std::max(max_hops, L.res.pack_hdr[8 * (size_t)p + 5] & 0xFFFFu);
            small = SmallDev{};
            small.ns = res2_ns; small.nl = res2_nl; small.n_packs = np; small.wpb = wpb; small.n_quads = cdiv(np, wpb);
            small.n_vars = (uint32_t)n_vars; small.n_entries = (uint32_t)n_layers; small.rec_words = res2_n_words;
            small.rec_cap = (max_hops + 1u) * 1024u;   // + the spare KiB the forward sweep's one-hop-ahead read lands in behind the last hop
            uint32_t bytes = small_lds_bytes((uint32_t)sizeof(REAL), np, (uint32_t)n_vars, (uint32_t)n_layers, small);
            small_rl = bytes + 512 <= lds_cu;
            if (!small_rl) {
                small.rec_cap = 0;
                bytes = small_lds_bytes((uint32_t)sizeof(REAL), np, (uint32_t)n_vars, (uint32_t)n_layers, small);
            }
            if (ok && bytes + 512 <= lds_cu) {
                if ((rc = upload(&d_small_lds, lds_off))) return rc;
                small.pack_hdr = d_pack_hdr; small.quad_hdr = d_quad_hdr; small.rec = d_res2_rec; small.rec_off = d_res2_rec_off;
                small.var_ptr = d_var_ptr; small.var_lds = d_small_lds; small.var_ent = d_vpos;
                small_lds = bytes;
                small_nw = np <= 1 ? 1 : np <= 2 ? 2 : np <= 4 ? 4 : np <= 8 ? 8 : 16;
                small_ok = true;
                fused_small = true;
                small_ln = small;
                small_ln.rec_cap = (max_hops + 1u) * 1024u;
                uint32_t max_layers = 0;
                for (uint32_t p = 0; p < np; ++p) max_layers = std::max(max_layers, L.res.pack_hdr[8 * (size_t)p + 3]);
                small_ln_arg.om_stride = max_layers;
                auto learned_bytes = [&]() {
                    const uint32_t plain = small_lds_bytes((uint32_t)sizeof(REAL), np, (uint32_t)n_vars, (uint32_t)n_layers, small_ln);
                    return small_learn_lds_bytes((uint32_t)sizeof(REAL), np, res2_nl, max_layers, plain, small_ln_arg.off_om);
                };
                uint32_t lbytes = learned_bytes();
                small_ln_rl = lbytes + 512 <= lds_cu;
                if (!small_ln_rl) {
                    small_ln.rec_cap = 0;
                    lbytes = learned_bytes();
                }
                if (lbytes + 512 <= lds_cu) {
                    small_ln_lds = lbytes;
                    small_ln_ok = true;
                    fused_small_learned = true;
                    // The history step keeps its on-path marks in the 64 dummy entries behind a pack's costs-from-root and its decisions in
                    // the .y halves of the staging pairs, so it needs no LDS of its own; a thread per BDD holds the bounds.
                    small_hist_ok = small_hist_fits((uint64_t)n_bdds, (uint32_t)small_nw);
                    fused_small_history = small_hist_ok;
                    // The stopping rule keeps its working values in static LDS beside the dynamic area; a call may ask for a history, so
                    // the history form must be there too — and compiled without scratch (small_stop_built).
                    small_stop_ok = small_hist_ok && lbytes + SMALL_STOP_LDS + 512 <= lds_cu && small_stop_built<REAL>(small_nw, small_ln_rl);
                    fused_small_stop = small_stop_ok;
                }
            }
        }
        resolve_kernels();
        if ((rc = raise_lds_limits(kern))) return rc;
        solve_sweep_kind = !nb_.n_packs ? BDDMMA_SWEEPS_NONE : mixed ? BDDMMA_SWEEPS_MIXED : (use_res && use_res2) ? BDDMMA_SWEEPS_RESIDENT2 : use_res ? BDDMMA_SWEEPS_RESIDENT1
                           : use_narrow3 ? BDDMMA_SWEEPS_STREAMING3 : use_narrow2 ? BDDMMA_SWEEPS_STREAMING2 : BDDMMA_SWEEPS_STREAMING1;
        HIPCHK(hipStreamSynchronize(stream));
        return BDDMMA_OK;
    }

    // ---------------------------------------------------------------------------- launches
    DevPtrs<REAL> ptrs(const REAL* delta_lay) const
    {
        DevPtrs<REAL> d;
        d.nwords = d_nwords; d.n_nwords = n_nwords; d.wwords = d_wwords; d.wide_slot_base = wide_slot_base;
        d.F = d_F; d.T = d_T; d.lohi = d_lohi;
        d.delta_lay = delta_lay; d.mm_binned = d_mm_binned; d.lpos = d_lpos; d.cs_entry = d_cs_entry; d.cs_slot = d_cs_slot;
        d.n_slots = (uint32_t)n_slots; d.n_layers = (uint32_t)n_layers; d.n_narrow_layers = n_narrow_layers;
        d.lb_partial = d_lb_partial;
        d.mm0_out = d_tmp0; d.mm1_out = d_tmp1; d.sol_out = d_sol;
        d.x_layer = d_x_layer;  // nullptr until an L-BFGS wrapper asks for it (lbfgs_views)
        d.stop = run_stop;
        d.run_iter = run_iter;
        d.big = big ? 1u : 0u;
        return d;
    }
    PackDev pdev(const PackBufs& b, uint32_t lb_base, uint32_t seg_off = 0) const
    {
        const bool narrow_set = &b == &nb_;
        return PackDev{b.pack_hop_ptr, b.hop_node_off, b.hop_layer_off, b.pack_steps, b.hop_root, d_pack_word_off,
                       d_pack_group_ptr, d_grp_layer_off, d_grp_hop_end, d_quad_round_ptr, d_cs_ptr, stage_cap, seg_off, b.n_packs, lb_base,
                       nt_potentials, xcd_chunk(), narrow_set ? n2_hdr_pack() : nullptr, narrow_set ? n2_hdr_quad() : nullptr};
    }
    // dynamic LDS of a narrow launch with `w` waves per workgroup: `base` bytes of the kernel's own use, then (only when some pack has
    // layers wider than two nodes) the seg_min2 scratch, 128 REALs per wave
    uint32_t seg_bytes(uint32_t w) const { return narrow_seg ? w * 128 * (uint32_t)sizeof(REAL) : 0; }
    // block -> pack map of the narrow launches (kernels.hpp: block_to_pack): chunks of 32 workgroups interleaved over the XCDs
    // — chosen when contiguous eighths would be unbalanced (init: hop counts per eighth differ by more than 10 %: instances that mix
    // constraint families); homogeneous instances keep the contiguous map, which measured 1-3 % faster there (neighbouring packs share
    // more L2 lines).  variant_flags bit 7 forces the contiguous map, bit 8 the interleaved one.
    uint32_t xcd_chunk_auto = 0;
    uint32_t xcd_chunk() const { return xcd_chunk_auto; }
    uint32_t narrow_grid(uint32_t n_quads) const
    {
        const uint32_t c = xcd_chunk();
        return c ? 8 * c * cdiv(n_quads, 8 * c) : 8 * cdiv(n_quads, 8);
    }

    // ---------------------------------------------------------------------------- the kernel table
    // Which instantiation of a sweep, exchange or projection kernel this solver launches is a function of what init() has fixed
    // (pack_width, wpb, use_res, narrow_gen, ...).  resolve_kernels() evaluates that function once, at the end of init(), into typed
    // function pointers together with the dynamic LDS each is launched with; the launches below take both from the table, and
    // raise_lds_limits() sets the launch attribute of exactly the table's entries: what is prepared and what is launched is one object.
    // (A kernel family's parameter list depends on REAL only, so one pointer type serves all of its instantiations.)
    template <typename FN>
    struct Kern { FN fn = nullptr; uint32_t lds = 0; };
    using NarrowFn = void (*)(DevPtrs<REAL>, PackDev, REAL);
    using RecFn = void (*)(DevPtrs<REAL>, PackDev, const uint32_t*, const uint32_t*, uint32_t, REAL);  // second / third generation: + records
    using ResFn = void (*)(const uint32_t*, const uint32_t*, uint32_t, uint32_t, uint32_t, uint32_t, const uint32_t*, uint32_t, DevPtrs<REAL>, PackDev, REAL);
    using Res2Fn = void (*)(const uint32_t*, const uint32_t*, uint32_t, uint32_t, uint32_t, uint32_t, const uint32_t*, uint32_t, const uint32_t*,
                            const uint32_t*, uint32_t, DevPtrs<REAL>, PackDev, REAL);
    using WideFn = void (*)(DevPtrs<REAL>, PackDev, REAL, uint32_t);
    using HugeFn = void (*)(DevPtrs<REAL>, PackDev, REAL, uint32_t, unsigned char*);
    using MixedFn = void (*)(DevPtrs<REAL>, PackDev, PackDev, REAL, uint32_t);
    using ExFn = void (*)(const REAL*, const uint32_t*, const uint16_t*, const uint32_t*, uint32_t, uint32_t, uint32_t, uint32_t, const int32_t*, REAL*, REAL*,
                          RunStep, const REAL*);
    using SegFn = void (*)(const REAL*, const uint4*, const uint32_t*, uint32_t, const uint4*, const uint2*, uint32_t, uint32_t, REAL*, RunStep, const REAL*);
    using ProjFn = void (*)(REAL*, const uint32_t*, const uint16_t*, const int32_t*, uint32_t, uint32_t, uint32_t);
    using SmallFn = void (*)(SmallDev, DevPtrs<REAL>, PackDev, REAL, uint32_t, RunStep);
    using TransFn = void (*)(const REAL*, REAL*, PackDev, const uint32_t*, const uint16_t*, uint32_t, uint32_t, REAL*, REAL);
    using LincombFn = void (*)(LinComb, REAL*, PackDev, const uint32_t*, const uint16_t*, uint32_t, uint32_t);
    // one sweep (a direction and a MODE) over every pack family
    struct Sweep {
        // narrow packs: the one kernel the rules chose (resident 2 / resident 1 / on records / first generation), `w` packs per workgroup
        Res2Fn res2 = nullptr;
        ResFn res = nullptr;
        RecFn rec = nullptr;
        NarrowFn narrow = nullptr;
        uint32_t narrow_lds = 0, w = 1, seg_off = 0;    // seg_off: PackDev::seg_off, where the seg_min2 scratch starts
        const uint32_t *rec_tab = nullptr, *rec_off = nullptr;  // rec's records: the third generation's (d_lrec) or the second's (d_srec)
        uint32_t rec_words = 0;
        Kern<WideFn> wide;
        Kern<MixedFn> mixed;  // SOLVE, where init() admitted `mixed`: narrow + wide in one launch
        HugeFn huge = nullptr;
        bool reads_pot = true, stores_pot = true;  // SOLVE: the sweep reads T (forward) / F (backward) from memory, and stores F / T there
        const void* narrow_fn() const { return res2 ? (const void*)res2 : res ? (const void*)res : rec ? (const void*)rec : (const void*)narrow; }
    };
    struct Kernels {
        Sweep sweep[2][3];             // [backward][MODE]
        uint32_t ex_threads = 0;       // workgroup size of the binned exchange and of k_project_entries
        Kern<ExFn> ex[2], ex_w, ex_raw;  // LDS-atomic exchange: [RUN], WEIGHTED, and the raw sums of the explicit API
        Kern<SegFn> seg[2], seg_w;     // scheduled exchange (use_seg): [RUN], WEIGHTED
        Kern<ProjFn> project;
        Kern<SmallFn> small;           // small_ok: whole iterations in one launch
        Kern<TransFn> transpose[2];    // staged projection: [TO_LAYERS]
        Kern<LincombFn> lincomb[2];    // [the five-vector form]
        Sweep onchip[2];               // onchip_hc: iteration()'s solve sweeps with the potentials on chip, [backward]
    } kern;
    Sweep ov_sweep[2];  // [backward]: the SOLVE sweeps with omega per layer (OV), filled by ov_prepare()
    // OV: the instantiation that takes omega per layer from d_omega_lay (learned iterations with omega_vec), SOLVE only.  The <true> form is
    // named in solver_ov.hpp alone, so that those kernels compile in translation units of their own (solver_ov_f32.hip / solver_ov_f64.hip).
    template <int MODE, bool OV>
    Sweep resolve_sweep(bool bwd) const
    {
        constexpr bool SOLVE = MODE == FWD_SOLVE;  // == BWD_SOLVE
        static_assert(!OV || SOLVE, "omega per layer: solve sweeps only");
        Sweep s;
        if (hb_.n_packs) s.huge = bwd ? &k_bwd_wide<REAL, MODE, true, OV> : &k_fwd_wide<REAL, MODE, true, OV>;
        if (wb_.n_packs)
            s.wide = {pick<1, 2, 4>(wide_npt, [&](auto N) -> WideFn { return bwd ? &k_bwd_wide2<REAL, MODE, N.value, OV> : &k_fwd_wide2<REAL, MODE, N.value, OV>; }),
                      wide_lds};
        if (!nb_.n_packs) return s;
        if constexpr (!SOLVE) {
            // the other modes stage nothing: one pack per workgroup, the SEG = true form
            s.narrow = pick<64, 128, 256>(pack_width, [&](auto PW) -> NarrowFn {
                constexpr int R = PW.value / 64;
                return bwd ? &k_bwd_narrow<REAL, R, MODE, 1, true, false, false> : &k_fwd_narrow<REAL, R, MODE, 1, true, false, false>;
            });
            s.narrow_lds = seg_bytes(1);
        } else {
            // `wpb` packs per workgroup with cooperative staging.  Precedence, top to bottom: resident 2, resident 1, third generation (NT), second
            // generation NT, first generation NT (both: packs of 128 slots, 4 / 8 per workgroup), second generation general form, second
            // generation, first generation two-node form (SEG = false), first generation.
            s.w = wpb;
            s.seg_off = use_res ? res_lds : stage_lds;
            s.narrow_lds = (use_res && use_res2) ? res2_lds : s.seg_off + seg_bytes(wpb);
            pick<64, 128, 256>(pack_width, [&](auto PW) {
                pick<1, 2, 4, 8>(wpb, [&](auto W_) {
                    constexpr int R = PW.value / 64, W = W_.value, W48 = W == 8 ? 8 : 4;  // W48: the instantiations that exist for 4 / 8 only
                    const bool w48 = W == 4 || W == 8;
                    if (use_res && use_res2) s.res2 = bwd ? &k_bwd_res2<REAL, W, OV> : &k_fwd_res2<REAL, W, OV>;
                    else if (use_res) s.res = bwd ? &k_bwd_res<REAL, R, W, OV> : &k_fwd_res<REAL, R, W, OV>;
                    else if (use_narrow3 && w48) {
                        s.rec = bwd ? &k_bwd_narrow3<REAL, W48, false, OV> : &k_fwd_narrow3<REAL, W48, false, OV>;
                        if constexpr (sizeof(REAL) == 8)
                            if (n3_nt) s.rec = bwd ? &k_bwd_narrow3<REAL, W48, true, OV> : &k_fwd_narrow3<REAL, W48, true, OV>;
                        s.rec_tab = d_lrec; s.rec_off = d_lrec_off; s.rec_words = lrec_words;
                    } else if (use_narrow2) {
                        if (n12_nt && R == 2 && w48) s.rec = bwd ? &k_bwd_narrow2<REAL, 2, W48, false, sizeof(REAL) == 8, OV> : &k_fwd_narrow2<REAL, 2, W48, false, sizeof(REAL) == 8, OV>;
                        else if (narrow_gen) s.rec = bwd ? &k_bwd_narrow2<REAL, R, W, true, false, OV> : &k_fwd_narrow2<REAL, R, W, true, false, OV>;
                        else s.rec = bwd ? &k_bwd_narrow2<REAL, R, W, false, false, OV> : &k_fwd_narrow2<REAL, R, W, false, false, OV>;
                        s.rec_tab = d_srec; s.rec_off = d_srec_off; s.rec_words = srec_words;
                    } else if (n12_nt && R == 2 && w48) s.narrow = bwd ? &k_bwd_narrow<REAL, 2, MODE, W48, false, true, OV> : &k_fwd_narrow<REAL, 2, MODE, W48, false, true, OV>;
                    else if (!narrow_seg) s.narrow = bwd ? &k_bwd_narrow<REAL, R, MODE, W, false, false, OV> : &k_fwd_narrow<REAL, R, MODE, W, false, false, OV>;
                    else s.narrow = bwd ? &k_bwd_narrow<REAL, R, MODE, W, true, false, OV> : &k_fwd_narrow<REAL, R, MODE, W, true, false, OV>;
                });
            });
            if (mixed)
                s.mixed = {pick<64, 128, 256>(pack_width, [&](auto PW) {
                               return pick<1, 2, 4, 8>(wpb, [&](auto W) {
                                   return pick<1, 2, 4>(mixed_npt, [&](auto N) -> MixedFn {
                                       constexpr int R = PW.value / 64;
                                       return bwd ? &k_bwd_mixed<REAL, R, W.value, N.value, OV> : &k_fwd_mixed<REAL, R, W.value, N.value, OV>;
                                   });
                               });
                           }),
                           mixed_lds};
        }
        return s;
    }
    // k_fwd_narrow4 / k_bwd_narrow4 (float): the pair that keeps both potentials on chip for 4 / 8 packs per workgroup of <= 10 and of <= 12
    // hops; the backward kernel that rebuilds F and stores T for packs of <= 16 hops (the forward form, which keeps the four gathered child
    // potentials of every hop in registers, fits 12 hops at 126 VGPRs but spills at 14 and 16: there the third generation's forward sweep
    // stays); the pairs that keep one potential (variant_flags bits 22, 23: the decomposition of NOTES round 10) for the
    // headline's 4 packs and 10 hops
    RecFn onchip_fn(bool bwd, bool rebuild, bool store) const
    {
        if (lane5)  // k_fwd_narrow5 / k_bwd_narrow5: capacity 10 or 12, both potentials on chip (the rule of init())
            return pick<4, 8>(wpb, [&](auto W) -> RecFn {
                if (onchip_hc == 12) return bwd ? &k_bwd_narrow5<REAL, W.value, 12> : &k_fwd_narrow5<REAL, W.value, 12>;
                return bwd ? &k_bwd_narrow5<REAL, W.value, 10> : &k_fwd_narrow5<REAL, W.value, 10>;
            });
        if (onchip_hc == 16) return pick<4, 8>(wpb, [&](auto W) -> RecFn { return &k_bwd_narrow4<REAL, W.value, 16, true, true>; });
        if (onchip_hc == 12)
            return pick<4, 8>(wpb, [&](auto W) -> RecFn {
                return bwd ? &k_bwd_narrow4<REAL, W.value, 12, true, false> : &k_fwd_narrow4<REAL, W.value, 12, true, false>;
            });
        if (rebuild && !store)
            return pick<4, 8>(wpb, [&](auto W) -> RecFn {
                return bwd ? &k_bwd_narrow4<REAL, W.value, 10, true, false> : &k_fwd_narrow4<REAL, W.value, 10, true, false>;
            });
        if (rebuild) return bwd ? &k_bwd_narrow4<REAL, 4, 10, true, true> : &k_fwd_narrow4<REAL, 4, 10, true, true>;
        return bwd ? &k_bwd_narrow4<REAL, 4, 10, false, false> : &k_fwd_narrow4<REAL, 4, 10, false, false>;
    }
    // everything but the OV sweeps; called once, at the end of init()
    void resolve_kernels()
    {
        for (int bwd = 0; bwd < 2; ++bwd) {
            kern.sweep[bwd][FWD_PLAIN] = resolve_sweep<FWD_PLAIN, false>(bwd);
            kern.sweep[bwd][FWD_SOLVE] = resolve_sweep<FWD_SOLVE, false>(bwd);
            kern.sweep[bwd][FWD_SOLUTION] = resolve_sweep<FWD_SOLUTION, false>(bwd);  // backward: BWD_MARGINALS
        }
        if (onchip_hc) {
            // the third generation's launch (grid, staging area, records) with the kernels of kernels/narrow4.hpp.  onchip_mode: 0 both
            // potentials on chip, 1 T only (the forward sweep still stores F, the backward one reads it), 2 F only, 3 F only behind the third
            // generation's own forward sweep (packs of 11-16 hops)
            for (int bwd = 0; bwd < 2; ++bwd) {
                Sweep s = kern.sweep[bwd][FWD_SOLVE];
                if (onchip_mode == 3 && !bwd) { kern.onchip[0] = s; continue; }
                const bool rebuild = onchip_mode == 0 || (onchip_mode == 1) == !bwd;  // forward rebuilds T, backward F
                const bool store = onchip_mode != 0 && rebuild;  // the pairs that keep one potential on chip store the other one's partner: <1, 1> with <0, 0>
                if constexpr (sizeof(REAL) == 4) s.rec = onchip_fn(bwd, rebuild, onchip_mode == 3 || store);
                if (lane5) { s.rec_tab = d_lcode; s.rec_off = d_lcode_off; s.rec_words = lcode_words; }
                s.reads_pot = !rebuild;
                s.stores_pot = onchip_mode == 3 || store;
                kern.onchip[bwd] = s;
            }
        }
        kern.ex_threads = exch_small ? EXS_THREADS : exch_medium ? EXM_THREADS : EX_THREADS;
        pick<EXS_THREADS, EXM_THREADS, EX_THREADS>(kern.ex_threads, [&](auto T_) {
            constexpr int T = T_.value, U = T == EXS_THREADS ? EXS_UNROLL : T == EXM_THREADS ? EXM_UNROLL : EX_UNROLL,
                          N = T == EXS_THREADS ? EXS_NPT : T == EXM_THREADS ? EXM_NPT : EX_NPT;
            kern.ex[0] = {&k_exchange_reduce<REAL, BDDMMA_EX_ACC, EX_ITER, T, U, N, false>, exch_lds};
            kern.ex[1] = {&k_exchange_reduce<REAL, BDDMMA_EX_ACC, EX_ITER, T, U, N, true>, exch_lds};          // run_plain()'s
            kern.ex_w = {&k_exchange_reduce<REAL, BDDMMA_EX_ACC, EX_ITER, T, U, N, false, true>, exch_lds};    // learned_iterations()'s
            kern.project = {&k_project_entries<REAL, T>, vars_per_bin * (uint32_t)sizeof(double)};
            if (use_seg)
                pick<2, 4>(seg_groups <= 2 ? 2 : 4, [&](auto G) {
                    kern.seg[0] = {&k_exchange_seg<REAL, T, G.value, false>, seg_lds};
                    kern.seg[1] = {&k_exchange_seg<REAL, T, G.value, true>, seg_lds};
                    kern.seg_w = {&k_exchange_seg<REAL, T, G.value, false, true>, seg_lds};
                });
        });
        kern.ex_raw = {&k_exchange_reduce<REAL, BDDMMA_EX_ACC, EX_RAW>, exch_lds};
        if (small_ok)
            kern.small = {pick<1, 2, 4, 8, 16>(small_nw, [&](auto NW) -> SmallFn {
                              return small_rl ? &k_iterate_small<REAL, NW.value, true> : &k_iterate_small<REAL, NW.value, false>;
                          }),
                          small_lds};
        if (n_narrow_layers)
            pick<1, 2, 4, 8>(wpb, [&](auto W) {
                const uint32_t lds = wpb * stage_cap * (uint32_t)sizeof(REAL);
                kern.transpose[0] = {&k_stage_transpose<REAL, W.value, 0>, lds};
                kern.transpose[1] = {&k_stage_transpose<REAL, W.value, 1>, lds};
                kern.lincomb[0] = {&k_stage_lincomb<REAL, W.value, 0>, lds};
                kern.lincomb[1] = {&k_stage_lincomb<REAL, W.value, 5>, lds};
            });
    }
    // The dynamic-LDS limit (launch attribute) of table entries.  One rule: every entry that is launched with dynamic LDS gets exactly those
    // bytes as its limit, whatever their number — a limit is not a reservation, and "only above the default 64 KiB" would have to know each
    // kernel's static LDS as well.  The mixed kernels alone get none: init() admits `mixed` only where static + dynamic LDS stay within 64 KiB.
    int raise_lds_limit(const void* fn, uint32_t lds)
    {
        if (fn && lds) HIPCHK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        return BDDMMA_OK;
    }
    template <typename FN>
    int raise_lds_limit(const Kern<FN>& k) { return raise_lds_limit(reinterpret_cast<const void*>(k.fn), k.lds); }
    int raise_lds_limits(const Sweep& s)
    {
        if (int rc = raise_lds_limit(s.narrow_fn(), s.narrow_lds)) return rc;
        return raise_lds_limit(s.wide);
    }
    int raise_lds_limits(const Kernels& k)
    {
        int rc = BDDMMA_OK;
        for (const auto& dir : k.sweep)
            for (const Sweep& s : dir)
                if ((rc = raise_lds_limits(s))) return rc;
        if (onchip_hc)
            for (const Sweep& s : k.onchip)
                if ((rc = raise_lds_limits(s))) return rc;
        for (const auto* e : {&k.ex[0], &k.ex[1], &k.ex_w, &k.ex_raw})
            if ((rc = raise_lds_limit(*e))) return rc;
        for (const auto* e : {&k.seg[0], &k.seg[1], &k.seg_w})
            if ((rc = raise_lds_limit(*e))) return rc;
        for (const auto* e : {&k.transpose[0], &k.transpose[1]})
            if ((rc = raise_lds_limit(*e))) return rc;
        for (const auto* e : {&k.lincomb[0], &k.lincomb[1]})
            if ((rc = raise_lds_limit(*e))) return rc;
        if ((rc = raise_lds_limit(k.project))) return rc;
        return raise_lds_limit(k.small);
    }

    int ov_prepare();  // fills ov_sweep and raises its limits (solver_ov.hpp)
    // the learned one-workgroup kernels (solver_sl.hpp): this solver's instantiation, and the batch form's for a (waves, records in LDS) pair
    using SmallLnFn = void (*)(SmallDev, DevPtrs<REAL>, PackDev, SmallLearn<REAL>, REAL, uint32_t);
    using SmallLnBatchFn = void (*)(const SmallLearnItem<REAL>*, REAL, uint32_t, uint32_t);
    Kern<SmallLnFn> small_ln_kern;
    int sl_prepare();
    static SmallLnBatchFn sl_batch_fn(int nw, bool rl);
    // The backward of the learned iterations for a batch (kernels/gradsmall.hpp; BatchT::grad_learned_iterations): the kernels live in
    // solver_gs_f32.hip / _f64.hip, a translation unit of their own as the ones above.
    using GradSmallFn = void (*)(const GradSmallItem<REAL>*, REAL, uint32_t, uint32_t, GradSmallIO<REAL>);
    using GradSmallLoadFn = void (*)(const GradSmallItem<REAL>*, GradSmallIO<REAL>, uint32_t*);
    static GradSmallFn gs_batch_fn(int nw, bool rl);
    static GradSmallLoadFn gs_load_fn();
    // ... with per-member counts (BatchT::grad_learned_iterations_counts): the untracked iterations in front, and the call itself
    using GradSmallUntrackedFn = void (*)(const GradSmallItem<REAL>*, REAL, uint32_t, uint32_t, uint32_t, const uint32_t*);
    using GradSmallCountsFn = void (*)(const GradSmallItem<REAL>*, REAL, uint32_t, const GradSmallIO<REAL>*, const uint32_t*);
    static GradSmallUntrackedFn gs_untracked_fn(int nw, bool rl);
    static GradSmallCountsFn gs_counts_fn(int nw, bool rl);
    // The learned iterations with their history for a batch (kernels/smallhist.hpp; BatchT::learned_iterations_history): the kernels live in
    // solver_sh_f32.hip / _f64.hip.
    using SmallHistFn = void (*)(const SmallHistItem<REAL>*, REAL, uint32_t, uint32_t, uint32_t, uint32_t);
    static SmallHistFn sh_batch_fn(int nw, bool rl);
    // The learned iterations that stop on the bound's slope, for a batch (kernels/smallstop.hpp; BatchT::learned_iterations_stop): the kernels
    // live in solver_ss_f32.hip / _f64.hip.
    using SmallStopFn = void (*)(const SmallStopItem<REAL>*, REAL, uint32_t, uint32_t);
    static SmallStopFn ss_batch_fn(int nw, bool rl, bool hist);
    bool ov_ready = false;
    // One sweep: the wide and the narrow packs (one launch where `mixed`; forward only with mixed_fwd), then the huge ones.
    int launch_sweep(bool bwd, const Sweep& s, const REAL* delta_lay, REAL omega, int kclass, bool ov = false)
    {
        if (bwd) {  // the costs-to-terminal change: the cached bound is stale
            lb_cached = false;
            ++lb_gen;
        }
        DevPtrs<REAL> d = ptrs(delta_lay);
        if (ov) d.omega_lay = d_omega_lay;
        prof_begin(kclass);
        if (s.mixed.fn && (bwd || mixed_fwd)) {
            const PackDev pkw = pdev(wb_, nb_.n_packs), pkn = pdev(nb_, 0, stage_lds);
            const uint32_t nw8 = (wb_.n_packs + 7u) & ~7u;
            const dim3 grid(nw8 + narrow_grid(cdiv(nb_.n_packs, wpb))), block(64 * wpb);
            hipLaunchKernelGGL(s.mixed.fn, grid, block, s.mixed.lds, stream, d, pkn, pkw, omega, wide_pack_width);
        } else {
            if (s.wide.fn) hipLaunchKernelGGL(s.wide.fn, dim3(wb_.n_packs), dim3(wide_threads), s.wide.lds, stream, d, pdev(wb_, nb_.n_packs), omega, wide_pack_width);
            if (nb_.n_packs) {
                const PackDev pk = pdev(nb_, 0, s.seg_off);
                const dim3 grid(narrow_grid(cdiv(nb_.n_packs, s.w))), block(64 * s.w);
                if (s.res2)
                    hipLaunchKernelGGL(s.res2, grid, block, s.narrow_lds, stream, d_pack_hdr, d_quad_hdr, res2_ns, res2_nl, pk.n_packs, pk.xcd_chunk, d.stop, d.run_iter,
                                       d_res2_rec, d_res2_rec_off, res2_n_words, d, pk, omega);
                else if (s.res)
                    hipLaunchKernelGGL(s.res, grid, block, s.narrow_lds, stream, d_pack_hdr, d_quad_hdr, res_ns, res_nl, pk.n_packs, pk.xcd_chunk, d.stop, d.run_iter, d, pk, omega);
                else if (s.rec) hipLaunchKernelGGL(s.rec, grid, block, s.narrow_lds, stream, d, pk, s.rec_tab, s.rec_off, s.rec_words, omega);
                else hipLaunchKernelGGL(s.narrow, grid, block, s.narrow_lds, stream, d, pk, omega);
            }
        }
        if (s.huge) hipLaunchKernelGGL(s.huge, dim3(hb_.n_packs), dim3(WIDE_THREADS), 0, stream, d, pdev(hb_, nb_.n_packs + wb_.n_packs), omega, huge_pack_width, d_huge_scratch);
        prof_end(kclass);
        HIPCHK(hipGetLastError());
        return BDDMMA_OK;
    }
    int launch_fwd(int mode, const REAL* delta_lay, REAL omega, int kclass) { return launch_sweep(false, kern.sweep[0][mode], delta_lay, omega, kclass); }
    int launch_bwd(int mode, const REAL* delta_lay, REAL omega, int kclass) { return launch_sweep(true, kern.sweep[1][mode], delta_lay, omega, kclass); }
    // compute_delta + normalize_delta + broadcast to the layers, see kernels.hpp (k_exchange_reduce)
    void launch_bcast(const REAL* delta_var, REAL* delta_lay, RunGate g = RunGate{}, RunStep run = RunStep{})
    {
        hipLaunchKernelGGL((k_exchange_bcast<REAL>), dim3(cdiv(cdiv(n_layers, 4), 256)), dim3(256), 0, stream, delta_var, d_evar, delta_lay,
                           (uint32_t)n_layers, (uint32_t)n_vars, g, run);
    }
    // un-normalised per-variable sums of the deferred min-marginal differences (compute_delta only)
    void launch_reduce_raw(REAL* delta_var)
    {
        if (deterministic)
            hipLaunchKernelGGL((k_delta_gather<REAL, false>), dim3(cdiv(n_vars, 256)), dim3(256), 0, stream, d_mm_binned, d_var_ptr,
                               d_vpos, delta_var, (uint32_t)n_vars, RunGate{});
        else
            hipLaunchKernelGGL(kern.ex_raw.fn, dim3(n_bins), dim3(EX_THREADS), kern.ex_raw.lds, stream, d_mm_binned, d_bin_ptr, d_bvar,
                               (const uint32_t*)nullptr, 0u, vars_per_bin, (uint32_t)n_vars, (uint32_t)n_layers, d_nbdds, delta_var, (REAL*)nullptr, RunStep{},
                               (const REAL*)nullptr);
    }
    int exchange(bool ends_iteration = false)
    {
        const RunStep rstep = (ends_iteration && run_stop) ? run_step : RunStep{};
        prof_begin(BDDMMA_K_FINISH_DELTA);
        if (entry_by_var) {
            // entries of a variable are consecutive: one thread per variable reduces, normalises and broadcasts (deterministic order)
            hipLaunchKernelGGL((k_exchange_byvar<REAL>), dim3(cdiv(n_vars, 256)), dim3(256), 0, stream, d_mm_binned, d_var_ptr, d_delta_lay,
                               (uint32_t)n_vars, (uint32_t)n_layers, gate(), rstep);
            delta_var_valid = false;
        } else if (deterministic && !use_seg) {
            hipLaunchKernelGGL((k_delta_gather<REAL, true>), dim3(cdiv(n_vars, 256)), dim3(256), 0, stream, d_mm_binned, d_var_ptr,
                               d_vpos, d_delta_var, (uint32_t)n_vars, gate());
            launch_bcast(d_delta_var, d_delta_lay, gate(), rstep);
            delta_var_valid = true;
        } else {
            // RUN: the instantiation that looks at the stop word and, in the launch that ends an iteration, reduces the bound in one workgroup more
            const bool run = run_stop != nullptr;
            const dim3 grid(n_bins + (run && rstep.ctl != nullptr ? 1u : 0u)), block(kern.ex_threads);
            if (use_seg)
                hipLaunchKernelGGL(kern.seg[run].fn, grid, block, kern.seg[run].lds, stream, d_mm_binned, reinterpret_cast<const uint4*>(d_seg_bin), gate().stop,
                                   gate().iter, reinterpret_cast<const uint4*>(d_seg_perm), reinterpret_cast<const uint2*>(d_seg_thr), seg_tile_off, seg_cnt_off,
                                   d_delta_lay, rstep, (const REAL*)nullptr);
            else
                hipLaunchKernelGGL(kern.ex[run].fn, grid, block, kern.ex[run].lds, stream, d_mm_binned, d_bin_ptr, d_bvar, gate().stop, gate().iter, vars_per_bin,
                                   (uint32_t)n_vars, (uint32_t)n_layers, d_nbdds, (REAL*)nullptr, d_delta_lay, rstep, (const REAL*)nullptr);
            delta_var_valid = false;
        }
        prof_end(BDDMMA_K_FINISH_DELTA);
        HIPCHK(hipGetLastError());
        return BDDMMA_OK;
    }

    // ---------------------------------------------------------------------------- SolverBase
    int forward_run() override
    {
        if (fwd_valid) return BDDMMA_OK;
        HIPCHK(hipSetDevice(device));
        int rc = launch_fwd(FWD_PLAIN, nullptr, REAL(0), BDDMMA_K_OTHER);
        if (rc) return rc;
        fwd_valid = true;
        return BDDMMA_OK;
    }
    int backward_run() override
    {
        if (bwd_valid) return BDDMMA_OK;
        HIPCHK(hipSetDevice(device));
        int rc = launch_bwd(BWD_PLAIN, nullptr, REAL(0), BDDMMA_K_OTHER);
        if (rc) return rc;
        bwd_valid = lb_valid = true;
        return BDDMMA_OK;
    }
    // the bound's partial sums of the current costs: what the last backward sweep left (lb_valid), else a plain backward sweep
    int bound_run() { return lb_valid ? BDDMMA_OK : backward_run(); }
    int lower_bound(double* lb) override
    {
        int rc = bound_run();
        if (rc) return rc;
        if (lb_cached) {
            *lb = lb_cache;
            return BDDMMA_OK;
        }
        // no copy-engine round trip: one block writes the 8 bytes to pinned host memory, the host waits for the stream
        if ((rc = launch_bound(0))) return rc;
        if ((rc = wait_bound(0))) return rc;
        *lb = lb_cache = ((volatile double*)h_lb)[0];
        lb_cached = true;
        return BDDMMA_OK;
    }
    // The reduce kernel writes the bound and, behind it, a sequence number into pinned host memory; the host polls the number.  Waiting
    // for the stream instead goes through an interrupt: measured 26 us of idle GPU per bound read in the L-BFGS loop (tools/gaps.sh), which
    // reads 1.4 bounds per iteration.  After 2 ms without the number (a long queue ahead, or a fault) it falls back to the blocking wait.
    int launch_bound(int k)
    {
        lb_seq_expect[k] = ++lb_seq_next;
        hipLaunchKernelGGL(k_lb_reduce, dim3(1), dim3(1024), 0, stream, d_lb_partial, nb_.n_packs + wb_.n_packs + hb_.n_packs, d_lb + k, d_lb_seq + k, lb_seq_expect[k]);
        HIPCHK(hipGetLastError());
        return BDDMMA_OK;
    }
    int wait_bound(int k)
    {
        volatile uint64_t* w = h_lb_seq + k;
        const auto t0 = std::chrono::steady_clock::now();
        uint32_t spins = 0;
        while (*w != lb_seq_expect[k]) {
            cpu_relax();
            if ((++spins & 1023u) == 0 && std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > 2e-3) {
                HIPCHK(hipStreamSynchronize(stream));
                if (*w != lb_seq_expect[k]) { err = "lower bound: the reduce kernel did not report"; return BDDMMA_ERR_DEVICE; }
                break;
            }
        }
        std::atomic_thread_fence(std::memory_order_acquire);
        return BDDMMA_OK;
    }
    int lower_bound_enqueue(int slot) override
    {
        if (slot < 0 || slot > 1) { err = "lower_bound_enqueue: slot must be 0 or 1"; return BDDMMA_ERR_INVALID_ARGUMENT; }
        int rc = bound_run();
        if (rc) return rc;
        lb_slot_gen[slot] = lb_gen;
        if (lb_cached) {
            lb_slot_known[slot] = true;
            lb_slot_value[slot] = lb_cache;
            return BDDMMA_OK;
        }
        if ((rc = launch_bound(1 + slot))) return rc;
        lb_slot_known[slot] = false;
        lb_slot_enqueued[slot] = true;
        return BDDMMA_OK;
    }
    int lower_bound_fetch(int slot, double* lb) override
    {
        if (slot < 0 || slot > 1) { err = "lower_bound_fetch: slot must be 0 or 1"; return BDDMMA_ERR_INVALID_ARGUMENT; }
        if (!lb_slot_known[slot]) {
            if (!lb_slot_enqueued[slot]) { err = "lower_bound_fetch without lower_bound_enqueue"; return BDDMMA_ERR_STATE; }
            int rc = wait_bound(1 + slot);
            if (rc) return rc;
            lb_slot_value[slot] = ((volatile double*)h_lb)[1 + slot];
            lb_slot_known[slot] = true;
        }
        *lb = lb_slot_value[slot];
        if (lb_slot_gen[slot] == lb_gen && lb_valid) {  // no backward launch since: this is the bound of the current costs
            lb_cache = *lb;
            lb_cached = true;
        }
        return BDDMMA_OK;
    }
    int lower_bound_per_bdd(void* out, int on_device) override
    {
        int rc = backward_run();
        if (rc) return rc;
        REAL* tmp = nullptr;
        REAL* dst = (REAL*)out;
        if (!on_device) { HIPCHK(hipMalloc((void**)&tmp, n_bdds * sizeof(REAL))); dst = tmp; }
        hipLaunchKernelGGL((k_lb_per_bdd<REAL>), dim3(cdiv(n_bdds, 256)), dim3(256), 0, stream, d_T, d_root_slot, dst, (uint32_t)n_bdds);
        if (!on_device) {
            hipError_t e = hipMemcpyAsync(out, tmp, n_bdds * sizeof(REAL), hipMemcpyDeviceToHost, stream);
            if (e == hipSuccess) e = hipStreamSynchronize(stream);
            (void)hipFree(tmp);
            HIPCHK(e);
        }
        return BDDMMA_OK;
    }

    // ov: omega per layer from d_omega_lay (learned iterations with omega_vec; ov_sweep)
    // on_chip: the caller allows the sweeps that keep potentials on chip (kernels/narrow4.hpp) — iteration() alone; taken where the rule
    // of init() holds (onchip_hc) and no L-BFGS wrapper wants x in layer order from the backward sweeps
    bool onchip_usable(bool ov) const { return onchip_hc != 0 && !ov && d_x_layer == nullptr; }
    int mma_forward(REAL omega, const REAL* delta_lay, bool ov = false, bool on_chip = false)
    {
        int rc;
        const Sweep& s = ov ? ov_sweep[0] : (on_chip && onchip_usable(ov)) ? kern.onchip[0] : kern.sweep[0][FWD_SOLVE];
        if (s.reads_pot && !bwd_valid && (rc = backward_run())) return rc;  // bdd_cuda_parallel_mma.cu:211-212 (not for a sweep that rebuilds the costs-to-terminal)
        rc = launch_sweep(false, s, delta_lay, omega, BDDMMA_K_FORWARD_MM, ov);
        x_layer_valid = false;  // the forward sweep rewrites the deferred values by entry only
        if (rc) return rc;
        fwd_valid = s.stores_pot;
        bwd_valid = lb_valid = false;
        return BDDMMA_OK;
    }
    int mma_backward(REAL omega, const REAL* delta_lay, bool ov = false, bool on_chip = false)
    {
        const Sweep& s = ov ? ov_sweep[1] : (on_chip && onchip_usable(ov)) ? kern.onchip[1] : kern.sweep[1][BWD_SOLVE];
        if (s.reads_pot && !fwd_valid) {
            err = "backward_mm requires a valid forward state (call forward_mm first)";  // assert at :304
            return BDDMMA_ERR_STATE;
        }
        int rc = launch_sweep(true, s, delta_lay, omega, BDDMMA_K_BACKWARD_MM, ov);
        if (rc) return rc;
        x_layer_valid = d_x_layer != nullptr;
        fwd_valid = false;
        bwd_valid = s.stores_pot;
        lb_valid = true;
        return BDDMMA_OK;
    }
    // ---- instances that fit one workgroup: n iterations inside one launch (kernels/small.hpp).  Not while event pairs are wanted per launch
    // (profiling) or an L-BFGS wrapper wants x in layer order from the backward sweeps.
    bool small_usable() const { return small_ok && !profiling && d_x_layer == nullptr; }
    // the host-side state after a launch of whole iterations: what the last iteration's four launches leave (mma_forward, exchange,
    // mma_backward, exchange); the costs-to-terminal have changed, so the cached bound is stale
    void small_launched()
    {
        lb_cached = false;
        ++lb_gen;
        x_layer_valid = false;
        fwd_valid = false;
        bwd_valid = lb_valid = true;
        delta_var_valid = false;
    }
    int launch_small(REAL omega, uint32_t n, const RunStep& rstep)
    {
        int rc;
        if (!bwd_valid && (rc = backward_run())) return rc;  // bdd_cuda_parallel_mma.cu:211-212, as mma_forward
        const DevPtrs<REAL> d = ptrs(d_delta_lay);
        const PackDev pk = pdev(nb_, 0, 0);
        hipLaunchKernelGGL(kern.small.fn, dim3(1), dim3(64 * small_nw), kern.small.lds, stream, small, d, pk, omega, n, rstep);
        HIPCHK(hipGetLastError());
        small_launched();
        return BDDMMA_OK;
    }
    // n learned iterations in one launch (k_learned_small): the weights from d_alpha_ent, omega per layer from d_omega_lay (`ov`) or the scalar
    bool small_learned_usable() const { return small_ln_ok && small_usable(); }
    int launch_small_learned(REAL omega, bool ov, uint32_t n)
    {
        int rc;
        if (!sl_ready) {
            if ((rc = sl_prepare())) return rc;
            sl_ready = true;
        }
        if (!bwd_valid && (rc = backward_run())) return rc;  // as mma_forward
        SmallLearn<REAL> ln = small_ln_arg;
        ln.alpha_ent = d_alpha_ent;
        ln.omega_lay = ov ? d_omega_lay : nullptr;
        hipLaunchKernelGGL(small_ln_kern.fn, dim3(1), dim3(64 * small_nw), small_ln_kern.lds, stream, small_ln, ptrs(d_delta_lay), pdev(nb_, 0, 0), ln, omega, n);
        HIPCHK(hipGetLastError());
        small_launched();
        return BDDMMA_OK;
    }
    // (d_alpha_ent and d_omega_lay must exist: BatchT::learned_iterations allocates them first)
    SmallLearnItem<REAL> small_learn_item() const
    {
        SmallLearn<REAL> ln = small_ln_arg;
        ln.alpha_ent = d_alpha_ent;
        ln.omega_lay = d_omega_lay;
        return SmallLearnItem<REAL>{small_ln, ptrs(d_delta_lay), pdev(nb_, 0, 0), ln};
    }
    // the same launch as an item of a batch (solver_bt.hpp: one workgroup per member of BatchT); the run_solver fields are the batch's
    SmallItem<REAL> small_item() const { return SmallItem<REAL>{small, ptrs(d_delta_lay), pdev(nb_, 0, 0), RunStep{d_lb_partial, nb_.n_packs + wb_.n_packs + hb_.n_packs, nullptr, nullptr}}; }
    int iterations(double omega, uint64_t n) override
    {
        HIPCHK(hipSetDevice(device));
        if (!small_usable() || run_stop) {
            for (uint64_t i = 0; i < n; ++i)
                if (int rc = iteration(omega)) return rc;
            return BDDMMA_OK;
        }
        while (n) {
            const uint32_t chunk = (uint32_t)std::min<uint64_t>(n, 1u << 14);   // <= ~60 ms per launch: other processes' queues get the GPU in between
            if (int rc = launch_small((REAL)omega, chunk, RunStep{})) return rc;
            n -= chunk;
        }
        return BDDMMA_OK;
    }
    int iteration(double omega) override
    {
        HIPCHK(hipSetDevice(device));
        int rc;
        if (small_usable() && !run_stop) return launch_small((REAL)omega, 1, RunStep{});
        prof_active = profiling && (prof_iter++ % prof_stride == 0);
        if ((rc = mma_forward((REAL)omega, d_delta_lay, false, true))) return rc;
        if ((rc = exchange())) return rc;
        if ((rc = mma_backward((REAL)omega, d_delta_lay, false, true))) return rc;
        if ((rc = exchange(true))) return rc;
        return BDDMMA_OK;
    }
    // ---- learned iterations (bdd_cuda_learned_mma.cu:9-262, include/bdd_mma.h: bddmma_learned_iterations)
    // The weighted exchange of the deferred differences: {lo, hi} of entry e = alpha[e] * the variable's sums (no division by n[v]), into
    // d_delta_lay where the sweeps read it.  The same kernel family as exchange(), in its WEIGHTED instantiation, RUN = false.
    void weighted_exchange()
    {
        const REAL* al = d_alpha_ent;
        prof_begin(BDDMMA_K_FINISH_DELTA);
        if (entry_by_var) {
            hipLaunchKernelGGL((k_exchange_byvar<REAL, true>), dim3(cdiv(n_vars, 256)), dim3(256), 0, stream, d_mm_binned, d_var_ptr, d_delta_lay,
                               (uint32_t)n_vars, (uint32_t)n_layers, RunGate{}, RunStep{}, al);
        } else if (deterministic && !use_seg) {
            // raw sums into the explicit API's scratch (the solver's own per-variable delta is rebuilt by the exit exchange)
            hipLaunchKernelGGL((k_delta_gather<REAL, false>), dim3(cdiv(n_vars, 256)), dim3(256), 0, stream, d_mm_binned, d_var_ptr,
                               d_vpos, d_delta_c, (uint32_t)n_vars, RunGate{});
            hipLaunchKernelGGL((k_exchange_bcast<REAL, true>), dim3(cdiv(cdiv(n_layers, 4), 256)), dim3(256), 0, stream, (const REAL*)d_delta_c, d_evar,
                               d_delta_lay, (uint32_t)n_layers, (uint32_t)n_vars, RunGate{}, RunStep{}, al);
        } else if (use_seg) {
            hipLaunchKernelGGL(kern.seg_w.fn, dim3(n_bins), dim3(kern.ex_threads), kern.seg_w.lds, stream, d_mm_binned, reinterpret_cast<const uint4*>(d_seg_bin),
                               (const uint32_t*)nullptr, 0u, reinterpret_cast<const uint4*>(d_seg_perm), reinterpret_cast<const uint2*>(d_seg_thr), seg_tile_off,
                               seg_cnt_off, d_delta_lay, RunStep{}, al);
        } else {
            hipLaunchKernelGGL(kern.ex_w.fn, dim3(n_bins), dim3(kern.ex_threads), kern.ex_w.lds, stream, d_mm_binned, d_bin_ptr, d_bvar, (const uint32_t*)nullptr,
                               0u, vars_per_bin, (uint32_t)n_vars, (uint32_t)n_layers, d_nbdds, (REAL*)nullptr, d_delta_lay, RunStep{}, al);
        }
        delta_var_valid = false;
        prof_end(BDDMMA_K_FINISH_DELTA);
    }
    int isotropic_dist_weights(void* out, int on_device) override
    {
        HIPCHK(hipSetDevice(device));
        REAL* dst = on_device ? (REAL*)out : d_tmp0;
        hipLaunchKernelGGL((k_isotropic_alpha<REAL>), dim3(cdiv(n_layers, 256)), dim3(256), 0, stream, d_var, d_nbdds, dst, (uint32_t)n_layers);
        HIPCHK(hipGetLastError());
        if (!on_device) return copy_out(out, dst, n_layers * sizeof(REAL), 0);
        HIPCHK(hipStreamSynchronize(stream));
        return BDDMMA_OK;
    }
    // a REAL[n_layers] argument (dist_weights, omega_vec) -> dst on the device; BDDMMA_ERR_INVALID_ARGUMENT when a value is negative or not
    // finite (host input: before anything is copied)
    int load_layer_values(REAL* dst, const void* src, int on_dev, const char* what)
    {
        if (!on_dev) {
            const REAL* h = (const REAL*)src;
            for (uint64_t l = 0; l < n_layers; ++l)
                if (!(h[l] >= REAL(0) && h[l] < std::numeric_limits<REAL>::infinity())) {
                    err = std::string("learned_iterations: ") + what + "[" + std::to_string(l) + "] is negative or not finite";
                    return BDDMMA_ERR_INVALID_ARGUMENT;
                }
        }
        HIPCHK(hipMemcpyAsync(dst, src, n_layers * sizeof(REAL), on_dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, stream));
        if (on_dev) {
            HIPCHK(hipMemsetAsync(d_counts, 0, sizeof(uint32_t), stream));
            hipLaunchKernelGGL((k_count_bad_weights<REAL>), dim3(cdiv(n_layers, 256)), dim3(256), 0, stream, (const REAL*)dst, d_counts, (uint32_t)n_layers);
            uint32_t bad = 0;
            HIPCHK(hipMemcpyAsync(&bad, d_counts, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
            HIPCHK(hipStreamSynchronize(stream));
            if (bad) {
                err = "learned_iterations: " + std::to_string(bad) + " of the " + what + " are negative or not finite";
                return BDDMMA_ERR_INVALID_ARGUMENT;
            }
        }
        return BDDMMA_OK;
    }
    // omega_vec (bddmma_learned_iterations_omega_vec): null = the scalar omega; otherwise REAL[n_layers] in layer order, replacing it
    int learned_iterations(const void* w, int w_dev, uint64_t num_itr, double omega, double slope, void* sol_avg, void* lb1_avg, void* lb2_avg,
                           uint64_t cfi, double beta_d, int out_dev, uint64_t* itr_done, const void* omega_vec, int ov_dev) override
    {
        HIPCHK(hipSetDevice(device));
        int rc;
        if (itr_done) *itr_done = 0;
        if (!w) { err = "learned_iterations: dist_weights is null"; return BDDMMA_ERR_INVALID_ARGUMENT; }
        if (cfi > 0 && (!sol_avg || !lb1_avg || !lb2_avg)) {
            err = "learned_iterations: compute_history_for_itr > 0 needs sol_avg, lb_first_diff_avg and lb_second_diff_avg";
            return BDDMMA_ERR_INVALID_ARGUMENT;
        }
        if (*lbfgs_attached > 0) {
            err = "learned_iterations: an L-BFGS wrapper is attached to this solver (destroy it first: its history would not describe the costs any more)";
            return BDDMMA_ERR_STATE;
        }
        if (run_stop) { err = "learned_iterations: run_solver is queueing iterations"; return BDDMMA_ERR_STATE; }
        if (!d_alpha_ent && (rc = dalloc(&d_alpha_ent, n_layers))) return rc;
        // omega per layer: layer order is d_lohi's, so it goes to the sweeps as it is (checked before the weights touch anything)
        const bool ov = omega_vec != nullptr;
        if (ov) {
            if (!ov_ready) {
                if ((rc = ov_prepare())) return rc;
                ov_ready = true;
            }
            if (!d_omega_lay && (rc = dalloc(&d_omega_lay, n_layers))) return rc;
            if ((rc = load_layer_values(d_omega_lay, omega_vec, ov_dev, "omega_vec"))) return rc;
        }
        // the weights, layer order -> d_tmp0 (checked there) -> binned entry order
        if ((rc = load_layer_values(d_tmp0, w, w_dev, "dist_weights"))) return rc;
        hipLaunchKernelGGL((k_layers_to_entries<REAL>), dim3(cdiv(n_layers, 256)), dim3(256), 0, stream, (const REAL*)d_tmp0, d_lpos, d_alpha_ent, (uint32_t)n_layers);
        HIPCHK(hipGetLastError());
        // history buffers (:202-209): on the device; the caller's host outputs go through device copies, loaded first (an output the
        // history does not reach keeps what the caller had put there, as in the reference)
        const uint64_t B = n_bdds, L = n_layers;
        REAL *o_sol = (REAL*)sol_avg, *o_lb1 = (REAL*)lb1_avg, *o_lb2 = (REAL*)lb2_avg;
        REAL *last_sol = nullptr, *lb_last = nullptr, *lb_second = nullptr, *lb_third = nullptr, *chg = nullptr, *prev_chg = nullptr;
        if (cfi > 0) {
            if (!d_hist && (rc = dalloc(&d_hist, L + 5 * B))) return rc;
            last_sol = d_hist; lb_last = d_hist + L; lb_second = lb_last + B; lb_third = lb_second + B; chg = lb_third + B; prev_chg = chg + B;
            if (!out_dev) {
                if (!d_hist_out && (rc = dalloc(&d_hist_out, L + 2 * B))) return rc;
                o_sol = d_hist_out; o_lb1 = d_hist_out + L; o_lb2 = o_lb1 + B;
                HIPCHK(hipMemcpyAsync(o_sol, sol_avg, L * sizeof(REAL), hipMemcpyHostToDevice, stream));
                HIPCHK(hipMemcpyAsync(o_lb1, lb1_avg, B * sizeof(REAL), hipMemcpyHostToDevice, stream));
                HIPCHK(hipMemcpyAsync(o_lb2, lb2_avg, B * sizeof(REAL), hipMemcpyHostToDevice, stream));
            }
        }
        const REAL omega_r = (REAL)omega, beta = (REAL)beta_d;
        const dim3 gl(cdiv(L, 256)), gb(cdiv(B, 256)), blk(256);
        // the bound: read every iteration only where the stopping rule can fire (slope > 0); otherwise the set-once initial change is
        // taken from two enqueued bounds, fetched after the loop (no host synchronisation inside it)
        const bool track_lb = slope > 0;
        const bool want_initial = !std::isfinite(initial_lb_change);
        double lb_initial = 0.0, lb_prev = 0.0, lb_post = 0.0;
        if (num_itr > 0) {
            if (track_lb) {
                if ((rc = lower_bound(&lb_initial))) return rc;
            } else if (want_initial && (rc = lower_bound_enqueue(0))) return rc;
        }
        lb_post = lb_initial;
        bool converged = false;
        uint64_t tracked = 0, itr = 0, ran = 0;
        // One-workgroup instances without a stopping rule: the iterations the history does not reach run inside one launch each chunk
        // (k_learned_small; n then m learned iterations are n + m, and a launch leaves the state this loop starts from).  The first
        // iteration is a launch of its own where the initial change is still to be set: its bound is enqueued behind it.
        uint64_t fused_n = (!track_lb && small_learned_usable()) ? num_itr - std::min(num_itr, cfi) : 0;
        if (fused_n > 0) {
            uint64_t left = fused_n;
            if (want_initial) {
                if ((rc = launch_small_learned(omega_r, ov, 1)) || (rc = lower_bound_enqueue(1))) return rc;
                --left;
            }
            while (left) {
                const uint32_t chunk = (uint32_t)std::min<uint64_t>(left, 1u << 14);   // as iterations()
                if ((rc = launch_small_learned(omega_r, ov, chunk))) return rc;
                left -= chunk;
            }
            ran = fused_n;
        }
        const bool loop_runs = fused_n < num_itr;   // false: the last launch has made the exit exchange itself
        for (itr = fused_n; itr < num_itr; ++itr) {
            prof_active = profiling && (prof_iter++ % prof_stride == 0);
            weighted_exchange();  // forward_iteration_learned_mm_dist: compute_delta of the deferred differences (:68)
            if ((rc = mma_forward(omega_r, d_delta_lay, ov))) return rc;
            weighted_exchange();  // backward_iteration_learned_mm_dist (:143)
            if ((rc = mma_backward(omega_r, d_delta_lay, ov))) return rc;
            ++ran;
            if (cfi > 0 && (cfi >= num_itr - itr || converged)) {  // :211-254
                HIPCHK(hipMemsetAsync(d_sol, 0, n_layers, stream));
                if ((rc = launch_fwd(FWD_SOLUTION, nullptr, REAL(0), BDDMMA_K_OTHER))) return rc;
                hipLaunchKernelGGL((k_char_to_real<REAL>), gl, blk, 0, stream, (const char*)d_sol, last_sol, (uint32_t)L);
                hipLaunchKernelGGL((k_lb_per_bdd<REAL>), gb, blk, 0, stream, d_T, d_root_slot, lb_last, (uint32_t)B);
                if (tracked == 0) {
                    HIPCHK(hipMemcpyAsync(o_sol, last_sol, L * sizeof(REAL), hipMemcpyDeviceToDevice, stream));
                } else {
                    hipLaunchKernelGGL((k_ema<REAL>), gl, blk, 0, stream, o_sol, (const REAL*)last_sol, beta, (uint32_t)L);
                    hipLaunchKernelGGL((k_diff<REAL, REAL>), gb, blk, 0, stream, chg, (const REAL*)lb_last, (const REAL*)lb_second, (uint32_t)B);
                    if (tracked == 1) {
                        HIPCHK(hipMemcpyAsync(o_lb1, chg, B * sizeof(REAL), hipMemcpyDeviceToDevice, stream));
                    } else {
                        hipLaunchKernelGGL((k_ema<REAL>), gb, blk, 0, stream, o_lb1, (const REAL*)chg, beta, (uint32_t)B);
                        hipLaunchKernelGGL((k_diff<REAL, REAL>), gb, blk, 0, stream, prev_chg, (const REAL*)lb_second, (const REAL*)lb_third, (uint32_t)B);
                        hipLaunchKernelGGL((k_diff<REAL, REAL>), gb, blk, 0, stream, chg, (const REAL*)chg, (const REAL*)prev_chg, (uint32_t)B);
                        if (tracked == 2) HIPCHK(hipMemcpyAsync(o_lb2, chg, B * sizeof(REAL), hipMemcpyDeviceToDevice, stream));
                        else hipLaunchKernelGGL((k_ema<REAL>), gb, blk, 0, stream, o_lb2, (const REAL*)chg, beta, (uint32_t)B);
                    }
                }
                HIPCHK(hipGetLastError());
                // :251-252: second <- last, third <- second, last <- the old third (overwritten next time)
                REAL* t = lb_third;
                lb_third = lb_second;
                lb_second = lb_last;
                lb_last = t;
                ++tracked;
            }
            if (track_lb) {
                lb_prev = lb_post;
                if ((rc = lower_bound(&lb_post))) return rc;
                if (itr == 0 && want_initial) initial_lb_change = std::abs(lb_initial - lb_post);   // set_initial_lb_change: once per solver
                if (!converged && std::abs(lb_prev - lb_post) < slope * initial_lb_change) converged = true;
                if (converged && tracked == cfi) break;
            } else if (itr == 0 && want_initial && (rc = lower_bound_enqueue(1))) {
                return rc;
            }
        }
        // exit: the isotropic exchange of the last backward pass's differences — the state bddmma_iteration leaves
        if (ran > 0 && loop_runs && (rc = exchange())) return rc;
        if (ran > 0 && !track_lb && want_initial) {
            double a = 0.0, b = 0.0;
            if ((rc = lower_bound_fetch(0, &a)) || (rc = lower_bound_fetch(1, &b))) return rc;
            initial_lb_change = std::abs(a - b);
        }
        if (cfi > 0 && !out_dev) {
            HIPCHK(hipMemcpyAsync(sol_avg, o_sol, L * sizeof(REAL), hipMemcpyDeviceToHost, stream));
            HIPCHK(hipMemcpyAsync(lb1_avg, o_lb1, B * sizeof(REAL), hipMemcpyDeviceToHost, stream));
            HIPCHK(hipMemcpyAsync(lb2_avg, o_lb2, B * sizeof(REAL), hipMemcpyDeviceToHost, stream));
            HIPCHK(hipStreamSynchronize(stream));
        }
        if (itr_done) *itr_done = ran;
        return BDDMMA_OK;
    }
    // run_solver for the plain MMA iteration with the termination tests on the device (kernels.hpp: run_ctl_step).  The host
    // keeps up to `window` iterations queued and reads the published bounds; when the tests fire, the launches queued behind that
    // iteration return at once, so the state and the iteration count are the ones of the reference's sequential loop
    // (run_solver_util.h:40-73).  The wall-clock limit is tested on the host after every iteration it sees complete, as the reference
    // does; close to the limit the window shrinks to one iteration, so no iteration is queued that the sequential loop would not run.
    int run_plain(uint64_t max_iter, double tolerance, double slope, double time_limit, int verbose, bddmma_run_result* res) override
    {
        HIPCHK(hipSetDevice(device));
        const auto t0 = std::chrono::steady_clock::now();
        auto elapsed = [&]() { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); };
        if (!d_run_ctl) {
            HIPCHK(hipMalloc((void**)&d_run_ctl, sizeof(RunCtl)));
            HIPCHK(hipHostMalloc((void**)&h_run, sizeof(RunHost), hipHostMallocMapped | hipHostMallocCoherent));
            HIPCHK(hipHostGetDevicePointer((void**)&d_run_host, h_run, 0));
        }
        double lb_initial;
        int rc = lower_bound(&lb_initial);
        if (rc) return rc;
        if (verbose) std::printf("[bdd solver] initial lower bound = %.10g, time = %.3f s\n", lb_initial, elapsed());
        RunCtl c{};
        c.stop = RUN_NOT_STOPPED;
        c.lb_initial = lb_initial;
        c.lb_first = std::numeric_limits<double>::max();
        c.lb_post = lb_initial;
        c.tolerance = tolerance;
        c.slope = slope;
        c.time_limit = time_limit;
        std::memset((void*)h_run, 0, sizeof(RunHost));
        run_step = RunStep{d_lb_partial, nb_.n_packs + wb_.n_packs + hb_.n_packs, d_run_ctl, d_run_host};
        HIPCHK(hipMemcpyAsync(d_run_ctl, &c, sizeof(RunCtl), hipMemcpyHostToDevice, stream));
        hipLaunchKernelGGL(k_run_begin, dim3(1), dim3(1), 0, stream, d_run_ctl, (uint64_t)(elapsed() * RUN_TICKS_PER_SECOND));
        HIPCHK(hipStreamSynchronize(stream));  // c is a stack object
        constexpr uint64_t WINDOW = 6;  // iterations queued ahead of the last bound seen (< RUN_RING)
        volatile RunHost* hr = h_run;
        uint64_t queued = 0, seen = 0;
        uint32_t idle_spins = 0;
        double idle_since = 0.0;
        int reason = 0;
        double lb_post = lb_initial;
        run_stop = &d_run_ctl->stop;
        while (true) {
            // (the wall-clock limit is tested on the device with the other criteria, run_ctl_step: iterations queued behind the one that
            // crossed it return at once like those behind any other stop)
            // instances that fit one workgroup: SMALL_CHUNK iterations per launch, the tests inside the kernel after each (k_iterate_small); at most
            // two chunks are outstanding, fewer bounds than the ring of published ones holds
            constexpr uint64_t SMALL_CHUNK = 64;
            static_assert(2 * SMALL_CHUNK < RUN_RING, "published bounds must not wrap before the host has read them");
            const bool fused = small_usable();
            const uint64_t window = fused ? SMALL_CHUNK + 1 : WINDOW;
            bool launched = false;
            while (queued < max_iter && queued - seen < window) {
                run_iter = (uint32_t)std::min<uint64_t>(queued, RUN_NOT_STOPPED - 1);
                const uint64_t n_launch = fused ? std::min<uint64_t>(SMALL_CHUNK, max_iter - queued) : 1;
                // the sequential path's last launch also reduces the bound and runs the tests (exchange(true))
                rc = fused ? launch_small(REAL(0.5), (uint32_t)n_launch, run_step) : iteration(0.5);
                if (rc) {  // launches of this and earlier iterations may be in flight: drain them before the gate goes away
                    (void)hipStreamSynchronize(stream);
                    run_stop = nullptr;
                    return rc;
                }
                queued += n_launch;
                launched = true;
            }
            if (queued == 0) break;  // max_iter == 0
            const uint64_t st = hr->state;
            const uint64_t done = st & ((1ull << 56) - 1);
            const int dev_reason = (int)(st >> 56);
            bool stop = false;
            const bool progressed = done > seen;
            for (; seen < done && !stop; ++seen) {
                lb_post = hr->lb[seen % RUN_RING];
                if (verbose) std::printf("[bdd solver] iteration %llu, lower bound = %.10g, time = %.3f s\n", (unsigned long long)seen, lb_post, elapsed());
            }
            if (stop) break;
            if (dev_reason && seen == done) { reason = dev_reason; break; }
            if (seen == max_iter) break;
            if (!launched && !progressed) {
                // nothing new (no launch in this pass, no bound published since the last one): spin for the first millisecond (an iteration is 20-250 us), then poll every 50 us without holding a core.
                // After 0.2 s without a published bound make sure the device is still alive: a blocking wait for the stream (harmless
                // if an iteration is simply that long) — still nothing then means the queued launches were lost, which the checks
                // behind the loop report.  (hipStreamQuery is not used for this: it was seen to report an idle stream with launches
                // still queued, which ended runs early.)  A pass that SAW progress is not idle, whatever the clock says: through round 5 the
                // test was "no launch in this pass", so a pass that found the window full at its start and all of it done at its read —
                // with a 0.2 s old idle stamp, which takes a GPU shared by a dozen processes — synchronised an empty stream, found "nothing
                // new" and ended the run early with reason 0 (soak of round 6: 1 of 32 loops; tests/tools/stress_run_solver.py: 15 of 3 200).
                const double now = elapsed();
                if (idle_spins++ == 0) idle_since = now;
                if (now - idle_since > 0.2) {
                    const hipError_t e = hipStreamSynchronize(stream);
                    if (e != hipSuccess) {
                        run_stop = nullptr;
                        err = std::string("run_solver: ") + hipGetErrorString(e);
                        return BDDMMA_ERR_DEVICE;
                    }
                    if ((hr->state & ((1ull << 56) - 1)) == seen && seen < queued) break;   // launches are outstanding and the idle stream has not run them
                    idle_spins = 0;
                } else if (now - idle_since > 1e-3) {
                    std::this_thread::sleep_for(std::chrono::microseconds(50));
                } else {
                    cpu_relax();
                }
            } else {
                idle_spins = 0;
            }
        }
        run_stop = nullptr;
        HIPCHK(hipStreamSynchronize(stream));
        // iterations that were still in flight when the time limit was seen have run too (at most `window` - 1; they are counted)
        {
            const uint64_t st = hr->state;
            const uint64_t done = st & ((1ull << 56) - 1);
            for (; seen < done; ++seen) lb_post = hr->lb[seen % RUN_RING];
        }
        if (reason == 0 && seen < queued) {
            err = "run_solver: queued iterations did not complete";
            return BDDMMA_ERR_DEVICE;
        }
        if (seen > 0) {  // the device's bound of the last iteration that ran is lower_bound() of the state it left (same sum, same order)
            lb_cache = lb_post;
            lb_cached = true;
        }
        if (verbose) std::printf("[bdd solver] final lower bound = %.10g\n", lb_post);
        if (res) {
            res->iterations = seen;
            res->lb_initial = lb_initial;
            res->lb_final = lb_post;
            res->seconds = elapsed();
            res->stop_reason = reason;
        }
        return BDDMMA_OK;
    }
    int explicit_mm(bool forward, double omega, void* delta, int on_device)
    {
        HIPCHK(hipSetDevice(device));
        const size_t bytes = 2 * n_vars * sizeof(REAL);
        HIPCHK(hipMemcpyAsync(d_delta_c, delta, bytes, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, stream));
        launch_bcast(d_delta_c, d_delta_lay_c);  // the caller's delta, as given, to every layer
        int rc = forward ? mma_forward((REAL)omega, d_delta_lay_c) : mma_backward((REAL)omega, d_delta_lay_c);
        if (rc) return rc;
        launch_reduce_raw(d_delta_c);
        HIPCHK(hipMemcpyAsync(delta, d_delta_c, bytes, on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, stream));
        HIPCHK(hipStreamSynchronize(stream));
        return BDDMMA_OK;
    }
    int forward_mm(double omega, void* delta, int on_device) override { return explicit_mm(true, omega, delta, on_device); }
    int backward_mm(double omega, void* delta, int on_device) override { return explicit_mm(false, omega, delta, on_device); }

    int normalize_delta(void* delta, int on_device) override
    {
        HIPCHK(hipSetDevice(device));
        const size_t bytes = 2 * n_vars * sizeof(REAL);
        REAL* p = (REAL*)delta;
        if (!on_device) { p = d_delta_c; HIPCHK(hipMemcpyAsync(p, delta, bytes, hipMemcpyHostToDevice, stream)); }
        hipLaunchKernelGGL((k_normalize_delta<REAL>), dim3(cdiv(2 * n_vars, 256)), dim3(256), 0, stream, p, d_nbdds, (uint32_t)(2 * n_vars));
        if (!on_device) HIPCHK(hipMemcpyAsync(delta, p, bytes, hipMemcpyDeviceToHost, stream));
        HIPCHK(hipStreamSynchronize(stream));
        return BDDMMA_OK;
    }
    int distribute_delta() override
    {
        HIPCHK(hipSetDevice(device));
        // what this call applies and clears is what bddmma_grad_distribute_delta reads afterwards: keep a copy
        int rc;
        if (!d_mm_consumed && (rc = dalloc(&d_mm_consumed, n_layers))) return rc;
        HIPCHK(hipMemcpyAsync(d_mm_consumed, d_mm_binned, n_layers * sizeof(REAL), hipMemcpyDeviceToDevice, stream));
        mm_consumed_valid = true;
        hipLaunchKernelGGL((k_distribute_delta<REAL>), dim3(cdiv(n_layers, 256)), dim3(256), 0, stream, d_lo, d_hi, d_mm_binned, d_lpos, (uint32_t)n_layers);
        x_layer_valid = false;
        HIPCHK(hipMemsetAsync(d_delta_var, 0, 2 * n_vars * sizeof(REAL), stream));  // bdd_cuda_base.cu:1428
        HIPCHK(hipMemsetAsync(d_delta_lay, 0, 2 * n_layers * sizeof(REAL), stream));
        delta_var_valid = true;
        costs_changed();
        HIPCHK(hipGetLastError());
        return BDDMMA_OK;
    }
    int get_delta(void* out, int on_device) override
    {
        HIPCHK(hipSetDevice(device));
        if (!delta_var_valid) {
            hipLaunchKernelGGL((k_delta_var_from_lay<REAL>), dim3(cdiv(n_vars, 256)), dim3(256), 0, stream, d_delta_lay, d_var_ptr, d_vpos,
                               d_delta_var, (uint32_t)n_vars);
            delta_var_valid = true;
        }
        HIPCHK(hipMemcpyAsync(out, d_delta_var, 2 * n_vars * sizeof(REAL), on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, stream));
        HIPCHK(hipStreamSynchronize(stream));
        return BDDMMA_OK;
    }

    int set_delta(const void* in, int on_device) override
    {
        HIPCHK(hipSetDevice(device));
        HIPCHK(hipMemcpyAsync(d_delta_var, in, 2 * n_vars * sizeof(REAL), on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, stream));
        launch_bcast(d_delta_var, d_delta_lay);
        delta_var_valid = true;
        HIPCHK(hipStreamSynchronize(stream));
        return BDDMMA_OK;
    }

    template <typename TIN>
    int update_both(const void* lo, uint64_t n_lo, const void* hi, uint64_t n_hi, int on_device)
    {
        if (n_lo == 0 && n_hi == 0) return BDDMMA_OK;
        if (n_lo > n_vars || n_hi > n_vars) { err = "cost vector longer than nr_variables()"; return BDDMMA_ERR_INVALID_ARGUMENT; }
        const TIN *dlo = (const TIN*)lo, *dhi = (const TIN*)hi;
        TIN* tmp = nullptr;
        if (!on_device) {  // one staging buffer for both sides
            HIPCHK(hipMalloc((void**)&tmp, (n_lo + n_hi) * sizeof(TIN)));
            hipError_t e = hipSuccess;
            if (n_lo) e = hipMemcpyAsync(tmp, lo, n_lo * sizeof(TIN), hipMemcpyHostToDevice, stream);
            if (n_hi && e == hipSuccess) e = hipMemcpyAsync(tmp + n_lo, hi, n_hi * sizeof(TIN), hipMemcpyHostToDevice, stream);
            if (e != hipSuccess) { (void)hipFree(tmp); HIPCHK(e); }
            dlo = tmp;
            dhi = tmp + n_lo;
        }
        if (!d_cost_q) {
            int rc;
            if ((rc = dalloc(&d_cost_q, n_vars)) || (rc = dalloc(&d_cost_flags, n_vars))) { if (tmp) (void)hipFree(tmp); return rc; }
        }
        hipLaunchKernelGGL((k_cost_quotients<TIN>), dim3(cdiv(n_vars, 256)), dim3(256), 0, stream, d_cost_q, d_cost_flags, d_nbdds, dlo, n_lo, dhi, n_hi,
                           (uint32_t)n_vars);
        hipLaunchKernelGGL((k_update_costs<REAL>), dim3(cdiv(n_layers, 256)), dim3(256), 0, stream, d_lohi, d_var, (const CostQuot*)d_cost_q,
                           (const uint8_t*)d_cost_flags, (uint32_t)(n_lo != 0), (uint32_t)(n_hi != 0), (uint32_t)n_layers);
        if (tmp) { HIPCHK(hipStreamSynchronize(stream)); (void)hipFree(tmp); }
        return BDDMMA_OK;
    }
    int update_costs(const void* lo, uint64_t n_lo, const void* hi, uint64_t n_hi, int elem_precision, int on_device) override
    {
        HIPCHK(hipSetDevice(device));
        int rc = elem_precision == BDDMMA_F64 ? update_both<double>(lo, n_lo, hi, n_hi, on_device) : update_both<float>(lo, n_lo, hi, n_hi, on_device);
        if (rc) return rc;
        costs_changed();
        HIPCHK(hipGetLastError());
        return BDDMMA_OK;
    }
    int set_cost(double c, uint64_t var) override
    {
        if (var >= n_vars) { err = "variable out of range"; return BDDMMA_ERR_INVALID_ARGUMENT; }
        HIPCHK(hipSetDevice(device));
        const uint32_t k0 = h_var_ptr[var], k1 = h_var_ptr[var + 1];
        if (k1 > k0) {
            const REAL cc = REAL(c / (double)(k1 - k0));
            hipLaunchKernelGGL((k_set_cost<REAL>), dim3(cdiv(k1 - k0, 64)), dim3(64), 0, stream, d_hi, d_var_layers, k0, k1, cc);
        }
        costs_changed();
        HIPCHK(hipGetLastError());
        return BDDMMA_OK;
    }
    int copy_out(void* dst, const void* src, size_t bytes, int on_device) const
    {
        std::string& err = const_cast<std::string&>(this->err);
        if (!dst) return BDDMMA_OK;
        HIPCHK(hipMemcpyAsync(dst, src, bytes, on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, stream));
        HIPCHK(hipStreamSynchronize(stream));
        return BDDMMA_OK;
    }
    int get_solver_costs(void* lo, void* hi, void* mm, int on_device) override
    {
        int rc;
        std::string& err = const_cast<std::string&>(this->err);
        HIPCHK(hipSetDevice(device));
        const dim3 g(cdiv(n_layers, 256)), b(256);
        if (lo) {
            hipLaunchKernelGGL((k_strided_copy<REAL>), g, b, 0, stream, d_tmp0, 1u, (const REAL*)d_lo, 2u, (uint32_t)n_layers);
            if ((rc = copy_out(lo, d_tmp0, n_layers * sizeof(REAL), on_device))) return rc;
        }
        if (hi) {
            hipLaunchKernelGGL((k_strided_copy<REAL>), g, b, 0, stream, d_tmp0, 1u, (const REAL*)d_hi, 2u, (uint32_t)n_layers);
            if ((rc = copy_out(hi, d_tmp0, n_layers * sizeof(REAL), on_device))) return rc;
        }
        if (!mm) return BDDMMA_OK;
        hipLaunchKernelGGL((k_entries_to_layers<REAL>), dim3(cdiv(n_layers, 256)), dim3(256), 0, stream, d_mm_binned, d_lpos, d_tmp0, (uint32_t)n_layers);
        return copy_out(mm, d_tmp0, n_layers * sizeof(REAL), on_device);
    }
    int set_solver_costs(const void* lo, const void* hi, const void* mm, int on_device) override
    {
        const hipMemcpyKind k = on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
        HIPCHK(hipSetDevice(device));
        const dim3 g(cdiv(n_layers, 256)), b(256);
        if (lo) {
            HIPCHK(hipMemcpyAsync(d_tmp0, lo, n_layers * sizeof(REAL), k, stream));
            hipLaunchKernelGGL((k_strided_copy<REAL>), g, b, 0, stream, d_lo, 2u, (const REAL*)d_tmp0, 1u, (uint32_t)n_layers);
        }
        if (hi) {
            HIPCHK(hipMemcpyAsync(d_tmp0, hi, n_layers * sizeof(REAL), k, stream));
            hipLaunchKernelGGL((k_strided_copy<REAL>), g, b, 0, stream, d_hi, 2u, (const REAL*)d_tmp0, 1u, (uint32_t)n_layers);
        }
        if (mm) {
            x_layer_valid = false;
            HIPCHK(hipMemcpyAsync(d_tmp0, mm, n_layers * sizeof(REAL), k, stream));
            hipLaunchKernelGGL((k_layers_to_entries<REAL>), dim3(cdiv(n_layers, 256)), dim3(256), 0, stream, d_tmp0, d_lpos, d_mm_binned, (uint32_t)n_layers);
        }
        HIPCHK(hipStreamSynchronize(stream));
        costs_changed();
        return BDDMMA_OK;
    }
    int primal_objective_vec(void* out, int on_device) override
    {
        HIPCHK(hipSetDevice(device));
        REAL* dst = on_device ? (REAL*)out : d_delta_c;  // 2V scratch is large enough
        hipLaunchKernelGGL((k_primal_objective<REAL>), dim3(cdiv(n_vars, 256)), dim3(256), 0, stream, d_lo, d_hi, d_var_ptr, d_var_layers, dst, (uint32_t)n_vars);
        if (!on_device) return copy_out(out, dst, n_vars * sizeof(REAL), 0);
        HIPCHK(hipStreamSynchronize(stream));
        return BDDMMA_OK;
    }
    int min_marginals(int sorted, int32_t* var, void* mm0, void* mm1, int on_device) override
    {
        HIPCHK(hipSetDevice(device));
        int rc;
        if ((rc = forward_run())) return rc;  // bdd_cuda_base.cu:720
        if ((rc = launch_bwd(BWD_MARGINALS, nullptr, REAL(0), BDDMMA_K_OTHER))) return rc;
        bwd_valid = lb_valid = true;
        return marginals_out(sorted, var, mm0, mm1, on_device);
    }
    // the per-layer pair a marginal sweep left in d_tmp0 / d_tmp1 (min-marginals, sum-marginals) -> the caller, in layer order or gathered
    // by primal_variable_sorting_order_
    int marginals_out(int sorted, int32_t* var, void* mm0, void* mm1, int on_device)
    {
        const hipMemcpyKind k = on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
        if (!sorted) {
            if (var) HIPCHK(hipMemcpyAsync(var, d_var, n_layers * sizeof(int32_t), k, stream));
            if (mm0) HIPCHK(hipMemcpyAsync(mm0, d_tmp0, n_layers * sizeof(REAL), k, stream));
            if (mm1) HIPCHK(hipMemcpyAsync(mm1, d_tmp1, n_layers * sizeof(REAL), k, stream));
            HIPCHK(hipStreamSynchronize(stream));
            return BDDMMA_OK;
        }
        // gather by primal_variable_sorting_order_ (:737-746)
        REAL *s0 = nullptr, *s1 = nullptr;
        int32_t* sv = nullptr;
        HIPCHK(hipMalloc((void**)&s0, std::max<uint64_t>(n_layers, 1) * sizeof(REAL)));
        HIPCHK(hipMalloc((void**)&s1, std::max<uint64_t>(n_layers, 1) * sizeof(REAL)));
        HIPCHK(hipMalloc((void**)&sv, std::max<uint64_t>(n_layers, 1) * sizeof(int32_t)));
        const dim3 g(cdiv(n_layers, 256)), b(256);
        hipLaunchKernelGGL((k_gather<REAL>), g, b, 0, stream, d_tmp0, d_var_layers, s0, (uint32_t)n_layers);
        hipLaunchKernelGGL((k_gather<REAL>), g, b, 0, stream, d_tmp1, d_var_layers, s1, (uint32_t)n_layers);
        hipLaunchKernelGGL(k_gather_var, g, b, 0, stream, d_var, d_var_layers, sv, (uint32_t)n_layers);
        hipError_t e = hipSuccess;
        if (var && e == hipSuccess) e = hipMemcpyAsync(var, sv, n_layers * sizeof(int32_t), k, stream);
        if (mm0 && e == hipSuccess) e = hipMemcpyAsync(mm0, s0, n_layers * sizeof(REAL), k, stream);
        if (mm1 && e == hipSuccess) e = hipMemcpyAsync(mm1, s1, n_layers * sizeof(REAL), k, stream);
        if (e == hipSuccess) e = hipStreamSynchronize(stream);
        (void)hipFree(s0); (void)hipFree(s1); (void)hipFree(sv);
        HIPCHK(e);
        return BDDMMA_OK;
    }
    // ---------------------------------------------------------------------------- the pull sweeps (kernels/pull.hpp)
    // One launch per pack family, each a profiled group of its own (class BDDMMA_K_OTHER), so that the launch counts of bddmma_get_profile
    // count these kernels.  The parent tables are the solver's (sm_prepare), the same for every sweep; `tail` = the sweep's own arguments.
    template <typename... TAIL, typename... ARGS>
    int launch_pull(const PullSweep<REAL, TAIL...>& s, ARGS... tail)
    {
        const DevPtrs<REAL> d = ptrs(nullptr);
        auto family = [&](auto fn, const PackBufs& b, uint32_t lb_base, uint32_t threads, uint32_t ww, const uint32_t* ptr, const uint32_t* par, unsigned char* scratch) {
            if (!b.n_packs) return;
            prof_begin(BDDMMA_K_OTHER);
            hipLaunchKernelGGL(fn, dim3(b.n_packs), dim3(threads), scratch ? 0 : s.bytes(sizeof(REAL), ww), stream, d, pdev(b, lb_base), ptr, par, ww, scratch, tail...);
            prof_end(BDDMMA_K_OTHER);
        };
        family(s.narrow, nb_, 0, 64, pack_width, d_sm_nptr, d_sm_npar, nullptr);
        family(s.wide, wb_, nb_.n_packs, WIDE_THREADS, wide_pack_width, d_sm_wptr, d_sm_wpar, nullptr);
        family(s.huge, hb_, nb_.n_packs + wb_.n_packs, WIDE_THREADS, huge_pack_width, d_sm_wptr, d_sm_wpar, s.scratch);
        HIPCHK(hipGetLastError());
        return BDDMMA_OK;
    }
    // The wide launches of an operator's two sweeps (they share their bytes per pack): an error where a wide pack does not fit the LDS, the
    // launch attribute where its dynamic LDS is beyond the default limit.  Not through raise_lds_limit(): that sets the attribute for every
    // size but zero, and these kernels have always been launched without it up to 48 KiB.
    template <typename... A, typename... B>
    int pull_wide_lds(const char* what, const PullSweep<REAL, A...>& a, const PullSweep<REAL, B...>& b)
    {
        const uint32_t wl = (uint32_t)a.bytes(sizeof(REAL), wide_pack_width);
        if (wb_.n_packs && wl > lds_cu) { err = std::string(what) + ": a wide pack does not fit the LDS"; return BDDMMA_ERR_UNSUPPORTED; }
        if (wb_.n_packs && wl > 48 * 1024) {
            HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(a.wide), hipFuncAttributeMaxDynamicSharedMemorySize, (int)wl));
            HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(b.wide), hipFuncAttributeMaxDynamicSharedMemorySize, (int)wl));
        }
        return BDDMMA_OK;
    }
    // Sum-marginals (kernels/summarg.hpp).  Defined in solver_sm.hpp and instantiated in translation units of their own (solver_sm_f32.hip /
    // solver_sm_f64.hip), as the OV sweeps are: only declared here.
    PullSweep<REAL> sm_fwd_sweep() const, sm_bwd_sweep() const;
    int sm_prepare();       // first call: the parent tables of the forward pull, derived from the node words
    int sm_launch_fwd();    // launch_pull of the sweep, and what it does to the solver's state
    int sm_launch_bwd();
    int sm_sum_marginals(int sorted, int log_probs, int32_t* var, void* sm0, void* sm1, int on_device);
    int sm_smooth_solution(void* out, int on_device);
    bool sm_ready = false;
    uint32_t *d_sm_nptr = nullptr, *d_sm_npar = nullptr, *d_sm_wptr = nullptr, *d_sm_wpar = nullptr;  // parent tables: narrow words / wide words
    unsigned char* d_sm_scratch = nullptr;  // huge packs: the sum sweeps' per-pack arrays (sm_lds_bytes of the huge width each)
    int sum_marginals(int sorted, int log_probs, int32_t* var, void* sm0, void* sm1, int on_device) override
    {
        return sm_sum_marginals(sorted, log_probs, var, sm0, sm1, on_device);
    }
    int smooth_solution(void* out, int on_device) override { return sm_smooth_solution(out, on_device); }
    // Gradients (kernels/gradmm.hpp and three elementwise kernels).  Defined in solver_gr.hpp and instantiated in translation units of their
    // own (solver_gr_f32.hip / solver_gr_f64.hip), as the sum-marginals are: only declared here.
    PullSweep<REAL, const REAL*, REAL*, REAL*, uint32_t*> gr_down_sweep() const;
    PullSweep<REAL, const REAL*, REAL*, REAL*, const uint32_t*> gr_up_sweep() const;
    int gr_prepare();       // first call: the parent tables (sm_prepare) and this operator's per-layer scratch
    int gr_inputs(bool second);  // d_gr_in0 and, for the operators that take two gradients, d_gr_in1: allocated on first use
    int gr_launch_down();   // root -> terminal: seeds, the gradient through T
    int gr_launch_up();     // terminal -> root: the gradient through F
    int gr_load(REAL* dst, const void* src, uint64_t n, int on_dev, const char* what);  // an incoming gradient -> the device, checked finite
    // The same for up to LOAD_MAX_ARRAYS device arrays of n values at once (k_load_checked: one launch, one read of the counts, one
    // synchronisation): checked in the order given, the first offending one reported in the words gr_load / load_layer_values use.
    // weights: the array must also be >= 0 and is reported as load_layer_values does, `what` prefixed by `me`.
    struct LoadSpec { REAL* dst; const void* src; const char* what; bool weights; };
    int gr_load_device(const LoadSpec* specs, int count, uint64_t n, const char* me);
    int gr_min_marginal_diff(const void* grad_mm, void* grad_lo, void* grad_hi, int on_device);
    int gr_lower_bound_per_bdd(const void* grad_lb, void* grad_lo, void* grad_hi, int smooth, int on_device);
    int gr_distribute_delta(const void* grad_lo, const void* grad_hi, void* grad_deferred_mm, int on_device);
    int gr_cost_perturbation(const void* grad_lo, const void* grad_hi, void* grad_lo_pert, void* grad_hi_pert, int on_device);
    bool gr_ready = false;
    REAL *d_gr_in0 = nullptr, *d_gr_in1 = nullptr;   // incoming gradients in layer order (L each; the per-BDD one fits as well: B <= L)
    uint32_t* d_gr_arg = nullptr;                    // 2L: hop-local slot of the arg-min node of every layer's lo / hi arc (GR_NONE: no finite path)
    unsigned char* d_gr_scratch = nullptr;           // huge packs: the gradient sweeps' per-pack arrays (gr_lds_bytes of the huge width each)
    REAL* d_mm_consumed = nullptr;                   // L, binned entry order: the deferred differences the last distribute_delta() applied
    bool mm_consumed_valid = false;
    int grad_min_marginal_diff(const void* g, void* lo, void* hi, int on_device) override { return gr_min_marginal_diff(g, lo, hi, on_device); }
    int grad_lower_bound_per_bdd(const void* g, void* lo, void* hi, int smooth, int on_device) override { return gr_lower_bound_per_bdd(g, lo, hi, smooth, on_device); }
    int grad_distribute_delta(const void* lo, const void* hi, void* out, int on_device) override { return gr_distribute_delta(lo, hi, out, on_device); }
    int grad_cost_perturbation(const void* lo, const void* hi, void* lo_p, void* hi_p, int on_device) override { return gr_cost_perturbation(lo, hi, lo_p, hi_p, on_device); }
    // The backward of the learned iterations (kernels/graditer.hpp).  Defined in solver_gi.hpp and instantiated in translation units of its
    // own (solver_gi_f32.hip / solver_gi_f64.hip), as the single-shot operators are: only declared here.
    int gi_prepare(uint64_t n_caches);  // every buffer of a call with that many caches, before the solver is touched
    int gi_grad_learned_iterations(const void* w, int w_dev, double omega, const void* omega_vec, int ov_dev, void* grad_lo, void* grad_hi, void* grad_mm,
                                   void* grad_w_out, void* grad_omega_out, uint64_t after, uint64_t n, uint64_t num_caches, int on_device);
    int gi_time_kernel(int kind, uint64_t reps, double* ms);  // bddmma_time_kernel kinds 13 - 17
    struct { int kind = 0; uint64_t reps = 0; float ms = 0.f; } gi_timing;  // kind != 0: that launch group of the call is repeated and timed
    bool gi_ready = false;
    REAL* d_gi = nullptr;                  // the call's per-layer / per-slot / per-variable arrays, one block (solver_gi.hpp)
    std::vector<REAL*> gi_caches;          // {lo, hi} per layer + deferred differences in binned entry order, 3 L each
    unsigned char* d_gi_scratch = nullptr; // huge packs: the reverse sweeps' per-pack arrays (gi_lds_bytes of the huge width each)
    int grad_learned_iterations(const void* w, int w_dev, double omega, const void* omega_vec, int ov_dev, void* grad_lo, void* grad_hi, void* grad_mm,
                                void* grad_w_out, void* grad_omega_out, uint64_t after, uint64_t n, uint64_t num_caches, int on_device) override
    {
        return gi_grad_learned_iterations(w, w_dev, omega, omega_vec, ov_dev, grad_lo, grad_hi, grad_mm, grad_w_out, grad_omega_out, after, n, num_caches, on_device);
    }
    int min_marginal_diff(void* out, int on_device) override
    {
        HIPCHK(hipSetDevice(device));
        int rc;
        if ((rc = forward_run())) return rc;
        if ((rc = launch_bwd(BWD_MARGINALS, nullptr, REAL(0), BDDMMA_K_OTHER))) return rc;
        bwd_valid = lb_valid = true;
        REAL* dst = on_device ? (REAL*)out : d_tmp0;  // in place over mm0 when the result goes to the host
        hipLaunchKernelGGL((k_diff<REAL, REAL>), dim3(cdiv(n_layers, 256)), dim3(256), 0, stream, dst, (const REAL*)d_tmp1, (const REAL*)d_tmp0, (uint32_t)n_layers);
        if (!on_device) return copy_out(out, dst, n_layers * sizeof(REAL), 0);
        HIPCHK(hipStreamSynchronize(stream));
        return BDDMMA_OK;
    }
    int bdds_solution(int sorted, char* sol, int on_device) override
    {
        HIPCHK(hipSetDevice(device));
        int rc;
        if ((rc = backward_run())) return rc;
        HIPCHK(hipMemsetAsync(d_sol, 0, n_layers, stream));
        if ((rc = launch_fwd(FWD_SOLUTION, nullptr, REAL(0), BDDMMA_K_OTHER))) return rc;
        // (fwd_valid stays what it was: the solution sweep recomputes the costs-from-root on the fly and does not store them)
        const hipMemcpyKind k = on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
        if (!sorted) {
            HIPCHK(hipMemcpyAsync(sol, d_sol, n_layers, k, stream));
            HIPCHK(hipStreamSynchronize(stream));
            return BDDMMA_OK;
        }
        char* s = nullptr;
        HIPCHK(hipMalloc((void**)&s, std::max<uint64_t>(n_layers, 1)));
        hipLaunchKernelGGL((k_gather<char>), dim3(cdiv(n_layers, 256)), dim3(256), 0, stream, d_sol, d_var_layers, s, (uint32_t)n_layers);
        hipError_t e = hipMemcpyAsync(sol, s, n_layers, k, stream);
        if (e == hipSuccess) e = hipStreamSynchronize(stream);
        (void)hipFree(s);
        HIPCHK(e);
        return BDDMMA_OK;
    }
    int bdds_solution_async(char* dev_out, int prezeroed) override
    {
        HIPCHK(hipSetDevice(device));
        int rc;
        if ((rc = backward_run())) return rc;
        if (!prezeroed) HIPCHK(hipMemsetAsync(dev_out, 0, n_layers, stream));
        char* const own = d_sol;
        d_sol = dev_out;  // ptrs() hands d_sol to the sweep
        rc = launch_fwd(FWD_SOLUTION, nullptr, REAL(0), BDDMMA_K_OTHER);
        d_sol = own;
        if (rc) return rc;
        return BDDMMA_OK;
    }
    int lbfgs_views(LbfgsViews* out) override
    {
        HIPCHK(hipSetDevice(device));
        int rc;
        if (!d_x_layer && (rc = dalloc(&d_x_layer, n_layers))) return rc;
        if (!x_layer_valid) {  // the first call, or something other than a backward solve sweep has changed costs / deferred values since
            hipLaunchKernelGGL((k_net_costs<REAL>), dim3(cdiv(n_layers, 256)), dim3(256), 0, stream, d_lo, d_hi, d_mm_binned, d_lpos, d_x_layer, (uint32_t)n_layers);
            HIPCHK(hipGetLastError());
            x_layer_valid = true;
        }
        *out = LbfgsViews{d_x_layer};
        return BDDMMA_OK;
    }
    int net_solver_costs(void* out, int on_device) override
    {
        HIPCHK(hipSetDevice(device));
        REAL* dst = on_device ? (REAL*)out : d_tmp0;
        hipLaunchKernelGGL((k_net_costs<REAL>), dim3(cdiv(n_layers, 256)), dim3(256), 0, stream, d_lo, d_hi, d_mm_binned, d_lpos, dst, (uint32_t)n_layers);
        if (!on_device) return copy_out(out, dst, n_layers * sizeof(REAL), 0);
        HIPCHK(hipGetLastError());
        return BDDMMA_OK;
    }
    int make_dual_feasible(void* g, int on_device) override
    {
        HIPCHK(hipSetDevice(device));
        REAL* p = (REAL*)g;
        if (!on_device) { p = d_tmp0; HIPCHK(hipMemcpyAsync(p, g, n_layers * sizeof(REAL), hipMemcpyHostToDevice, stream)); }
        hipLaunchKernelGGL((k_make_dual_feasible<REAL>), dim3(cdiv(n_vars, 256)), dim3(256), 0, stream, p, d_var_ptr, d_var_layers, (uint32_t)n_vars);
        if (!on_device) return copy_out(g, p, n_layers * sizeof(REAL), 0);
        HIPCHK(hipGetLastError());
        return BDDMMA_OK;
    }
    int gradient_step(const void* g, double step, int on_device) override
    {
        HIPCHK(hipSetDevice(device));
        const REAL* p = (const REAL*)g;
        if (!on_device) { HIPCHK(hipMemcpyAsync(d_tmp0, g, n_layers * sizeof(REAL), hipMemcpyHostToDevice, stream)); p = d_tmp0; }
        hipLaunchKernelGGL((k_gradient_step<REAL>), dim3(cdiv(n_layers, 256)), dim3(256), 0, stream, d_hi, p, REAL(step), (uint32_t)n_layers);
        costs_changed();
        HIPCHK(hipGetLastError());
        return BDDMMA_OK;
    }
    // make_dual_feasible + gradient_step for a device vector that is only applied, never read back (lbfgs.hip).
    // Large instances (>= 500 k layers; variant_flags bit 9 forces it, bit 10 forbids it): the vector goes through the staging tables
    // to entry order, is projected per bin in LDS and comes back to layer order together with the first step (kernels.hpp:
    // k_stage_transpose / k_project_entries) — then every further step is a plain stream.  Small ones: the per-variable means by gather ...
    REAL* d_proj_q = nullptr;
    REAL* d_proj_dir = nullptr;     // the projected vector in layer order (staged path)
    REAL* d_proj_ent = nullptr;     // ... and in entry order
    bool proj_staged = false;       // the last projection_means took the staged path
    bool proj_pending = false;      // ... and its way back to layer order is still to be done (with the first step)
    const void* proj_of = nullptr;  // the vector the last projection_means was called on
    bool use_staged_projection() const
    {
        if (opts_variant & 0x400u) return false;
        if (n_narrow_layers == 0) return false;
        return (opts_variant & 0x200u) != 0 || n_layers >= 500000;
    }
    void launch_stage_transpose(int to_layers, const REAL* in, REAL* out, REAL* lohi, REAL step)
    {
        const Kern<TransFn>& k = kern.transpose[to_layers];
        hipLaunchKernelGGL(k.fn, dim3(cdiv(nb_.n_packs, wpb)), dim3(64 * wpb), k.lds, stream, in, out, pdev(nb_, 0), (const uint32_t*)d_cs_entry,
                           (const uint16_t*)d_cs_slot, n_narrow_layers, (uint32_t)n_layers, lohi, step);
    }
    // x_e -= mean over the entries of its variable (d_proj_ent, in place); the way back to layer order is then pending
    void launch_project_entries()
    {
        hipLaunchKernelGGL(kern.project.fn, dim3(n_bins), dim3(kern.ex_threads), kern.project.lds, stream, d_proj_ent, d_bin_ptr, d_bvar, d_nbdds, vars_per_bin,
                           (uint32_t)n_vars, (uint32_t)n_layers);
        proj_pending = true;
    }
    int projection_means(const void* g) override
    {
        HIPCHK(hipSetDevice(device));
        int rc;
        proj_staged = use_staged_projection();
        proj_pending = false;
        proj_of = g;
        if (!proj_staged) {
            if (!d_proj_q && (rc = dalloc(&d_proj_q, n_vars))) return rc;
            hipLaunchKernelGGL((k_projection_means<REAL>), dim3(cdiv(n_vars, 256)), dim3(256), 0, stream, (const REAL*)g, d_var_ptr, d_var_layers, d_proj_q, (uint32_t)n_vars);
            HIPCHK(hipGetLastError());
            return BDDMMA_OK;
        }
        if (!d_proj_dir && (rc = dalloc(&d_proj_dir, n_layers))) return rc;
        if (!d_proj_ent && (rc = dalloc(&d_proj_ent, n_layers))) return rc;
        // layers -> entries 
        launch_stage_transpose(0, (const REAL*)g, d_proj_ent, (REAL*)nullptr, REAL(0));
        if (n_layers > n_narrow_layers)
            hipLaunchKernelGGL((k_layers_to_entries<REAL>), dim3(cdiv(n_layers - n_narrow_layers, 256)), dim3(256), 0, stream, (const REAL*)g + n_narrow_layers,
                               d_lpos + n_narrow_layers, d_proj_ent, (uint32_t)(n_layers - n_narrow_layers));
        launch_project_entries();
        HIPCHK(hipGetLastError());
        return BDDMMA_OK;
    }
    // The same for a vector that is a linear combination of stored ones (the L-BFGS direction): formed inside the layers -> entries pass
    // (kernels.hpp: k_stage_lincomb).  Instances of narrow packs only; variant_flags bit 15: not offered (the wrapper writes the direction
    // and calls projection_means).
    bool projection_fuses_lincomb() const override { return use_staged_projection() && n_layers == n_narrow_layers && !(opts_variant & 0x8000u); }
    int projection_means_lincomb(const LinComb& lc, const void* tag) override
    {
        HIPCHK(hipSetDevice(device));
        int rc;
        if (!projection_fuses_lincomb() || lc.ns < 1 || lc.ns > LINCOMB_MAX) { err = "projection_means_lincomb: not available for this instance"; return BDDMMA_ERR_INVALID_ARGUMENT; }
        proj_staged = true;
        proj_pending = false;
        proj_of = tag;
        if (!d_proj_dir && (rc = dalloc(&d_proj_dir, n_layers))) return rc;
        if (!d_proj_ent && (rc = dalloc(&d_proj_ent, n_layers))) return rc;
        const Kern<LincombFn>& k = kern.lincomb[lc.ns == 5];
        hipLaunchKernelGGL(k.fn, dim3(cdiv(nb_.n_packs, wpb)), dim3(64 * wpb), k.lds, stream, lc, d_proj_ent, pdev(nb_, 0), (const uint32_t*)d_cs_entry,
                           (const uint16_t*)d_cs_slot, n_narrow_layers, (uint32_t)n_layers);
        launch_project_entries();
        HIPCHK(hipGetLastError());
        return BDDMMA_OK;
    }
    // ... then any number of steps along the projected vector
    int gradient_step_projected(const void* g, double step) override
    {
        HIPCHK(hipSetDevice(device));
        if (g != proj_of) { err = "gradient_step_projected: not the vector projection_means was called on"; return BDDMMA_ERR_INVALID_ARGUMENT; }
        if (proj_staged) {
            if (proj_pending) {
                // entries -> layers, with this step applied on the way
                launch_stage_transpose(1, (const REAL*)d_proj_ent, d_proj_dir, d_lohi, REAL(step));
                if (n_layers > n_narrow_layers) {
                    const uint32_t nw = (uint32_t)(n_layers - n_narrow_layers);
                    hipLaunchKernelGGL((k_entries_to_layers<REAL>), dim3(cdiv(nw, 256)), dim3(256), 0, stream, (const REAL*)d_proj_ent, d_lpos + n_narrow_layers,
                                       d_proj_dir + n_narrow_layers, nw);
                    hipLaunchKernelGGL((k_gradient_step<REAL>), dim3(cdiv(nw, 256)), dim3(256), 0, stream, d_hi + 2 * (size_t)n_narrow_layers,
                                       (const REAL*)d_proj_dir + n_narrow_layers, REAL(step), nw);
                }
                proj_pending = false;
            } else {
                hipLaunchKernelGGL((k_gradient_step<REAL>), dim3(cdiv(n_layers, 256)), dim3(256), 0, stream, d_hi, (const REAL*)d_proj_dir, REAL(step), (uint32_t)n_layers);
            }
            costs_changed();
            HIPCHK(hipGetLastError());
            return BDDMMA_OK;
        }
        if (!d_proj_q) { err = "gradient_step_projected without projection_means"; return BDDMMA_ERR_INVALID_ARGUMENT; }
        hipLaunchKernelGGL((k_gradient_step_projected<REAL>), dim3(cdiv(n_layers, 256)), dim3(256), 0, stream, d_hi, (const REAL*)g, d_proj_q, (const uint32_t*)d_var, REAL(step), (uint32_t)n_layers);
        costs_changed();
        HIPCHK(hipGetLastError());
        return BDDMMA_OK;
    }
    void* stream_handle() override { return (void*)stream; }
    int rounding_scratch(void** c0_dev, void** c1_dev) override
    {
        *c0_dev = d_delta_c;
        *c1_dev = d_delta_c + n_vars;
        return BDDMMA_OK;
    }
    int rounding_round(double delta, uint32_t round, uint32_t seed, uint32_t counts[4], char* sol_host, void* c0_host, void* c1_host,
                       bool apply_update, int* applied) override
    {
        HIPCHK(hipSetDevice(device));
        int rc;
        *applied = 0;
        if ((rc = distribute_delta())) return rc;                 // :265
        if ((rc = forward_run())) return rc;                      // min_marginals_cuda(), :266
        if ((rc = launch_bwd(BWD_MARGINALS, nullptr, REAL(0), BDDMMA_K_OTHER))) return rc;
        bwd_valid = lb_valid = true;
        HIPCHK(hipMemsetAsync(d_counts, 0, 4 * sizeof(uint32_t), stream));
        REAL* c0 = d_delta_c;               // 2V scratch: [0,V) cost_delta_0, [V,2V) cost_delta_1
        REAL* c1 = d_delta_c + n_vars;
        hipLaunchKernelGGL((k_round_perturb<REAL>), dim3(cdiv(n_vars, 256)), dim3(256), 0, stream, d_tmp0, d_tmp1, d_var_ptr, d_var_layers,
                           c0, c1, d_sol, d_counts, (uint32_t)n_vars, delta, round, seed);
        HIPCHK(hipMemcpyAsync(counts, d_counts, 4 * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
        if (c0_host) HIPCHK(hipMemcpyAsync(c0_host, c0, n_vars * sizeof(REAL), hipMemcpyDeviceToHost, stream));
        if (c1_host) HIPCHK(hipMemcpyAsync(c1_host, c1, n_vars * sizeof(REAL), hipMemcpyDeviceToHost, stream));
        HIPCHK(hipStreamSynchronize(stream));
        if ((uint64_t)counts[0] + counts[1] == n_vars) {          // all min-marginals agree: read off the solution, :295-305
            HIPCHK(hipMemcpyAsync(sol_host, d_sol, n_vars, hipMemcpyDeviceToHost, stream));
            HIPCHK(hipStreamSynchronize(stream));
            return BDDMMA_OK;
        }
        *applied = 1;
        if (!apply_update) return BDDMMA_OK;                        // the caller applies it (through the L-BFGS wrapper)
        return update_costs(c0, n_vars, c1, n_vars, precision, 1);  // :327
    }
    // STREAM triad / copy over temporary BDDMMA_TRIAD_BYTES arrays (n4 is a multiple of 4 * grid * 256)
    int time_stream(bool copy, uint64_t reps, double* ms)
    {
        const uint64_t n4 = BDDMMA_TRIAD_BYTES / 16;
        stream_v4 *a = nullptr, *b = nullptr, *c = nullptr;
        HIPCHK(hipMalloc(&a, BDDMMA_TRIAD_BYTES));
        HIPCHK(hipMalloc(&b, BDDMMA_TRIAD_BYTES));
        HIPCHK(hipMalloc(&c, BDDMMA_TRIAD_BYTES));
        HIPCHK(hipMemsetAsync(b, 0, BDDMMA_TRIAD_BYTES, stream));
        HIPCHK(hipMemsetAsync(c, 0, BDDMMA_TRIAD_BYTES, stream));
        const unsigned grid = (unsigned)((n4 + 255) / 256);  // one vector per thread (kernels.hpp: k_stream)
        auto once = [&]() {
            if (copy) k_stream<true><<<grid, 256, 0, stream>>>(a, b, c, 3.0f, n4);
            else k_stream<false><<<grid, 256, 0, stream>>>(a, b, c, 3.0f, n4);
        };
        once();
        HIPCHK(hipEventRecord(ev_t0, stream));
        for (uint64_t i = 0; i < reps; ++i) once();
        HIPCHK(hipEventRecord(ev_t1, stream));
        HIPCHK(hipEventSynchronize(ev_t1));
        float f = 0.f;
        HIPCHK(hipEventElapsedTime(&f, ev_t0, ev_t1));
        *ms = f;
        HIPCHK(hipFree(a));
        HIPCHK(hipFree(b));
        HIPCHK(hipFree(c));
        return BDDMMA_OK;
    }

    int time_kernel(int kind, uint64_t reps, double* ms) override
    {
        HIPCHK(hipSetDevice(device));
        if (kind >= 13 && kind <= 17) return gi_time_kernel(kind, reps, ms);
        int rc = BDDMMA_OK;
        auto once = [&]() -> int {
#ifdef BDDMMA_STAMPS
            // BDDMMA_STAMPS_ONCHIP: kinds 2 / 3 launch the solve sweeps iteration() runs (kernels/narrow4.hpp) instead of the third generation's
            if ((kind == 2 || kind == 3) && onchip_hc && std::getenv("BDDMMA_STAMPS_ONCHIP"))
                return launch_sweep(kind == 3, kern.onchip[kind - 2], d_delta_lay, REAL(0.5), BDDMMA_K_OTHER);
#endif
            switch (kind) {
                case 0: return launch_fwd(FWD_PLAIN, nullptr, REAL(0), BDDMMA_K_OTHER);
                case 1: return launch_bwd(BWD_PLAIN, nullptr, REAL(0), BDDMMA_K_OTHER);
                case 2: return launch_fwd(FWD_SOLVE, d_delta_lay, REAL(0.5), BDDMMA_K_OTHER);
                case 3: return launch_bwd(BWD_SOLVE, d_delta_lay, REAL(0.5), BDDMMA_K_OTHER);
                case 4: return exchange();
                case 5: launch_bcast(d_delta_c, d_delta_lay_c); return BDDMMA_OK;
                case 8: return sm_launch_fwd();
                case 9: return sm_launch_bwd();
                case 10: return gr_launch_down();
                case 11: return gr_launch_up();
                case 12: { const int r = gr_launch_down(); return r ? r : gr_launch_up(); }
                default: err = "unknown kernel kind"; return BDDMMA_ERR_INVALID_ARGUMENT;
            }
        };
        if (kind == 6 || kind == 7) return time_stream(kind == 7, reps, ms);
        if ((kind == 8 || kind == 9) && (rc = sm_prepare())) return rc;
        if (kind == 9 && (rc = sm_launch_fwd())) return rc;  // the backward sum sweep reads the forward one's log-partition values
        if (kind >= 10 && kind <= 12) {  // the gradient sweeps read the plain potentials, a gradient (zero here) and, upwards, the arg-min slots
            if ((rc = gr_prepare()) || (rc = forward_run()) || (rc = backward_run())) return rc;
            HIPCHK(hipMemsetAsync(d_gr_in0, 0, n_layers * sizeof(REAL), stream));
            if (kind == 11 && (rc = gr_launch_down())) return rc;
        }
        if ((rc = once())) return rc;  // warm-up
        HIPCHK(hipEventRecord(ev_t0, stream));
        for (uint64_t i = 0; i < reps; ++i)
            if ((rc = once())) return rc;
        HIPCHK(hipEventRecord(ev_t1, stream));
        HIPCHK(hipEventSynchronize(ev_t1));
        float f = 0.f;
        HIPCHK(hipEventElapsedTime(&f, ev_t0, ev_t1));
        *ms = f;
        costs_changed();
        x_layer_valid = false;
#ifdef BDDMMA_STAMPS
        if (const char* path = std::getenv("BDDMMA_STAMPS_FILE")) {  // one more launch with per-wave phase stamps (kernels.hpp: BDDMMA_STAMP)
            const size_t slots = 0x100000u + 65536u * 16u;
            unsigned long long* d_st = nullptr;
            HIPCHK(hipMalloc((void**)&d_st, slots * 8 * sizeof(unsigned long long)));
            HIPCHK(hipMemset(d_st, 0, slots * 8 * sizeof(unsigned long long)));
            HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(g_bddmma_stamps), &d_st, sizeof(d_st)));
            HIPCHK(hipStreamSynchronize(stream));
            rc = once();
            HIPCHK(hipStreamSynchronize(stream));
            unsigned long long* null_ = nullptr;
            HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(g_bddmma_stamps), &null_, sizeof(null_)));
            std::vector<unsigned long long> h(slots * 8);
            HIPCHK(hipMemcpy(h.data(), d_st, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
            (void)hipFree(d_st);
            if (FILE* f2 = std::fopen((std::string(path) + "." + std::to_string(kind)).c_str(), "w")) {
                for (size_t sl = 0; sl < slots; ++sl)
                    if (h[sl * 8] != 0)
                        std::fprintf(f2, "%zu %llu %llu %llu %llu %llu %llu\n", sl, h[sl * 8], h[sl * 8 + 1], h[sl * 8 + 2], h[sl * 8 + 3], h[sl * 8 + 4], h[sl * 8 + 5]);
                std::fclose(f2);
            }
            if (rc) return rc;
        }
#endif
        return BDDMMA_OK;
    }
};

}  // namespace bddmma
