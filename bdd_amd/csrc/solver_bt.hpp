// solver_bt.hpp — BatchT<REAL>: many one-workgroup instances in one launch (solver.hpp: BatchBase; kernels/small.hpp:
// k_iterate_small_batch).  Included by solver_bt_f32.hip / solver_bt_f64.hip only, so that the batch kernels compile in translation units of
// their own.
#pragma once
#include <algorithm>
#include <mutex>

#include "solver_impl.hpp"
#include "kernels/gradsmall.hpp"
#include "kernels/batchcosts.hpp"
#include "kernels/batchlb.hpp"
#include "kernels/batchbound.hpp"
#include "kernels/batchmm.hpp"
#include "kernels/batchsm.hpp"
#include "kernels/batchround.hpp"
#include "kernels/batchsol.hpp"
#include "kernels/smallhist.hpp"
#include "kernels/smallstop.hpp"

namespace bddmma {

template <typename REAL>
struct BatchT final : BatchBase {
    using S = SolverT<REAL>;
    using Fn = void (*)(const SmallItem<REAL>*, REAL, uint32_t);
    // The members in the caller's order; item j of the device arrays (items, control blocks, published bounds) is member order[j]: the items
    // are sorted by the instantiation the member's solver chose (small_nw x small_rl), so that each group is one contiguous launch.
    std::vector<S*> m;
    std::vector<uint32_t> order;
    struct Group {
        Fn fn;
        uint32_t threads, lds, first, count;   // lds: the largest small_lds of the group
    };
    std::vector<Group> groups;
    int device = -1;
    hipStream_t stream = nullptr;
    std::vector<hipEvent_t> ev_in;             // one per member: recorded on the member's stream on entry
    hipEvent_t ev_out = nullptr, ev_chunk[2] = {nullptr, nullptr};
    hipEvent_t ev_t0 = nullptr, ev_t1 = nullptr;   // time_iterations (created on first use)
    SmallItem<REAL>* d_items = nullptr;
    RunCtl *d_ctl = nullptr, *h_ctl = nullptr;           // h_ctl: pinned staging of the control blocks' initial values
    RunHost *h_run = nullptr, *d_run_host = nullptr;     // pinned + its device address: what the members' workgroups publish

    ~BatchT() override
    {
        // (the members are not touched: they may be gone already — the caller's error, but not one to crash on)
        if (device >= 0) (void)hipSetDevice(device);
        if (stream) (void)hipStreamSynchronize(stream);
        for (hipEvent_t e : ev_in) (void)hipEventDestroy(e);
        for (hipEvent_t e : {ev_out, ev_chunk[0], ev_chunk[1], ev_t0, ev_t1, ev_order})
            if (e) (void)hipEventDestroy(e);
        if (d_items) (void)hipFree(d_items);
        for (void* q : {(void*)d_hs_items, (void*)d_hs_stage, (void*)d_st_items, (void*)d_st_blocks, (void*)d_ln_items, (void*)d_ln_tab, (void*)d_ln_in, (void*)d_ln_bad, (void*)d_gs_items, (void*)d_gs_ws, (void*)d_gs_io, (void*)d_gs_bad, (void*)d_gs_cnt, (void*)d_bc_items, (void*)d_bc_stage, (void*)d_bl_words, (void*)d_bb_items, (void*)d_bb_stage, (void*)d_bb_bad, (void*)d_bm_items, (void*)d_bm_stage, (void*)d_bm_bad, (void*)d_bsm_items, (void*)d_bsm_stage, (void*)d_br_items, (void*)d_br_words, (void*)d_bp_items, (void*)d_bp_stage, (void*)d_bp_bad})
            if (q) (void)hipFree(q);
        if (d_ctl) (void)hipFree(d_ctl);
        if (h_ctl) (void)hipHostFree(h_ctl);
        if (h_run) (void)hipHostFree(h_run);
        if (h_br_words) (void)hipHostFree(h_br_words);
        if (h_bl_out) (void)hipHostFree(h_bl_out);
        if (stream) (void)hipStreamDestroy(stream);
    }
    uint64_t size() const override { return m.size(); }

    static Fn batch_fn(int nw, bool rl)
    {
        return pick<1, 2, 4, 8, 16>((uint32_t)nw, [&](auto NW) -> Fn {
            return rl ? &k_iterate_small_batch<REAL, NW.value, true> : &k_iterate_small_batch<REAL, NW.value, false>;
        });
    }
    // The dynamic-LDS limit of a batch kernel is a property of the function, shared by every batch of the process: it is only ever raised
    // (a limit is not a reservation), so that a later batch of smaller members does not take it away from an earlier one.
    int raise_lds_limit(const void* fn, uint32_t lds)
    {
        static std::mutex mtx;
        static std::vector<std::pair<const void*, uint32_t>> limits;
        std::lock_guard<std::mutex> lock(mtx);
        auto it = std::find_if(limits.begin(), limits.end(), [&](const std::pair<const void*, uint32_t>& e) { return e.first == fn; });
        if (it != limits.end() && it->second >= lds) return BDDMMA_OK;
        HIPCHK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        if (it != limits.end()) it->second = lds;
        else limits.push_back({fn, lds});
        return BDDMMA_OK;
    }

    int init(SolverBase* const* members, uint64_t n)
    {
        m.resize(n);
        for (uint64_t i = 0; i < n; ++i) m[i] = static_cast<S*>(members[i]);
        device = m[0]->device;
        if (int rc = check_state()) return rc;
        order.resize(n);
        for (uint32_t i = 0; i < n; ++i) order[i] = i;
        auto key = [&](uint32_t i) { return (uint32_t)m[i]->small_nw * 2u + (m[i]->small_rl ? 1u : 0u); };
        std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return key(a) < key(b); });
        std::vector<SmallItem<REAL>> items(n);
        for (uint32_t j = 0; j < n; ++j) {
            const S* s = m[order[j]];
            items[j] = s->small_item();
            if (groups.empty() || key(order[j]) != key(order[groups.back().first]))
                groups.push_back(Group{batch_fn(s->small_nw, s->small_rl), 64u * (uint32_t)s->small_nw, 0u, j, 0u});
            Group& g = groups.back();
            g.lds = std::max(g.lds, s->small_lds);
            ++g.count;
        }
        HIPCHK(hipSetDevice(device));
        for (const Group& g : groups)
            if (int rc = raise_lds_limit(reinterpret_cast<const void*>(g.fn), g.lds)) return rc;
        HIPCHK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
        ev_in.assign(n, nullptr);
        for (hipEvent_t& e : ev_in) HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        HIPCHK(hipEventCreateWithFlags(&ev_out, hipEventDisableTiming));
        for (hipEvent_t& e : ev_chunk) HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        HIPCHK(hipMalloc((void**)&d_items, n * sizeof(SmallItem<REAL>)));
        HIPCHK(hipMalloc((void**)&d_ctl, n * sizeof(RunCtl)));
        HIPCHK(hipHostMalloc((void**)&h_ctl, n * sizeof(RunCtl), hipHostMallocDefault));
        HIPCHK(hipHostMalloc((void**)&h_run, n * sizeof(RunHost), hipHostMallocMapped | hipHostMallocCoherent));
        HIPCHK(hipHostGetDevicePointer((void**)&d_run_host, h_run, 0));
        HIPCHK(hipMemcpy(d_items, items.data(), n * sizeof(SmallItem<REAL>), hipMemcpyHostToDevice));
        return BDDMMA_OK;
    }

    // per call, before anything is launched: what small_usable() asks of a solver, for every member
    int check_state()
    {
        for (size_t i = 0; i < m.size(); ++i) {
            const char* why = m[i]->profiling                                        ? "profiling is on"
                              : (*m[i]->lbfgs_attached > 0 || m[i]->d_x_layer != nullptr) ? "an L-BFGS wrapper is or was attached (its backward sweeps write x per layer)"
                              : m[i]->run_stop != nullptr                            ? "run_solver is in progress"
                                                                                     : nullptr;
            if (why) {
                err = "batch member " + std::to_string(i) + ": " + why;
                return BDDMMA_ERR_STATE;
            }
        }
        return BDDMMA_OK;
    }
    // entry: members whose costs-to-terminal are stale get their own backward_run() first, as launch_small does; then the batch stream waits
    // for everything queued on every member's stream
    int join_in()
    {
        for (size_t i = 0; i < m.size(); ++i)
            if (!masked(i))
                if (int rc = m[i]->backward_run()) { err = m[i]->err; return rc; }
        for (size_t i = 0; i < m.size(); ++i) {
            HIPCHK(hipEventRecord(ev_in[i], m[i]->stream));
            HIPCHK(hipStreamWaitEvent(stream, ev_in[i], 0));
        }
        return BDDMMA_OK;
    }
    // run_plain's optional mask (member order), set for the duration of that call only: a masked member runs no iteration and keeps its
    // host-side state
    const char* run_mask = nullptr;
    bool masked(size_t i) const { return run_mask != nullptr && run_mask[i] != 0; }
    // exit: every member's stream waits for what the batch stream holds now
    int join_out()
    {
        HIPCHK(hipEventRecord(ev_out, stream));
        for (S* s : m) HIPCHK(hipStreamWaitEvent(s->stream, ev_out, 0));
        return BDDMMA_OK;
    }
    int refresh(bool run, uint32_t run_iter)
    {
        const uint32_t n = (uint32_t)m.size();
        hipLaunchKernelGGL((k_small_items_refresh<REAL>), dim3(cdiv(n, 256)), dim3(256), 0, stream, d_items, n, run ? d_ctl : (RunCtl*)nullptr, d_run_host, run_iter);
        HIPCHK(hipGetLastError());
        return BDDMMA_OK;
    }
    // one launch per group: the group's member count as the grid, its largest small_lds as the dynamic LDS
    int launch(REAL omega, uint32_t n_iters)
    {
        for (const Group& g : groups) {
            hipLaunchKernelGGL(g.fn, dim3(g.count), dim3(g.threads), g.lds, stream, (const SmallItem<REAL>*)(d_items + g.first), omega, n_iters);
            HIPCHK(hipGetLastError());
        }
        for (size_t i = 0; i < m.size(); ++i)
            if (!masked(i)) m[i]->small_launched();
        return BDDMMA_OK;
    }

    int iterations(double omega, uint64_t n) override { return iterations_timed(omega, n, nullptr); }
    // ms non-null: hipEvents on the batch stream around the launches, from the first to the last (the joins are outside); waits for them
    int iterations_timed(double omega, uint64_t n, double* ms)
    {
        int rc;
        if ((rc = check_state())) return rc;
        if (ms) *ms = 0.0;
        if (n == 0) return BDDMMA_OK;
        HIPCHK(hipSetDevice(device));
        if (ms && !ev_t0) {
            HIPCHK(hipEventCreate(&ev_t0));
            HIPCHK(hipEventCreate(&ev_t1));
        }
        if ((rc = join_in())) return rc;
        if (ms) HIPCHK(hipEventRecord(ev_t0, stream));
        if ((rc = refresh(false, 0))) return rc;
        while (n) {
            const uint32_t chunk = (uint32_t)std::min<uint64_t>(n, 1u << 14);   // as SolverT::iterations
            if ((rc = launch((REAL)omega, chunk))) break;
            n -= chunk;
        }
        if (ms && !rc) HIPCHK(hipEventRecord(ev_t1, stream));
        const int rc2 = join_out();   // also behind a failed launch: what was queued stays ordered
        if (rc || rc2) return rc ? rc : rc2;
        if (ms) {
            float f = 0.f;
            HIPCHK(hipEventSynchronize(ev_t1));
            HIPCHK(hipEventElapsedTime(&f, ev_t0, ev_t1));
            *ms = f;
        }
        return BDDMMA_OK;
    }
    int time_iterations(double omega, uint64_t n, double* ms) override { return iterations_timed(omega, n, ms); }

    // ---- learned iterations (kernels/small.hpp: k_learned_small_batch; the kernels themselves compile in solver_sl_f32.hip / _f64.hip)
    // Items and groups of their own: a member's learned form chooses records-in-LDS on its own budget, so the groups may differ from the
    // plain ones.  Built by the first call (the members' weight and omega buffers are allocated then).  ln_tab[i] is member i's row of
    // k_batch_learn_load, in the caller's order, as the concatenated inputs are.
    using LnFn = typename S::SmallLnBatchFn;
    struct LnGroup {
        LnFn fn;
        uint32_t threads, lds, first, count;
    };
    std::vector<LnGroup> ln_groups;
    SmallLearnItem<REAL>* d_ln_items = nullptr;
    LearnLoad<REAL>* d_ln_tab = nullptr;
    REAL* d_ln_in = nullptr;       // host inputs on the device: weights | omega_vec, ln_total values each
    uint32_t* d_ln_bad = nullptr;  // k_batch_learn_load's two words
    std::vector<uint64_t> ln_src;  // first value of member i in the inputs
    uint64_t ln_total = 0;
    bool ln_ready = false;

    int ln_prepare()
    {
        const uint32_t n = (uint32_t)m.size();
        std::vector<uint32_t> ord(n);
        for (uint32_t i = 0; i < n; ++i) ord[i] = i;
        auto key = [&](uint32_t i) { return (uint32_t)m[i]->small_nw * 2u + (m[i]->small_ln_rl ? 1u : 0u); };
        std::stable_sort(ord.begin(), ord.end(), [&](uint32_t a, uint32_t b) { return key(a) < key(b); });
        for (S* s : m) {
            int rc = BDDMMA_OK;
            if (!s->d_alpha_ent) rc = s->dalloc(&s->d_alpha_ent, s->n_layers);
            if (!rc && !s->d_omega_lay) rc = s->dalloc(&s->d_omega_lay, s->n_layers);
            if (rc) { err = s->err; return rc; }
        }
        std::vector<SmallLearnItem<REAL>> items(n);
        std::vector<LnGroup> groups_;
        for (uint32_t j = 0; j < n; ++j) {
            const S* s = m[ord[j]];
            items[j] = s->small_learn_item();
            if (groups_.empty() || key(ord[j]) != key(ord[groups_.back().first]))
                groups_.push_back(LnGroup{S::sl_batch_fn(s->small_nw, s->small_ln_rl), 64u * (uint32_t)s->small_nw, 0u, j, 0u});
            LnGroup& g = groups_.back();
            g.lds = std::max(g.lds, s->small_ln_lds);
            ++g.count;
        }
        for (const LnGroup& g : groups_)
            if (int rc = raise_lds_limit(reinterpret_cast<const void*>(g.fn), g.lds)) return rc;
        std::vector<LearnLoad<REAL>> tab(n);
        ln_src.assign(n, 0);
        ln_total = 0;
        for (uint32_t i = 0; i < n; ++i) {
            ln_src[i] = ln_total;
            tab[i] = LearnLoad<REAL>{m[i]->d_lpos, m[i]->d_alpha_ent, m[i]->d_omega_lay, (uint32_t)ln_total, (uint32_t)m[i]->n_layers};
            ln_total += m[i]->n_layers;
        }
        HIPCHK(hipMalloc((void**)&d_ln_items, n * sizeof(SmallLearnItem<REAL>)));
        HIPCHK(hipMalloc((void**)&d_ln_tab, n * sizeof(LearnLoad<REAL>)));
        HIPCHK(hipMalloc((void**)&d_ln_in, 2 * ln_total * sizeof(REAL)));
        HIPCHK(hipMalloc((void**)&d_ln_bad, 2 * sizeof(uint32_t)));
        HIPCHK(hipMemcpy(d_ln_items, items.data(), n * sizeof(SmallLearnItem<REAL>), hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(d_ln_tab, tab.data(), n * sizeof(LearnLoad<REAL>), hipMemcpyHostToDevice));
        ln_groups = std::move(groups_);
        return BDDMMA_OK;
    }
    int launch_learned(REAL omega, uint32_t n_iters, bool ov)
    {
        for (const LnGroup& g : ln_groups) {
            hipLaunchKernelGGL(g.fn, dim3(g.count), dim3(g.threads), g.lds, stream, (const SmallLearnItem<REAL>*)(d_ln_items + g.first), omega, n_iters, ov ? 1u : 0u);
            HIPCHK(hipGetLastError());
        }
        for (S* s : m) s->small_launched();
        return BDDMMA_OK;
    }
    // ---- ... with their history (kernels/smallhist.hpp: k_learned_small_hist_batch; the kernels compile in solver_sh_f32.hip / _f64.hip)
    // Items in the learned groups' order (the same key: waves x records in LDS); a member's two bounds that cross launches live in its
    // d_hist, allocated here before any member is touched.  Host outputs pass through hs_stage (sol_avg | lb_first | lb_second).
    using HsFn = typename S::SmallHistFn;
    std::vector<HsFn> hs_fn;       // per learned group
    SmallHistItem<REAL>* d_hs_items = nullptr;
    REAL* d_hs_stage = nullptr;
    uint64_t hs_bdds = 0;          // BDDs of all members
    bool hs_ready = false;
    std::vector<SmallHistItem<REAL>> hs_items;   // what d_hs_items was filled with, and the member of each (learned_iterations_stop builds on both)
    std::vector<uint32_t> hs_ord;

    int hs_prepare()
    {
        const uint32_t n = (uint32_t)m.size();
        std::vector<uint32_t> ord(n);
        for (uint32_t i = 0; i < n; ++i) ord[i] = i;
        auto key = [&](uint32_t i) { return (uint32_t)m[i]->small_nw * 2u + (m[i]->small_ln_rl ? 1u : 0u); };
        std::stable_sort(ord.begin(), ord.end(), [&](uint32_t a, uint32_t b) { return key(a) < key(b); });   // ln_prepare's order
        std::vector<uint64_t> src_b(n);
        uint64_t total_b = 0;
        for (uint32_t i = 0; i < n; ++i) {
            src_b[i] = total_b;
            total_b += m[i]->n_bdds;
        }
        if (ln_total > 0xFFFFFFFFull || total_b > 0xFFFFFFFFull) { err = "batch learned_iterations: too many layers"; return BDDMMA_ERR_UNSUPPORTED; }
        for (S* s : m)
            if (!s->d_hist)
                if (int rc = s->dalloc(&s->d_hist, s->n_layers + 5 * s->n_bdds)) { err = s->err; return rc; }
        std::vector<SmallHistItem<REAL>> items(n);
        for (uint32_t j = 0; j < n; ++j) {
            const S* s = m[ord[j]];
            // (of d_hist's L + 5 B values the per-member call uses all; it starts every call afresh, as this one does)
            // (the outputs and beta: k_hist_items_call, per call)
            items[j] = SmallHistItem<REAL>{s->small_learn_item(),
                                           SmallHistMem<REAL>{s->d_root_slot, s->d_hist + s->n_layers, nullptr, nullptr, nullptr, (uint32_t)s->n_bdds, REAL(0)},
                                           (uint32_t)ln_src[ord[j]], (uint32_t)src_b[ord[j]]};
        }
        std::vector<HsFn> fns;
        for (const LnGroup& g : ln_groups) {
            const S* s = m[ord[g.first]];
            fns.push_back(S::sh_batch_fn(s->small_nw, s->small_ln_rl));
            if (int rc = raise_lds_limit(reinterpret_cast<const void*>(fns.back()), g.lds)) return rc;
        }
        if (!d_hs_items) HIPCHK(hipMalloc((void**)&d_hs_items, n * sizeof(SmallHistItem<REAL>)));
        if (!d_hs_stage) HIPCHK(hipMalloc((void**)&d_hs_stage, std::max<uint64_t>(ln_total + 2 * total_b, 1) * sizeof(REAL)));
        HIPCHK(hipMemcpy(d_hs_items, items.data(), n * sizeof(SmallHistItem<REAL>), hipMemcpyHostToDevice));
        hs_fn = std::move(fns);
        hs_bdds = total_b;
        hs_items = std::move(items);
        hs_ord = std::move(ord);
        return BDDMMA_OK;
    }
    int launch_learned_hist(REAL omega, uint32_t n_iters, bool ov, uint32_t hist_from, uint32_t tracked)
    {
        for (size_t k = 0; k < ln_groups.size(); ++k) {
            const LnGroup& g = ln_groups[k];
            hipLaunchKernelGGL(hs_fn[k], dim3(g.count), dim3(g.threads), g.lds, stream, (const SmallHistItem<REAL>*)(d_hs_items + g.first), omega, n_iters, ov ? 1u : 0u,
                               hist_from, tracked);
            HIPCHK(hipGetLastError());
        }
        for (S* s : m) s->small_launched();
        return BDDMMA_OK;
    }
    int learned_iterations(const void* w, const void* omega_vec, double omega, uint64_t num_itr, int on_dev) override
    {
        return learned_iterations_history(w, omega_vec, omega, num_itr, nullptr, nullptr, nullptr, 0, 0.0, on_dev);
    }
    // What every learned call of a batch starts with: the refusals — each before any member is touched; `stop`: the stopping form's admission
    // on top — the preparation on first use, and the one kernel that checks every member's values and moves them into place, with the
    // host's wait for its verdict.  The batch stream is ordered behind the members' on return.
    int learned_begin(const void* w, const void* omega_vec, void* sol_avg, void* lb1_avg, void* lb2_avg, uint64_t cfi, int on_dev, bool stop)
    {
        int rc;
        const uint32_t n = (uint32_t)m.size();
        if (!w) { err = "batch learned_iterations: dist_weights is null"; return BDDMMA_ERR_INVALID_ARGUMENT; }
        if (cfi > 0 && (!sol_avg || !lb1_avg || !lb2_avg)) {
            err = "batch learned_iterations: compute_history_for_itr > 0 needs sol_avg, lb_first_diff_avg and lb_second_diff_avg";
            return BDDMMA_ERR_INVALID_ARGUMENT;
        }
        if ((rc = check_state())) return rc;
        for (uint32_t i = 0; i < n; ++i)
            if (stop && !m[i]->small_stop_ok) {
                err = "batch member " + std::to_string(i) + ": learned iterations with the stopping rule do not fit one workgroup (bddmma_fused_small_stop is 0)";
                return BDDMMA_ERR_UNSUPPORTED;
            } else if (cfi > 0 && !m[i]->small_hist_ok) {
                err = "batch member " + std::to_string(i) + ": learned iterations with their history do not fit one workgroup (bddmma_fused_small_history is 0)";
                return BDDMMA_ERR_UNSUPPORTED;
            } else if (!m[i]->small_ln_ok) {
                err = "batch member " + std::to_string(i) + ": learned iterations do not fit one workgroup's LDS (bddmma_fused_small_learned is 0)";
                return BDDMMA_ERR_UNSUPPORTED;
            }
        HIPCHK(hipSetDevice(device));
        if (!ln_ready) {
            if ((rc = ln_prepare())) return rc;
            ln_ready = true;
        }
        if ((cfi > 0 || stop) && !hs_ready) {
            if ((rc = hs_prepare())) return rc;
            hs_ready = true;
        }
        if (stop && !st_ready) {
            if ((rc = st_prepare())) return rc;
            st_ready = true;
        }
        const bool ov = omega_vec != nullptr;
        // host inputs: checked here, before anything is copied
        if (!on_dev) {
            const void* arr[2] = {w, omega_vec};
            const char* what[2] = {"dist_weights", "omega_vec"};
            for (int a = 0; a < 2; ++a) {
                const REAL* h = (const REAL*)arr[a];
                if (!h) continue;
                for (uint32_t i = 0; i < n; ++i)
                    for (uint64_t l = 0; l < m[i]->n_layers; ++l) {
                        const REAL x = h[ln_src[i] + l];
                        if (!(x >= REAL(0) && x < std::numeric_limits<REAL>::infinity())) {
                            err = "batch member " + std::to_string(i) + ": " + what[a] + "[" + std::to_string(l) + "] is negative or not finite";
                            return BDDMMA_ERR_INVALID_ARGUMENT;
                        }
                    }
            }
        }
        // The batch stream behind everything queued on the members (their earlier learned launches read the buffers written next); then one
        // kernel checks every member's values and moves them into place.  The members' own state is not touched before the check is read.
        for (uint32_t i = 0; i < n; ++i) {
            HIPCHK(hipEventRecord(ev_in[i], m[i]->stream));
            HIPCHK(hipStreamWaitEvent(stream, ev_in[i], 0));
        }
        const REAL *dw = (const REAL*)w, *dov = (const REAL*)omega_vec;
        if (!on_dev) {
            HIPCHK(hipMemcpyAsync(d_ln_in, w, ln_total * sizeof(REAL), hipMemcpyHostToDevice, stream));
            dw = d_ln_in;
            if (ov) {
                HIPCHK(hipMemcpyAsync(d_ln_in + ln_total, omega_vec, ln_total * sizeof(REAL), hipMemcpyHostToDevice, stream));
                dov = d_ln_in + ln_total;
            }
        }
        HIPCHK(hipMemsetAsync(d_ln_bad, 0xFF, 2 * sizeof(uint32_t), stream));
        hipLaunchKernelGGL((k_batch_learn_load<REAL>), dim3(n), dim3(256), 0, stream, (const LearnLoad<REAL>*)d_ln_tab, dw, dov, d_ln_bad);
        HIPCHK(hipGetLastError());
        uint32_t bad[2] = {0xFFFFFFFFu, 0xFFFFFFFFu};
        HIPCHK(hipMemcpyAsync(bad, d_ln_bad, sizeof(bad), hipMemcpyDeviceToHost, stream));
        HIPCHK(hipStreamSynchronize(stream));
        if (bad[0] != 0xFFFFFFFFu || bad[1] != 0xFFFFFFFFu) {
            const bool in_w = bad[0] != 0xFFFFFFFFu;
            err = "batch member " + std::to_string(in_w ? bad[0] : bad[1]) + ": some of its " + (in_w ? "dist_weights" : "omega_vec") + " are negative or not finite";
            (void)join_out();
            return BDDMMA_ERR_INVALID_ARGUMENT;
        }
        return BDDMMA_OK;
    }
    // cfi == 0: the call without a history, launch for launch what it was
    int learned_iterations_history(const void* w, const void* omega_vec, double omega, uint64_t num_itr, void* sol_avg, void* lb1_avg, void* lb2_avg, uint64_t cfi,
                                   double beta_d, int on_dev) override
    {
        int rc;
        const uint32_t n = (uint32_t)m.size();
        if ((rc = learned_begin(w, omega_vec, sol_avg, lb1_avg, lb2_avg, cfi, on_dev, false))) return rc;
        const bool ov = omega_vec != nullptr;
        if (num_itr == 0) return join_out();
        // set_initial_lb_change, once per solver: the bounds before and after the first iteration, enqueued on the member's stream and fetched
        // at the end — so the first iteration is a launch of its own when a member still wants it (n then m learned iterations are n + m)
        std::vector<char> want(n, 0);
        bool any = false;
        for (uint32_t i = 0; i < n; ++i) {
            want[i] = !std::isfinite(m[i]->initial_lb_change);
            any = any || want[i];
            if (want[i] && (rc = m[i]->lower_bound_enqueue(0))) { err = m[i]->err; (void)join_out(); return rc; }
        }
        uint64_t left = num_itr;
        const REAL omega_r = (REAL)omega;
        // The history: the last min(num_itr, cfi) iterations are tracked (bdd_cuda_learned_mma.cu:211).  A launch whose iterations all lie
        // in front of them is the learned launch without a history; any other runs the history form, told which of its iterations is the
        // first tracked one and how many history steps the call has made so far.  Host outputs: their content goes to the device first —
        // an entry the history does not reach keeps it — and comes back behind the last launch.
        const uint64_t untracked = num_itr - std::min(num_itr, cfi);
        const uint64_t hist_values = cfi > 0 ? ln_total + 2 * hs_bdds : 0;
        REAL *o_sol = (REAL*)sol_avg, *o_lb1 = (REAL*)lb1_avg, *o_lb2 = (REAL*)lb2_avg;
        if (cfi > 0) {
            hipError_t e = hipSuccess;
            if (!on_dev) {
                o_sol = d_hs_stage; o_lb1 = d_hs_stage + ln_total; o_lb2 = o_lb1 + hs_bdds;
                e = hipMemcpyAsync(o_sol, sol_avg, ln_total * sizeof(REAL), hipMemcpyHostToDevice, stream);
                if (e == hipSuccess) e = hipMemcpyAsync(o_lb1, lb1_avg, hs_bdds * sizeof(REAL), hipMemcpyHostToDevice, stream);
                if (e == hipSuccess) e = hipMemcpyAsync(o_lb2, lb2_avg, hs_bdds * sizeof(REAL), hipMemcpyHostToDevice, stream);
            }
            if (e == hipSuccess) {   // the call's outputs and beta into the items, in stream order
                hipLaunchKernelGGL((k_hist_items_call<REAL>), dim3(cdiv(n, 256)), dim3(256), 0, stream, d_hs_items, n, o_sol, o_lb1, o_lb2, (REAL)beta_d);
                e = hipGetLastError();
            }
            if (e != hipSuccess) { err = std::string("batch learned_iterations: ") + hipGetErrorString(e); (void)join_out(); return BDDMMA_ERR_DEVICE; }
        }
        // iterations [at, at + count) of the call
        auto launch_range = [&](uint64_t at, uint32_t count) -> int {
            if (at + count <= untracked) return launch_learned(omega_r, count, ov);
            const uint64_t first = std::max(at, untracked);
            return launch_learned_hist(omega_r, count, ov, (uint32_t)(first - at), (uint32_t)std::min<uint64_t>(first - untracked, 0xFFFFFFFFull));
        };
        if (any) {
            if ((rc = join_in())) { (void)join_out(); return rc; }
            rc = launch_range(0, 1);
            const int rc2 = join_out();
            if (rc || rc2) return rc ? rc : rc2;
            for (uint32_t i = 0; i < n; ++i)
                if (want[i] && (rc = m[i]->lower_bound_enqueue(1))) { err = m[i]->err; return rc; }
            --left;
        }
        if (left) {
            if ((rc = join_in())) { (void)join_out(); return rc; }
            while (left) {
                const uint32_t chunk = (uint32_t)std::min<uint64_t>(left, 1u << 14);   // as SolverT::iterations
                if ((rc = launch_range(num_itr - left, chunk))) break;
                left -= chunk;
            }
            const int rc2 = join_out();
            if (rc || rc2) return rc ? rc : rc2;
        }
        if (hist_values && !on_dev) {   // behind the last launch on the batch stream: the one synchronisation of the host outputs
            hipError_t e = hipMemcpyAsync(sol_avg, o_sol, ln_total * sizeof(REAL), hipMemcpyDeviceToHost, stream);
            if (e == hipSuccess) e = hipMemcpyAsync(lb1_avg, o_lb1, hs_bdds * sizeof(REAL), hipMemcpyDeviceToHost, stream);
            if (e == hipSuccess) e = hipMemcpyAsync(lb2_avg, o_lb2, hs_bdds * sizeof(REAL), hipMemcpyDeviceToHost, stream);
            if (e == hipSuccess) e = hipStreamSynchronize(stream);
            if (e != hipSuccess) { err = std::string("batch learned_iterations: ") + hipGetErrorString(e); return BDDMMA_ERR_DEVICE; }
        }
        for (uint32_t i = 0; i < n; ++i)
            if (want[i]) {
                double a = 0.0, b = 0.0;
                if ((rc = m[i]->lower_bound_fetch(0, &a)) || (rc = m[i]->lower_bound_fetch(1, &b))) { err = m[i]->err; return rc; }
                m[i]->initial_lb_change = std::abs(a - b);
            }
        return BDDMMA_OK;
    }

    // ---- ... that stop on the bound's slope (kernels/smallstop.hpp: k_learned_small_stop_batch, k_learned_small_hist_stop_batch; the kernels
    // compile in solver_ss_f32.hip / _f64.hip).  Items in the history items' order, each with the address of its member's stop block
    // (kernels/small.hpp: SmallStopBlock); st_host is the blocks' host copy, in the same order: written before a call's first launch, read
    // back behind its last.
    static constexpr uint32_t STOP_CHUNK = 32;   // iterations per launch: a member that has stopped idles through the rest of its launch's
                                                 // siblings only, and a launch queued behind its stop returns at its first instruction
    using StFn = typename S::SmallStopFn;
    std::vector<StFn> st_fn, st_hist_fn;   // per learned group: without / with the history step
    SmallStopItem<REAL>* d_st_items = nullptr;
    SmallStopBlock* d_st_blocks = nullptr;
    std::vector<SmallStopBlock> st_host;
    bool st_ready = false;

    int st_prepare()
    {
        const uint32_t n = (uint32_t)m.size();
        if (!d_st_items) HIPCHK(hipMalloc((void**)&d_st_items, n * sizeof(SmallStopItem<REAL>)));
        if (!d_st_blocks) HIPCHK(hipMalloc((void**)&d_st_blocks, n * sizeof(SmallStopBlock)));
        std::vector<SmallStopItem<REAL>> items(n);
        for (uint32_t j = 0; j < n; ++j) items[j] = SmallStopItem<REAL>{hs_items[j], d_st_blocks + j};
        std::vector<StFn> fns, hfns;
        for (const LnGroup& g : ln_groups) {
            const S* s = m[hs_ord[g.first]];
            fns.push_back(S::ss_batch_fn(s->small_nw, s->small_ln_rl, false));
            hfns.push_back(S::ss_batch_fn(s->small_nw, s->small_ln_rl, true));
            if (int rc = raise_lds_limit(reinterpret_cast<const void*>(fns.back()), g.lds)) return rc;
            if (int rc = raise_lds_limit(reinterpret_cast<const void*>(hfns.back()), g.lds)) return rc;
        }
        HIPCHK(hipMemcpy(d_st_items, items.data(), n * sizeof(SmallStopItem<REAL>), hipMemcpyHostToDevice));
        st_fn = std::move(fns);
        st_hist_fn = std::move(hfns);
        st_host.assign(n, SmallStopBlock{});
        return BDDMMA_OK;
    }
    // the next n_iters iterations of the call, for the members that have not stopped
    int launch_learned_stop(REAL omega, uint32_t n_iters, bool ov, bool hist)
    {
        for (size_t k = 0; k < ln_groups.size(); ++k) {
            const LnGroup& g = ln_groups[k];
            hipLaunchKernelGGL(hist ? st_hist_fn[k] : st_fn[k], dim3(g.count), dim3(g.threads), g.lds, stream, (const SmallStopItem<REAL>*)(d_st_items + g.first), omega,
                               n_iters, ov ? 1u : 0u);
            HIPCHK(hipGetLastError());
        }
        for (S* s : m) s->small_launched();
        return BDDMMA_OK;
    }
    // The per-member call with improvement_slope > 0 for every member: the rule runs in the member's workgroup behind every iteration, the
    // chunks of STOP_CHUNK iterations are queued without waiting, and the host waits once, for the stop blocks (and any host outputs).
    int learned_iterations_stop(const void* w, const void* omega_vec, double omega, uint64_t num_itr, double slope, void* sol_avg, void* lb1_avg, void* lb2_avg,
                                uint64_t cfi, double beta_d, int on_dev, uint64_t* done) override
    {
        int rc;
        const uint32_t n = (uint32_t)m.size();
        if (!done) { err = "batch learned_iterations: iterations_done is null"; return BDDMMA_ERR_INVALID_ARGUMENT; }
        if (!(slope > 0)) {   // never stops (NaN included): the call with a fixed window
            if ((rc = learned_iterations_history(w, omega_vec, omega, num_itr, sol_avg, lb1_avg, lb2_avg, cfi, beta_d, on_dev))) return rc;
            for (uint32_t i = 0; i < n; ++i) done[i] = num_itr;
            return BDDMMA_OK;
        }
        if ((rc = learned_begin(w, omega_vec, sol_avg, lb1_avg, lb2_avg, cfi, on_dev, true))) return rc;
        const bool ov = omega_vec != nullptr;
        for (uint32_t i = 0; i < n; ++i) done[i] = 0;
        if (num_itr == 0) return join_out();
        const char* const me = "batch learned_iterations: ";
        // the members' costs-to-terminal and the partial sums of their bounds valid, the batch stream behind them; then the blocks of this call
        if ((rc = join_in())) { (void)join_out(); return rc; }
        for (uint32_t j = 0; j < n; ++j) {
            SmallStopBlock b{};
            b.slope = slope;
            b.num_itr = num_itr;
            b.cfi = cfi;
            b.initial_change = m[hs_ord[j]]->initial_lb_change;
            st_host[j] = b;
        }
        hipError_t e = hipMemcpyAsync(d_st_blocks, st_host.data(), n * sizeof(SmallStopBlock), hipMemcpyHostToDevice, stream);
        // The history's outputs as in learned_iterations_history: host content to the device first — an entry the history does not reach
        // keeps it — and back behind the last launch.
        const uint64_t hist_values = cfi > 0 ? ln_total + 2 * hs_bdds : 0;
        REAL *o_sol = (REAL*)sol_avg, *o_lb1 = (REAL*)lb1_avg, *o_lb2 = (REAL*)lb2_avg;
        if (cfi > 0 && e == hipSuccess) {
            if (!on_dev) {
                o_sol = d_hs_stage; o_lb1 = d_hs_stage + ln_total; o_lb2 = o_lb1 + hs_bdds;
                e = hipMemcpyAsync(o_sol, sol_avg, ln_total * sizeof(REAL), hipMemcpyHostToDevice, stream);
                if (e == hipSuccess) e = hipMemcpyAsync(o_lb1, lb1_avg, hs_bdds * sizeof(REAL), hipMemcpyHostToDevice, stream);
                if (e == hipSuccess) e = hipMemcpyAsync(o_lb2, lb2_avg, hs_bdds * sizeof(REAL), hipMemcpyHostToDevice, stream);
            }
            if (e == hipSuccess) {
                hipLaunchKernelGGL((k_stop_items_call<REAL>), dim3(cdiv(n, 256)), dim3(256), 0, stream, d_st_items, n, o_sol, o_lb1, o_lb2, (REAL)beta_d);
                e = hipGetLastError();
            }
        }
        if (e != hipSuccess) { err = std::string(me) + hipGetErrorString(e); (void)join_out(); return BDDMMA_ERR_DEVICE; }
        uint64_t g0 = 0;
        while (g0 < num_itr && !rc) {
            const uint32_t chunk = (uint32_t)std::min<uint64_t>(num_itr - g0, STOP_CHUNK);
            rc = launch_learned_stop((REAL)omega, chunk, ov, cfi > 0);
            g0 += chunk;
        }
        const int rc2 = join_out();   // also behind a failed launch: what was queued stays ordered
        if (rc || rc2) return rc ? rc : rc2;
        // behind the last launch on the batch stream: the one synchronisation, for the stop blocks and any host outputs
        e = hipMemcpyAsync(st_host.data(), d_st_blocks, n * sizeof(SmallStopBlock), hipMemcpyDeviceToHost, stream);
        if (hist_values && !on_dev) {
            if (e == hipSuccess) e = hipMemcpyAsync(sol_avg, o_sol, ln_total * sizeof(REAL), hipMemcpyDeviceToHost, stream);
            if (e == hipSuccess) e = hipMemcpyAsync(lb1_avg, o_lb1, hs_bdds * sizeof(REAL), hipMemcpyDeviceToHost, stream);
            if (e == hipSuccess) e = hipMemcpyAsync(lb2_avg, o_lb2, hs_bdds * sizeof(REAL), hipMemcpyDeviceToHost, stream);
        }
        if (e == hipSuccess) e = hipStreamSynchronize(stream);
        if (e != hipSuccess) { err = std::string(me) + hipGetErrorString(e); return BDDMMA_ERR_DEVICE; }
        for (uint32_t j = 0; j < n; ++j) {
            S* s = m[hs_ord[j]];
            done[hs_ord[j]] = st_host[j].iters;
            if (!std::isfinite(s->initial_lb_change)) s->initial_lb_change = st_host[j].initial_change;   // set_initial_lb_change: once per solver
        }
        return BDDMMA_OK;
    }

    // ---- the backward of the learned iterations (kernels/gradsmall.hpp: k_grad_small_batch; the kernels compile in solver_gs_f32.hip / _f64.hip)
    // One workgroup per member runs the whole call: the tracked iterations once, recording, then their reverse.  The workspace — per member
    // the entry state, the arguments, the reverse's scratch and the records of every tracked iteration — is the batch's: allocated before
    // any member is touched, grown only when a call tracks more iterations than any call before it, freed with the batch.
    using GsFn = typename S::GradSmallFn;
    struct GsGroup {
        GsFn fn;
        typename S::GradSmallUntrackedFn fn_untracked;   // the call with per-member counts (grad_learned_iterations_counts)
        typename S::GradSmallCountsFn fn_counts;
        uint32_t threads, lds, first, count;
    };
    std::vector<GsGroup> gs_groups;
    std::vector<GradSmallItem<REAL>> gs_items;   // host copy, in launch order (member order within a group)
    std::vector<uint64_t> gs_slab_off;           // per item: first value of its slab for gs_n_rec tracked iterations
    GradSmallItem<REAL>* d_gs_items = nullptr;
    REAL *d_gs_ws = nullptr, *d_gs_io = nullptr; // the workspace; host arguments and results on the device: 5 inputs | 5 outputs
    uint32_t* d_gs_bad = nullptr;                // k_grad_small_load's five words
    uint32_t* d_gs_cnt = nullptr;                // the call with per-member counts: tracked[n] | after[n] (member order) | the call's GradSmallIO
    std::vector<uint32_t> gs_cnt;                // ... and what it is copied from
    uint64_t gs_n_rec = 0, gs_total = 0;         // tracked iterations the workspace holds; values of all members' layers
    bool gs_ready = false;

    int gs_prepare()
    {
        const uint32_t n = (uint32_t)m.size();
        if (!ln_ready) {
            if (int rc = ln_prepare()) return rc;
            ln_ready = true;
        }
        for (S* s : m)
            if (int rc = s->sm_prepare()) { err = s->err; return rc; }   // the parent tables of the pull sweeps
        std::vector<uint32_t> ord(n);
        for (uint32_t i = 0; i < n; ++i) ord[i] = i;
        auto key = [&](uint32_t i) { return (uint32_t)m[i]->small_nw * 2u + (m[i]->small_ln_rl ? 1u : 0u); };
        std::stable_sort(ord.begin(), ord.end(), [&](uint32_t a, uint32_t b) { return key(a) < key(b); });
        auto up4 = [](uint64_t x) { return (uint32_t)((x + 3) & ~3ull); };
        std::vector<GsGroup> groups_;
        gs_items.assign(n, GradSmallItem<REAL>{});
        for (uint32_t j = 0; j < n; ++j) {
            const S* s = m[ord[j]];
            GradSmallItem<REAL>& it = gs_items[j];
            it.fw = s->small_learn_item();
            it.par_ptr = s->d_sm_nptr; it.par = s->d_sm_npar;
            it.var = s->d_var; it.var_ptr = s->d_var_ptr; it.var_layers = s->d_var_layers; it.lpos = s->d_lpos;
            it.alpha_ent = s->d_alpha_ent; it.omega_lay = s->d_omega_lay;
            it.ww = s->pack_width;
            it.L = (uint32_t)s->n_layers; it.N = (uint32_t)s->n_slots; it.V = (uint32_t)s->n_vars;
            it.ls = up4(s->n_layers); it.ss = up4(s->n_slots); it.vs = up4(s->n_vars);
            it.src = (uint32_t)ln_src[ord[j]];
            it.member = ord[j];
            if (groups_.empty() || key(ord[j]) != key(ord[groups_.back().first]))
                groups_.push_back(GsGroup{S::gs_batch_fn(s->small_nw, s->small_ln_rl), S::gs_untracked_fn(s->small_nw, s->small_ln_rl),
                                          S::gs_counts_fn(s->small_nw, s->small_ln_rl), 64u * (uint32_t)s->small_nw, 0u, j, 0u});
            GsGroup& g = groups_.back();
            // the forward's LDS, or a wave's arrays of the reverse sweeps per pack, or the 256 doubles of the scalar omega's sum
            const uint32_t rev = (uint32_t)(s->nb_.n_packs * gi_lds_bytes(sizeof(REAL), s->pack_width));
            g.lds = std::max({g.lds, s->small_ln_lds, rev, 2048u});
            ++g.count;
        }
        for (const GsGroup& g : groups_) {
            if (g.lds > m[0]->lds_cu) { err = "batch grad_learned_iterations: the reverse sweeps do not fit the LDS"; return BDDMMA_ERR_UNSUPPORTED; }
            for (const void* fn : {reinterpret_cast<const void*>(g.fn), reinterpret_cast<const void*>(g.fn_untracked), reinterpret_cast<const void*>(g.fn_counts)})
                if (int rc = raise_lds_limit(fn, g.lds)) return rc;
        }
        gs_total = ln_total;
        HIPCHK(hipMalloc((void**)&d_gs_items, n * sizeof(GradSmallItem<REAL>)));
        HIPCHK(hipMalloc((void**)&d_gs_io, (10 * gs_total + n) * sizeof(REAL)));
        HIPCHK(hipMalloc((void**)&d_gs_bad, 5 * sizeof(uint32_t)));
        static_assert(sizeof(GradSmallIO<REAL>) % sizeof(uint32_t) == 0 && alignof(GradSmallIO<REAL>) <= 8, "io sits behind 2 n words: 8-byte aligned");
        gs_cnt.assign(2 * n + sizeof(GradSmallIO<REAL>) / sizeof(uint32_t), 0u);
        HIPCHK(hipMalloc((void**)&d_gs_cnt, gs_cnt.size() * sizeof(uint32_t)));
        gs_groups = std::move(groups_);
        return BDDMMA_OK;
    }
    // the workspace for n_rec tracked iterations and the items that point into it
    int gs_workspace(uint64_t n_rec)
    {
        if (d_gs_ws && n_rec <= gs_n_rec) return BDDMMA_OK;
        uint64_t total = 0;
        gs_slab_off.assign(gs_items.size(), 0);
        for (size_t j = 0; j < gs_items.size(); ++j) {
            gs_slab_off[j] = total;
            total += gs_slab_values(gs_items[j].ls, gs_items[j].ss, gs_items[j].vs, n_rec);
        }
        REAL* ws = nullptr;
        if (hipMalloc((void**)&ws, total * sizeof(REAL)) != hipSuccess) {
            (void)hipGetLastError();
            err = "batch grad_learned_iterations: no memory for the records of " + std::to_string(n_rec) + " tracked iterations";
            return BDDMMA_ERR_DEVICE;
        }
        HIPCHK(hipStreamSynchronize(stream));   // nothing in flight reads the old workspace or items
        if (d_gs_ws) (void)hipFree(d_gs_ws);
        d_gs_ws = ws;
        gs_n_rec = n_rec;
        for (size_t j = 0; j < gs_items.size(); ++j) gs_items[j].ws = d_gs_ws + gs_slab_off[j];
        HIPCHK(hipMemcpy(d_gs_items, gs_items.data(), gs_items.size() * sizeof(GradSmallItem<REAL>), hipMemcpyHostToDevice));
        return BDDMMA_OK;
    }
    // What both backward calls of a batch start with: the refusals, each before any member or output is touched; the preparation on first
    // use and the workspace for the call's largest tracked count; the arrays of the call (`io`; host arrays through the staging buffer); and
    // the one kernel that checks every array, moves the arguments into place and saves every member's entry state, with the host's wait
    // for its verdict.  after / tracked: the per-member counts (both null: `n_track` tracked iterations for every member), on the device
    // in d_gs_cnt — one copy with the call's io, in front of the check launch — when this returns; n_max: the largest tracked count.
    int grad_begin(const char* me, const void* w, const void* omega_vec, double omega, void* grad_lo, void* grad_hi, void* grad_mm, void* grad_w_out,
                   void* grad_omega_out, uint64_t n_track, const uint64_t* after, const uint64_t* tracked, bool counts, int on_dev, GradSmallIO<REAL>& io,
                   uint64_t& n_max)
    {
        int rc;
        const uint32_t n = (uint32_t)m.size();
        if (!w || !grad_lo || !grad_hi || !grad_mm || !grad_w_out || !grad_omega_out) { err = std::string(me) + ": null pointer"; return BDDMMA_ERR_INVALID_ARGUMENT; }
        if (counts && (!after || !tracked)) { err = "batch grad_learned_iterations_counts: null count array"; return BDDMMA_ERR_INVALID_ARGUMENT; }
        if ((rc = check_state())) return rc;
        for (uint32_t i = 0; i < n; ++i)
            if (!m[i]->small_ln_ok) {
                err = "batch member " + std::to_string(i) + ": learned iterations do not fit one workgroup's LDS (bddmma_fused_small_learned is 0)";
                return BDDMMA_ERR_UNSUPPORTED;
            }
        const bool ov = omega_vec != nullptr;
        if (!ov && !(omega >= 0.0 && omega < std::numeric_limits<double>::infinity())) { err = std::string(me) + ": omega is negative or not finite"; return BDDMMA_ERR_INVALID_ARGUMENT; }
        n_max = n_track;
        if (counts) {
            n_max = 0;
            for (uint32_t i = 0; i < n; ++i) {
                if (tracked[i] > 0xFFFFFFFFull) { err = "batch member " + std::to_string(i) + ": too many tracked iterations"; return BDDMMA_ERR_INVALID_ARGUMENT; }
                n_max = std::max(n_max, tracked[i]);
            }
            for (uint32_t i = 0; i < n; ++i)   // (a member that tracks nothing runs nothing: its untracked count is not looked at)
                if (tracked[i] > 0 && after[i] > 0xFFFFFFFFull) { err = "batch member " + std::to_string(i) + ": too many untracked iterations"; return BDDMMA_ERR_INVALID_ARGUMENT; }
        } else if (n_track > 0xFFFFFFFFull) {
            err = std::string(me) + ": too many tracked iterations";
            return BDDMMA_ERR_INVALID_ARGUMENT;
        }
        HIPCHK(hipSetDevice(device));
        if (!gs_ready) {
            if ((rc = gs_prepare())) return rc;
            gs_ready = true;
        }
        if ((rc = gs_workspace(n_max))) return rc;
        // The batch stream behind everything queued on the members; then one kernel checks every array, moves the arguments into place and
        // saves every member's entry state.  No member's state is written before the check has been read.
        for (uint32_t i = 0; i < n; ++i) {
            HIPCHK(hipEventRecord(ev_in[i], m[i]->stream));
            HIPCHK(hipStreamWaitEvent(stream, ev_in[i], 0));
        }
        io = GradSmallIO<REAL>{};
        if (on_dev) {
            io.w = (const REAL*)w; io.ov = (const REAL*)omega_vec;
            io.in_lo = (const REAL*)grad_lo; io.in_hi = (const REAL*)grad_hi; io.in_mm = (const REAL*)grad_mm;
            io.lo = (REAL*)grad_lo; io.hi = (REAL*)grad_hi; io.mm = (REAL*)grad_mm; io.gw = (REAL*)grad_w_out; io.gom = (REAL*)grad_omega_out;
        } else {
            const void* src[5] = {w, omega_vec, grad_lo, grad_hi, grad_mm};
            REAL* dst[5];
            for (int k = 0; k < 5; ++k) {
                dst[k] = d_gs_io + (uint64_t)k * gs_total;
                if (src[k]) HIPCHK(hipMemcpyAsync(dst[k], src[k], gs_total * sizeof(REAL), hipMemcpyHostToDevice, stream));
            }
            io.w = dst[0]; io.ov = ov ? dst[1] : nullptr; io.in_lo = dst[2]; io.in_hi = dst[3]; io.in_mm = dst[4];
            REAL* const o = d_gs_io + 5 * gs_total;
            io.lo = o; io.hi = o + gs_total; io.mm = o + 2 * gs_total; io.gw = o + 3 * gs_total; io.gom = o + 4 * gs_total;
        }
        if (counts) {   // tracked[n] | after[n] | io, which k_grad_small_counts_batch reads from memory (kernels/gradsmall.hpp)
            for (uint32_t i = 0; i < n; ++i) {
                gs_cnt[i] = (uint32_t)tracked[i];
                gs_cnt[n + i] = tracked[i] > 0 ? (uint32_t)after[i] : 0u;
            }
            std::memcpy(gs_cnt.data() + 2 * n, &io, sizeof(io));
            HIPCHK(hipMemcpyAsync(d_gs_cnt, gs_cnt.data(), gs_cnt.size() * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
        }
        HIPCHK(hipMemsetAsync(d_gs_bad, 0xFF, 5 * sizeof(uint32_t), stream));
        hipLaunchKernelGGL(S::gs_load_fn(), dim3(n), dim3(256), 0, stream, (const GradSmallItem<REAL>*)d_gs_items, io, d_gs_bad);
        HIPCHK(hipGetLastError());
        uint32_t bad[5];
        HIPCHK(hipMemcpyAsync(bad, d_gs_bad, sizeof(bad), hipMemcpyDeviceToHost, stream));
        HIPCHK(hipStreamSynchronize(stream));
        {
            // the per-member call's order: the first member with an offending value, and of its arrays the first the call would have checked
            static const char* const what[5] = {"omega_vec", "dist_weights", "grad_lo", "grad_hi", "grad_mm"};
            const uint32_t first = *std::min_element(bad, bad + 5);
            if (first != 0xFFFFFFFFu) {
                int k = 0;
                while (bad[k] != first) ++k;
                err = "batch member " + std::to_string(first) + ": some of its " + what[k] + (k < 2 ? " are negative or not finite" : " are not finite");
                (void)join_out();
                return BDDMMA_ERR_INVALID_ARGUMENT;
            }
        }
        if (n_max == 0) {   // the in-out arrays stay as they are, both outputs are zero
            const uint64_t n_omega = ov ? gs_total : n;
            if (on_dev) {
                HIPCHK(hipMemsetAsync(grad_w_out, 0, gs_total * sizeof(REAL), stream));
                HIPCHK(hipMemsetAsync(grad_omega_out, 0, n_omega * sizeof(REAL), stream));
            } else {
                std::memset(grad_w_out, 0, gs_total * sizeof(REAL));
                std::memset(grad_omega_out, 0, n_omega * sizeof(REAL));
            }
            return join_out();
        }
        return BDDMMA_OK;
    }
    // ... and end with: the results to host arrays, the members' streams behind the batch's
    int grad_end(const char* me, int rc, bool ov, void* grad_lo, void* grad_hi, void* grad_mm, void* grad_w_out, void* grad_omega_out, int on_dev)
    {
        if (!rc && !on_dev) {
            const uint64_t n_omega = ov ? gs_total : m.size();
            const REAL* const o = d_gs_io + 5 * gs_total;
            void* dst[5] = {grad_lo, grad_hi, grad_mm, grad_w_out, grad_omega_out};
            for (int k = 0; k < 5 && !rc; ++k)
                if (hipMemcpyAsync(dst[k], o + (uint64_t)k * gs_total, (k == 4 ? n_omega : gs_total) * sizeof(REAL), hipMemcpyDeviceToHost, stream) != hipSuccess) rc = BDDMMA_ERR_DEVICE;
            if (!rc && hipStreamSynchronize(stream) != hipSuccess) rc = BDDMMA_ERR_DEVICE;
            if (rc) err = std::string(me) + ": copying the results failed";
        }
        const int rc2 = join_out();
        return rc ? rc : rc2;
    }
    int grad_learned_iterations(const void* w, const void* omega_vec, double omega, void* grad_lo, void* grad_hi, void* grad_mm, void* grad_w_out,
                                void* grad_omega_out, uint64_t after, uint64_t n_track, uint64_t num_caches, int on_dev) override
    {
        (void)num_caches;   // every tracked iteration is recorded: nothing is replayed, and the result does not depend on it
        int rc;
        const char* const me = "batch grad_learned_iterations";
        const uint32_t n = (uint32_t)m.size();
        const bool ov = omega_vec != nullptr;
        GradSmallIO<REAL> io{};
        uint64_t n_max = 0;
        if ((rc = grad_begin(me, w, omega_vec, omega, grad_lo, grad_hi, grad_mm, grad_w_out, grad_omega_out, n_track, nullptr, nullptr, false, on_dev, io, n_max))) return rc;
        if (n_track == 0) return BDDMMA_OK;
        // ---- the members are touched from here on
        std::vector<char> dvar_valid(n);
        for (uint32_t i = 0; i < n; ++i) dvar_valid[i] = m[i]->delta_var_valid;
        if ((rc = join_in())) { (void)join_out(); return rc; }
        const REAL omega_r = (REAL)omega;
        uint64_t left = after;
        while (left && !rc) {   // the untracked iterations: the fused learned launches
            const uint32_t chunk = (uint32_t)std::min<uint64_t>(left, GS_CHUNK);
            rc = launch_learned(omega_r, chunk, ov);
            left -= chunk;
        }
        if (!rc)
            for (const GsGroup& g : gs_groups) {
                hipLaunchKernelGGL(g.fn, dim3(g.count), dim3(g.threads), g.lds, stream, (const GradSmallItem<REAL>*)(d_gs_items + g.first), omega_r, (uint32_t)n_track,
                                   ov ? 1u : 0u, io);
                if (hipGetLastError() != hipSuccess) { err = std::string(me) + ": launch failed"; rc = BDDMMA_ERR_DEVICE; break; }
            }
        // the state contract of the per-member call: the entry values are back (the kernel's last phase), both sweep states are invalid
        for (uint32_t i = 0; i < n; ++i) {
            m[i]->small_launched();
            m[i]->costs_changed();
            m[i]->delta_var_valid = dvar_valid[i];
        }
        return grad_end(me, rc, ov, grad_lo, grad_hi, grad_mm, grad_w_out, grad_omega_out, on_dev);
    }
    // Every member with its own two counts (kernels/gradsmall.hpp: k_grad_small_untracked_batch, k_grad_small_counts_batch).  A member whose
    // tracked count is 0 is not touched: no sweep, no iteration, no bookkeeping — its workgroups pass the in-out arrays through and zero
    // its outputs.  The host waits where grad_learned_iterations waits.
    int grad_learned_iterations_counts(const void* w, const void* omega_vec, double omega, void* grad_lo, void* grad_hi, void* grad_mm, void* grad_w_out,
                                       void* grad_omega_out, const uint64_t* after, const uint64_t* tracked, uint64_t num_caches, int on_dev) override
    {
        (void)num_caches;
        int rc;
        const char* const me = "batch grad_learned_iterations";   // (the shared refusals keep their messages)
        const uint32_t n = (uint32_t)m.size();
        const bool ov = omega_vec != nullptr;
        GradSmallIO<REAL> io{};
        uint64_t n_max = 0;
        if ((rc = grad_begin(me, w, omega_vec, omega, grad_lo, grad_hi, grad_mm, grad_w_out, grad_omega_out, 0, after, tracked, true, on_dev, io, n_max))) return rc;
        if (n_max == 0) return BDDMMA_OK;
        // ---- the members with a tracked count are touched from here on (join_in's sweeps for them alone)
        std::vector<char> dvar_valid(n), idle(n);
        uint32_t after_max = 0;
        for (uint32_t i = 0; i < n; ++i) {
            dvar_valid[i] = m[i]->delta_var_valid;
            idle[i] = gs_cnt[i] == 0;
            after_max = std::max(after_max, gs_cnt[n + i]);
        }
        run_mask = idle.data();
        rc = join_in();
        run_mask = nullptr;
        if (rc) { (void)join_out(); return rc; }
        const REAL omega_r = (REAL)omega;
        for (uint64_t first = 0; first < after_max && !rc; first += GS_CHUNK)
            for (const GsGroup& g : gs_groups) {
                hipLaunchKernelGGL(g.fn_untracked, dim3(g.count), dim3(g.threads), g.lds, stream, (const GradSmallItem<REAL>*)(d_gs_items + g.first), omega_r,
                                   ov ? 1u : 0u, (uint32_t)first, GS_CHUNK, (const uint32_t*)(d_gs_cnt + n));
                if (hipGetLastError() != hipSuccess) { err = std::string(me) + ": launch failed"; rc = BDDMMA_ERR_DEVICE; break; }
            }
        if (!rc)
            for (const GsGroup& g : gs_groups) {
                hipLaunchKernelGGL(g.fn_counts, dim3(g.count), dim3(g.threads), g.lds, stream, (const GradSmallItem<REAL>*)(d_gs_items + g.first), omega_r, ov ? 1u : 0u,
                                   reinterpret_cast<const GradSmallIO<REAL>*>(d_gs_cnt + 2 * n), (const uint32_t*)d_gs_cnt);
                if (hipGetLastError() != hipSuccess) { err = std::string(me) + ": launch failed"; rc = BDDMMA_ERR_DEVICE; break; }
            }
        for (uint32_t i = 0; i < n; ++i)
            if (!idle[i]) {
                m[i]->small_launched();
                m[i]->costs_changed();
                m[i]->delta_var_valid = dvar_valid[i];
            }
        return grad_end(me, rc, ov, grad_lo, grad_hi, grad_mm, grad_w_out, grad_omega_out, on_dev);
    }
    static constexpr uint32_t GS_CHUNK = 1u << 14;   // untracked iterations per launch

    // ---- the members' solver costs, all at once (kernels/batchcosts.hpp: k_small_set_batch, k_small_get_batch; the kernels compile in
    // solver_bc_f32.hip / _f64.hip).  The set kernel is grouped by the members' wave count, as the iteration kernels are; bc_items[j].src is
    // the first value of that member in the concatenated arrays, which are in the caller's order.  Host arrays pass through one staging
    // buffer the batch owns (lo | hi | mm, bc_total values each), allocated before any member is touched and freed with the batch.
    struct BcGroup {
        CostsSetFn<REAL> fn;
        uint32_t threads, lds, first, count;
    };
    std::vector<BcGroup> bc_groups;
    std::vector<uint32_t> bc_order;            // item j of d_bc_items is member bc_order[j]
    CostsItem<REAL>* d_bc_items = nullptr;
    REAL* d_bc_stage = nullptr;
    uint64_t bc_total = 0, bc_stage_cap = 0;   // values of all members' layers; values the staging buffer holds
    bool bc_ready = false;
    hipEvent_t ev_order = nullptr;             // stream_wait / stream_signal: timing disabled, created on first use

    int bc_prepare(bool host_arrays)
    {
        const uint32_t n = (uint32_t)m.size();
        if (!bc_ready) {
            std::vector<uint32_t> ord(n);
            for (uint32_t i = 0; i < n; ++i) ord[i] = i;
            std::stable_sort(ord.begin(), ord.end(), [&](uint32_t a, uint32_t b) { return m[a]->small_nw < m[b]->small_nw; });
            std::vector<uint64_t> src(n);
            uint64_t total = 0;
            for (uint32_t i = 0; i < n; ++i) {
                src[i] = total;
                total += m[i]->n_layers;
            }
            if (total > 0xFFFFFFFFull) { err = "batch solver costs: too many layers"; return BDDMMA_ERR_UNSUPPORTED; }
            std::vector<CostsItem<REAL>> items(n);
            std::vector<BcGroup> groups_;
            for (uint32_t j = 0; j < n; ++j) {
                const S* s = m[ord[j]];
                const SmallDev& sm = s->small;
                items[j] = CostsItem<REAL>{sm.pack_hdr, sm.rec, sm.rec_off, s->d_lpos, s->d_T, s->d_lohi, s->d_mm_binned, s->d_lb_partial,
                                           sm.rec_words, sm.ns, sm.nl, sm.n_packs, 0u, (uint32_t)s->n_layers, (uint32_t)src[ord[j]]};
                if (groups_.empty() || s->small_nw != m[ord[groups_.back().first]]->small_nw)
                    groups_.push_back(BcGroup{costs_set_fn<REAL>(s->small_nw), 64u * (uint32_t)s->small_nw, 0u, j, 0u});
                BcGroup& g = groups_.back();
                g.lds = std::max(g.lds, sm.n_packs * costs_region_bytes((uint32_t)sizeof(REAL), sm.ns, sm.nl));
                ++g.count;
            }
            for (const BcGroup& g : groups_) {
                if (g.lds > m[0]->lds_cu) { err = "batch set_solver_costs: the costs-to-terminal do not fit the LDS"; return BDDMMA_ERR_UNSUPPORTED; }
                if (int rc = raise_lds_limit(reinterpret_cast<const void*>(g.fn), g.lds)) return rc;
            }
            if (!d_bc_items) HIPCHK(hipMalloc((void**)&d_bc_items, n * sizeof(CostsItem<REAL>)));
            HIPCHK(hipMemcpy(d_bc_items, items.data(), n * sizeof(CostsItem<REAL>), hipMemcpyHostToDevice));
            bc_groups = std::move(groups_);
            bc_order = std::move(ord);
            bc_total = total;
            bc_ready = true;
        }
        if (host_arrays && bc_stage_cap < 3 * bc_total) {
            REAL* st = nullptr;
            HIPCHK(hipMalloc((void**)&st, std::max<uint64_t>(3 * bc_total, 1) * sizeof(REAL)));
            if (d_bc_stage) {
                (void)hipStreamSynchronize(stream);   // nothing in flight reads the old buffer
                (void)hipFree(d_bc_stage);
            }
            d_bc_stage = st;
            bc_stage_cap = 3 * bc_total;
        }
        return BDDMMA_OK;
    }
    // the batch stream behind everything queued on every member's stream (join_in without the members' backward sweeps)
    int members_in()
    {
        for (size_t i = 0; i < m.size(); ++i) {
            HIPCHK(hipEventRecord(ev_in[i], m[i]->stream));
            HIPCHK(hipStreamWaitEvent(stream, ev_in[i], 0));
        }
        return BDDMMA_OK;
    }
    int set_solver_costs(const void* lo, const void* hi, const void* mm, int on_dev) override
    {
        int rc;
        if ((rc = check_state())) return rc;
        if (!lo && !hi && !mm) return BDDMMA_OK;
        HIPCHK(hipSetDevice(device));
        if ((rc = bc_prepare(!on_dev))) return rc;
        if ((rc = members_in())) return rc;
        // ---- the members are touched from here on
        const REAL* a[3] = {(const REAL*)lo, (const REAL*)hi, (const REAL*)mm};
        hipError_t e = hipSuccess;
        if (!on_dev)
            for (int k = 0; k < 3 && e == hipSuccess; ++k)
                if (a[k]) {
                    REAL* const st = d_bc_stage + (uint64_t)k * bc_total;
                    e = hipMemcpyAsync(st, a[k], bc_total * sizeof(REAL), hipMemcpyHostToDevice, stream);
                    a[k] = st;
                }
        for (size_t g = 0; g < bc_groups.size() && e == hipSuccess; ++g) {
            const BcGroup& G = bc_groups[g];
            hipLaunchKernelGGL(G.fn, dim3(G.count), dim3(G.threads), G.lds, stream, (const CostsItem<REAL>*)(d_bc_items + G.first), a[0], a[1], a[2]);
            e = hipGetLastError();
        }
        if (e == hipSuccess && !on_dev) e = hipStreamSynchronize(stream);   // the caller may reuse its arrays on return
        // the host-side state after set_solver_costs and backward_run: the costs-to-terminal are those of the new costs, the cached bound
        // is stale; delta_var_valid stays.  Behind a failure nothing is known to be valid.
        for (S* s : m) {
            s->costs_changed();
            s->lb_cached = false;
            ++s->lb_gen;
            s->bwd_valid = s->lb_valid = e == hipSuccess;
        }
        const int rc2 = join_out();
        if (e != hipSuccess) { err = std::string("batch set_solver_costs: ") + hipGetErrorString(e); return BDDMMA_ERR_DEVICE; }
        return rc2;
    }
    int get_solver_costs(void* lo, void* hi, void* mm, int on_dev) override
    {
        int rc;
        if ((rc = check_state())) return rc;
        if (!lo && !hi && !mm) return BDDMMA_OK;
        HIPCHK(hipSetDevice(device));
        if ((rc = bc_prepare(!on_dev))) return rc;
        if ((rc = members_in())) return rc;
        void* const out[3] = {lo, hi, mm};
        REAL* o[3];
        for (int k = 0; k < 3; ++k) o[k] = !out[k] ? nullptr : on_dev ? (REAL*)out[k] : d_bc_stage + (uint64_t)k * bc_total;
        hipLaunchKernelGGL(costs_get_fn<REAL>(), dim3((uint32_t)m.size()), dim3(256), 0, stream, (const CostsItem<REAL>*)d_bc_items, o[0], o[1], o[2]);
        hipError_t e = hipGetLastError();
        if (!on_dev) {
            for (int k = 0; k < 3 && e == hipSuccess; ++k)
                if (out[k]) e = hipMemcpyAsync(out[k], o[k], bc_total * sizeof(REAL), hipMemcpyDeviceToHost, stream);
            if (e == hipSuccess) e = hipStreamSynchronize(stream);
        }
        const int rc2 = join_out();
        if (e != hipSuccess) { err = std::string("batch get_solver_costs: ") + hipGetErrorString(e); return BDDMMA_ERR_DEVICE; }
        return rc2;
    }
    // ---- the tail of the loss, all members at once (kernels/batchbound.hpp: k_small_bounds_batch, k_small_grad_lb_batch,
    // k_small_distribute_batch; the kernels compile in solver_bb_f32.hip / _f64.hip).  Items sorted by the members' wave count, as the cost
    // items are: the gradient kernel is one launch per wave count present, the other two one launch for all.  Host arrays pass through one
    // staging buffer the batch owns (per-BDD values | lo | hi); it, the check word and a member's d_mm_consumed are allocated before any
    // member is touched.
    struct BbGroup {
        BoundGradFn<REAL> fn;
        uint32_t threads, lds, first, count;
    };
    std::vector<BbGroup> bb_groups;
    std::vector<BoundItem<REAL>> bb_items;     // host copy, in launch order
    std::vector<uint32_t> bb_ord;              // item j is member bb_ord[j]
    BoundItem<REAL>* d_bb_items = nullptr;
    REAL* d_bb_stage = nullptr;
    uint32_t* d_bb_bad = nullptr;
    uint64_t bb_layers = 0, bb_bdds = 0;       // values of all members' layers / BDDs
    bool bb_ready = false, bb_dist_ready = false;

    // dist: the call is distribute_delta, whose items need every member's d_mm_consumed; host_arrays: the call needs the staging buffer
    int bb_prepare(bool dist, bool host_arrays)
    {
        const uint32_t n = (uint32_t)m.size();
        if (!bb_ready) {
            std::vector<uint32_t> ord(n);
            for (uint32_t i = 0; i < n; ++i) ord[i] = i;
            std::stable_sort(ord.begin(), ord.end(), [&](uint32_t a, uint32_t b) { return m[a]->small_nw < m[b]->small_nw; });
            std::vector<uint64_t> src(n), src_b(n);
            uint64_t total = 0, total_b = 0;
            for (uint32_t i = 0; i < n; ++i) {
                src[i] = total;
                src_b[i] = total_b;
                total += m[i]->n_layers;
                total_b += m[i]->n_bdds;
            }
            if (total > 0xFFFFFFFFull || total_b > 0xFFFFFFFFull) { err = "batch bounds: too many layers"; return BDDMMA_ERR_UNSUPPORTED; }
            std::vector<BoundItem<REAL>> items(n);
            std::vector<BbGroup> groups_;
            for (uint32_t j = 0; j < n; ++j) {
                const S* s = m[ord[j]];
                const SmallDev& sm = s->small;
                items[j] = BoundItem<REAL>{sm.pack_hdr, sm.rec, sm.rec_off, s->d_lpos, s->d_root_slot, s->d_bdd, s->d_T, s->d_lohi, s->d_mm_binned, s->d_mm_consumed,
                                           s->d_delta_var, s->d_delta_lay, sm.rec_words, sm.ns, sm.nl, sm.n_packs, (uint32_t)s->n_layers, (uint32_t)s->n_bdds,
                                           (uint32_t)s->n_vars, (uint32_t)src[ord[j]], (uint32_t)src_b[ord[j]], ord[j]};
                if (groups_.empty() || s->small_nw != m[ord[groups_.back().first]]->small_nw)
                    groups_.push_back(BbGroup{bound_grad_fn<REAL>(s->small_nw), 64u * (uint32_t)s->small_nw, 0u, j, 0u});
                BbGroup& g = groups_.back();
                g.lds = std::max(g.lds, sm.n_packs * bound_region_bytes((uint32_t)sizeof(REAL), sm.ns, sm.nl));
                ++g.count;
            }
            for (const BbGroup& g : groups_) {
                if (g.lds > m[0]->lds_cu) { err = "batch grad_lower_bound_per_bdd: the packs' state does not fit the LDS"; return BDDMMA_ERR_UNSUPPORTED; }
                if (int rc = raise_lds_limit(reinterpret_cast<const void*>(g.fn), g.lds)) return rc;
            }
            if (!d_bb_items) HIPCHK(hipMalloc((void**)&d_bb_items, n * sizeof(BoundItem<REAL>)));
            if (!d_bb_bad) HIPCHK(hipMalloc((void**)&d_bb_bad, sizeof(uint32_t)));
            HIPCHK(hipMemcpy(d_bb_items, items.data(), n * sizeof(BoundItem<REAL>), hipMemcpyHostToDevice));
            bb_items = std::move(items);
            bb_ord = std::move(ord);
            bb_groups = std::move(groups_);
            bb_layers = total;
            bb_bdds = total_b;
            bb_ready = true;
        }
        if (dist && !bb_dist_ready) {
            for (S* s : m)
                if (!s->d_mm_consumed)
                    if (int rc = s->dalloc(&s->d_mm_consumed, s->n_layers)) { err = s->err; return rc; }
            for (uint32_t j = 0; j < n; ++j) bb_items[j].mm_consumed = m[bb_ord[j]]->d_mm_consumed;
            HIPCHK(hipStreamSynchronize(stream));   // nothing in flight reads the items
            HIPCHK(hipMemcpy(d_bb_items, bb_items.data(), n * sizeof(BoundItem<REAL>), hipMemcpyHostToDevice));
            bb_dist_ready = true;
        }
        if (host_arrays && !d_bb_stage) HIPCHK(hipMalloc((void**)&d_bb_stage, std::max<uint64_t>(bb_bdds + 2 * bb_layers, 1) * sizeof(REAL)));
        return BDDMMA_OK;
    }
    int lower_bound_per_bdd(void* out, int on_dev) override
    {
        int rc;
        if (!out) { err = "batch lower_bound_per_bdd: null output pointer"; return BDDMMA_ERR_INVALID_ARGUMENT; }
        if ((rc = check_state())) return rc;
        HIPCHK(hipSetDevice(device));
        if ((rc = bb_prepare(false, !on_dev))) return rc;
        if ((rc = join_in())) { (void)join_out(); return rc; }
        REAL* const o = on_dev ? (REAL*)out : d_bb_stage;
        hipLaunchKernelGGL(bound_get_fn<REAL>(), dim3((uint32_t)m.size()), dim3(256), 0, stream, (const BoundItem<REAL>*)d_bb_items, o);
        hipError_t e = hipGetLastError();
        if (!on_dev) {
            if (e == hipSuccess) e = hipMemcpyAsync(out, o, bb_bdds * sizeof(REAL), hipMemcpyDeviceToHost, stream);
            if (e == hipSuccess) e = hipStreamSynchronize(stream);
        }
        const int rc2 = join_out();
        if (e != hipSuccess) { err = std::string("batch lower_bound_per_bdd: ") + hipGetErrorString(e); return BDDMMA_ERR_DEVICE; }
        return rc2;
    }
    int grad_lower_bound_per_bdd(const void* grad_lb, void* grad_lo, void* grad_hi, int on_dev) override
    {
        int rc;
        const char* const me = "batch grad_lower_bound_per_bdd";
        const uint32_t n = (uint32_t)m.size();
        if (!grad_lb || !grad_lo || !grad_hi) { err = std::string(me) + ": null pointer"; return BDDMMA_ERR_INVALID_ARGUMENT; }
        if ((rc = check_state())) return rc;
        HIPCHK(hipSetDevice(device));
        if ((rc = bb_prepare(false, !on_dev))) return rc;
        // the argument check, before any member or output is touched: host values here, device values by one launch for all members
        // (the batch stream is behind whatever the caller ordered it behind: bddmma_stream_wait_batch) and the call's one read
        uint32_t bad = 0xFFFFFFFFu;
        if (!on_dev) {
            const REAL* h = (const REAL*)grad_lb;
            for (uint32_t i = 0; i < n && bad == 0xFFFFFFFFu; ++i) {
                for (uint64_t b = 0; b < m[i]->n_bdds; ++b)
                    if (!std::isfinite(h[b])) { bad = i; break; }
                h += m[i]->n_bdds;
            }
        } else {
            HIPCHK(hipMemsetAsync(d_bb_bad, 0xFF, sizeof(uint32_t), stream));
            hipLaunchKernelGGL(bound_check_fn<REAL>(), dim3(n), dim3(256), 0, stream, (const BoundItem<REAL>*)d_bb_items, (const REAL*)grad_lb, d_bb_bad);
            HIPCHK(hipGetLastError());
            HIPCHK(hipMemcpyAsync(&bad, d_bb_bad, sizeof(bad), hipMemcpyDeviceToHost, stream));
            HIPCHK(hipStreamSynchronize(stream));
        }
        if (bad != 0xFFFFFFFFu) {
            err = "batch member " + std::to_string(bad) + ": some of its grad_lb_per_bdd are not finite";
            return BDDMMA_ERR_INVALID_ARGUMENT;
        }
        if ((rc = join_in())) { (void)join_out(); return rc; }
        const REAL* g = (const REAL*)grad_lb;
        REAL *lo = (REAL*)grad_lo, *hi = (REAL*)grad_hi;
        hipError_t e = hipSuccess;
        if (!on_dev) {
            e = hipMemcpyAsync(d_bb_stage, grad_lb, bb_bdds * sizeof(REAL), hipMemcpyHostToDevice, stream);
            g = d_bb_stage;
            lo = d_bb_stage + bb_bdds;
            hi = lo + bb_layers;
        }
        for (size_t k = 0; k < bb_groups.size() && e == hipSuccess; ++k) {
            const BbGroup& G = bb_groups[k];
            hipLaunchKernelGGL(G.fn, dim3(G.count), dim3(G.threads), G.lds, stream, (const BoundItem<REAL>*)(d_bb_items + G.first), g, lo, hi);
            e = hipGetLastError();
        }
        if (!on_dev) {
            if (e == hipSuccess) e = hipMemcpyAsync(grad_lo, lo, bb_layers * sizeof(REAL), hipMemcpyDeviceToHost, stream);
            if (e == hipSuccess) e = hipMemcpyAsync(grad_hi, hi, bb_layers * sizeof(REAL), hipMemcpyDeviceToHost, stream);
            if (e == hipSuccess) e = hipStreamSynchronize(stream);
        }
        const int rc2 = join_out();
        if (e != hipSuccess) { err = std::string(me) + ": " + hipGetErrorString(e); return BDDMMA_ERR_DEVICE; }
        return rc2;
    }
    int distribute_delta() override
    {
        int rc;
        if ((rc = check_state())) return rc;
        HIPCHK(hipSetDevice(device));
        if ((rc = bb_prepare(true, false))) return rc;
        if ((rc = members_in())) return rc;
        // ---- the members are touched from here on
        hipLaunchKernelGGL(bound_dist_fn<REAL>(), dim3((uint32_t)m.size()), dim3(256), 0, stream, (const BoundItem<REAL>*)d_bb_items);
        const hipError_t e = hipGetLastError();
        // the host-side state after SolverT::distribute_delta
        for (S* s : m) {
            s->mm_consumed_valid = true;
            s->x_layer_valid = false;
            s->delta_var_valid = true;
            s->costs_changed();
        }
        const int rc2 = join_out();
        if (e != hipSuccess) { err = std::string("batch distribute_delta: ") + hipGetErrorString(e); return BDDMMA_ERR_DEVICE; }
        return rc2;
    }
    // ---- the min-marginal differences and their gradient, all members at once (kernels/batchmm.hpp: k_small_mmdiff_batch,
    // k_small_grad_mm_batch; the kernels compile in solver_bm_f32.hip / _f64.hip).  Items sorted by the members' wave count, as the bound
    // items are: one launch per wave count present.  Host arrays pass through one staging buffer the batch owns (grad_mm or the
    // differences | lo | hi); it, the check word and what a member's gr_prepare() allocates exist before any member is touched.
    struct BmGroup {
        MmDiffFn<REAL> diff;
        MmGradFn<REAL> grad;
        uint32_t threads, lds_diff, lds_grad, first, count;
    };
    std::vector<BmGroup> bm_groups;
    std::vector<MmItem<REAL>> bm_items;        // host copy, in launch order
    std::vector<uint32_t> bm_ord;              // item j is member bm_ord[j]
    MmItem<REAL>* d_bm_items = nullptr;
    REAL* d_bm_stage = nullptr;
    uint32_t* d_bm_bad = nullptr;
    uint64_t bm_layers = 0;                    // values of all members' layers
    bool bm_ready = false, bm_grad_ready = false;

    // grad: the call is the gradient, whose items need every member's parent tables and d_gr_arg; host_arrays: the call needs the staging buffer
    int bm_prepare(bool grad, bool host_arrays)
    {
        const uint32_t n = (uint32_t)m.size();
        constexpr uint32_t RS = (uint32_t)sizeof(REAL);
        if (!bm_ready) {
            std::vector<uint32_t> ord(n);
            for (uint32_t i = 0; i < n; ++i) ord[i] = i;
            std::stable_sort(ord.begin(), ord.end(), [&](uint32_t a, uint32_t b) { return m[a]->small_nw < m[b]->small_nw; });
            std::vector<uint64_t> src(n);
            uint64_t total = 0;
            for (uint32_t i = 0; i < n; ++i) {
                src[i] = total;
                total += m[i]->n_layers;
            }
            if (total > 0xFFFFFFFFull) { err = "batch min_marginal_diff: too many layers"; return BDDMMA_ERR_UNSUPPORTED; }
            std::vector<MmItem<REAL>> items(n);
            std::vector<BmGroup> groups_;
            for (uint32_t j = 0; j < n; ++j) {
                const S* s = m[ord[j]];
                const SmallDev& sm = s->small;
                items[j] = MmItem<REAL>{sm.pack_hdr, sm.rec, sm.rec_off, sm.rec_words, sm.ns, sm.nl, sm.n_packs, (uint32_t)s->n_layers, (uint32_t)src[ord[j]], ord[j],
                                        s->pack_width, s->ptrs(nullptr), s->pdev(s->nb_, 0, 0), nullptr, nullptr, nullptr};
                if (groups_.empty() || s->small_nw != m[ord[groups_.back().first]]->small_nw)
                    groups_.push_back(BmGroup{mm_diff_fn<REAL>(s->small_nw), mm_grad_fn<REAL>(s->small_nw), 64u * (uint32_t)s->small_nw, 0u, 0u, j, 0u});
                BmGroup& g = groups_.back();
                g.lds_diff = std::max(g.lds_diff, sm.n_packs * mmdiff_region_bytes(RS, sm.ns, sm.nl));
                g.lds_grad = std::max(g.lds_grad, sm.n_packs * mmgrad_region_bytes(RS, sm.ns, sm.nl));
                ++g.count;
            }
            for (const BmGroup& g : groups_) {
                // (never taken for a fused_small member: both regions are smaller than a pack's share of small_lds, kernels/batchmm.hpp)
                if (std::max(g.lds_diff, g.lds_grad) > m[0]->lds_cu) { err = "batch min_marginal_diff: the packs' state does not fit the LDS"; return BDDMMA_ERR_UNSUPPORTED; }
                if (int rc = raise_lds_limit(reinterpret_cast<const void*>(g.diff), g.lds_diff)) return rc;
                if (int rc = raise_lds_limit(reinterpret_cast<const void*>(g.grad), g.lds_grad)) return rc;
            }
            if (!d_bm_items) HIPCHK(hipMalloc((void**)&d_bm_items, n * sizeof(MmItem<REAL>)));
            if (!d_bm_bad) HIPCHK(hipMalloc((void**)&d_bm_bad, sizeof(uint32_t)));
            HIPCHK(hipMemcpy(d_bm_items, items.data(), n * sizeof(MmItem<REAL>), hipMemcpyHostToDevice));
            bm_items = std::move(items);
            bm_ord = std::move(ord);
            bm_groups = std::move(groups_);
            bm_layers = total;
            bm_ready = true;
        }
        if (grad && !bm_grad_ready) {
            for (S* s : m)
                if (int rc = s->gr_prepare()) { err = s->err; return rc; }
            for (uint32_t j = 0; j < n; ++j) {
                const S* s = m[bm_ord[j]];
                bm_items[j].par_ptr = s->d_sm_nptr;
                bm_items[j].par = s->d_sm_npar;
                bm_items[j].arg = s->d_gr_arg;
            }
            HIPCHK(hipStreamSynchronize(stream));   // nothing in flight reads the items
            HIPCHK(hipMemcpy(d_bm_items, bm_items.data(), n * sizeof(MmItem<REAL>), hipMemcpyHostToDevice));
            bm_grad_ready = true;
        }
        if (host_arrays && !d_bm_stage) HIPCHK(hipMalloc((void**)&d_bm_stage, std::max<uint64_t>(3 * bm_layers, 1) * sizeof(REAL)));
        return BDDMMA_OK;
    }
    // the host-side state after SolverT::min_marginal_diff / gr_min_marginal_diff: the costs-from-root are the plain sweep's (the launch has
    // stored them), the costs-to-terminal join_in's.  Behind a failed launch the costs-from-root are not known to be valid.
    void bm_launched(bool ok)
    {
        for (S* s : m) s->fwd_valid = ok;
    }
    int min_marginal_diff(void* out, int on_dev) override
    {
        int rc;
        if (!out) { err = "batch min_marginal_diff: null output pointer"; return BDDMMA_ERR_INVALID_ARGUMENT; }
        if ((rc = check_state())) return rc;
        HIPCHK(hipSetDevice(device));
        if ((rc = bm_prepare(false, !on_dev))) return rc;
        if ((rc = join_in())) { (void)join_out(); return rc; }
        // ---- the members are touched from here on (their costs-from-root)
        REAL* const o = on_dev ? (REAL*)out : d_bm_stage;
        hipError_t e = hipSuccess;
        for (size_t k = 0; k < bm_groups.size() && e == hipSuccess; ++k) {
            const BmGroup& G = bm_groups[k];
            hipLaunchKernelGGL(G.diff, dim3(G.count), dim3(G.threads), G.lds_diff, stream, (const MmItem<REAL>*)(d_bm_items + G.first), o);
            e = hipGetLastError();
        }
        bm_launched(e == hipSuccess);
        if (!on_dev) {
            if (e == hipSuccess) e = hipMemcpyAsync(out, o, bm_layers * sizeof(REAL), hipMemcpyDeviceToHost, stream);
            if (e == hipSuccess) e = hipStreamSynchronize(stream);
        }
        const int rc2 = join_out();
        if (e != hipSuccess) { err = std::string("batch min_marginal_diff: ") + hipGetErrorString(e); return BDDMMA_ERR_DEVICE; }
        return rc2;
    }
    int grad_min_marginal_diff(const void* grad_mm, void* grad_lo, void* grad_hi, int on_dev) override
    {
        int rc;
        const char* const me = "batch grad_min_marginal_diff";
        const uint32_t n = (uint32_t)m.size();
        if (!grad_mm || !grad_lo || !grad_hi) { err = std::string(me) + ": null pointer"; return BDDMMA_ERR_INVALID_ARGUMENT; }
        if ((rc = check_state())) return rc;
        HIPCHK(hipSetDevice(device));
        if ((rc = bm_prepare(true, !on_dev))) return rc;
        // the argument check, before any member or output is touched: host values here, device values by one launch for all members
        // (the batch stream is behind whatever the caller ordered it behind: bddmma_stream_wait_batch) and the call's one read
        uint32_t bad = 0xFFFFFFFFu;
        if (!on_dev) {
            const REAL* h = (const REAL*)grad_mm;
            for (uint32_t i = 0; i < n && bad == 0xFFFFFFFFu; ++i) {
                for (uint64_t l = 0; l < m[i]->n_layers; ++l)
                    if (!std::isfinite(h[l])) { bad = i; break; }
                h += m[i]->n_layers;
            }
        } else {
            HIPCHK(hipMemsetAsync(d_bm_bad, 0xFF, sizeof(uint32_t), stream));
            hipLaunchKernelGGL(mm_check_fn<REAL>(), dim3(n), dim3(256), 0, stream, (const MmItem<REAL>*)d_bm_items, (const REAL*)grad_mm, d_bm_bad);
            HIPCHK(hipGetLastError());
            HIPCHK(hipMemcpyAsync(&bad, d_bm_bad, sizeof(bad), hipMemcpyDeviceToHost, stream));
            HIPCHK(hipStreamSynchronize(stream));
        }
        if (bad != 0xFFFFFFFFu) {
            err = "batch member " + std::to_string(bad) + ": some of its grad_mm are not finite";
            return BDDMMA_ERR_INVALID_ARGUMENT;
        }
        if ((rc = join_in())) { (void)join_out(); return rc; }
        // ---- the members are touched from here on (their costs-from-root and d_gr_arg)
        const REAL* g = (const REAL*)grad_mm;
        REAL *lo = (REAL*)grad_lo, *hi = (REAL*)grad_hi;
        hipError_t e = hipSuccess;
        if (!on_dev) {
            e = hipMemcpyAsync(d_bm_stage, grad_mm, bm_layers * sizeof(REAL), hipMemcpyHostToDevice, stream);
            g = d_bm_stage;
            lo = d_bm_stage + bm_layers;
            hi = lo + bm_layers;
        }
        for (size_t k = 0; k < bm_groups.size() && e == hipSuccess; ++k) {
            const BmGroup& G = bm_groups[k];
            hipLaunchKernelGGL(G.grad, dim3(G.count), dim3(G.threads), G.lds_grad, stream, (const MmItem<REAL>*)(d_bm_items + G.first), g, lo, hi);
            e = hipGetLastError();
        }
        bm_launched(e == hipSuccess);
        if (!on_dev) {
            if (e == hipSuccess) e = hipMemcpyAsync(grad_lo, lo, bm_layers * sizeof(REAL), hipMemcpyDeviceToHost, stream);
            if (e == hipSuccess) e = hipMemcpyAsync(grad_hi, hi, bm_layers * sizeof(REAL), hipMemcpyDeviceToHost, stream);
            if (e == hipSuccess) e = hipStreamSynchronize(stream);
        }
        const int rc2 = join_out();
        if (e != hipSuccess) { err = std::string(me) + ": " + hipGetErrorString(e); return BDDMMA_ERR_DEVICE; }
        return rc2;
    }
    // ---- the log-sum-exp family, all members at once (kernels/batchsm.hpp: k_small_summarg_batch; the kernel compiles in
    // solver_bsm_f32.hip / _f64.hip): sum-marginals, smooth solutions and the gradient of the smooth per-BDD bounds are one kernel with
    // three epilogues.  Items sorted by the members' wave count, as the min-marginal items are: one launch per wave count present.  Host
    // arrays pass through one staging buffer the batch owns (per-BDD values | first output | second output); it, the parent tables of
    // every member's sm_prepare() and the bound items of the argument check exist before any member is touched.
    struct BsmGroup {
        SmBatchFn<REAL> fn;
        uint32_t threads, lds, first, count;
    };
    std::vector<BsmGroup> bsm_groups;
    SmItem<REAL>* d_bsm_items = nullptr;
    REAL* d_bsm_stage = nullptr;
    uint64_t bsm_layers = 0, bsm_bdds = 0;     // values of all members' layers / BDDs
    bool bsm_ready = false;

    // grad: the call is the gradient, whose argument check reads the bound items; host_arrays: the call needs the staging buffer
    int bsm_prepare(bool grad, bool host_arrays)
    {
        const uint32_t n = (uint32_t)m.size();
        constexpr uint32_t RS = (uint32_t)sizeof(REAL);
        if (!bsm_ready) {
            for (S* s : m)
                if (int rc = s->sm_prepare()) { err = s->err; return rc; }
            std::vector<uint32_t> ord(n);
            for (uint32_t i = 0; i < n; ++i) ord[i] = i;
            std::stable_sort(ord.begin(), ord.end(), [&](uint32_t a, uint32_t b) { return m[a]->small_nw < m[b]->small_nw; });
            std::vector<uint64_t> src(n), src_b(n);
            uint64_t total = 0, total_b = 0;
            for (uint32_t i = 0; i < n; ++i) {
                src[i] = total;
                src_b[i] = total_b;
                total += m[i]->n_layers;
                total_b += m[i]->n_bdds;
            }
            if (total > 0xFFFFFFFFull || total_b > 0xFFFFFFFFull) { err = "batch sum_marginals: too many layers"; return BDDMMA_ERR_UNSUPPORTED; }
            std::vector<SmItem<REAL>> items(n);
            std::vector<BsmGroup> groups_;
            for (uint32_t j = 0; j < n; ++j) {
                const S* s = m[ord[j]];
                items[j] = SmItem<REAL>{s->ptrs(nullptr), s->pdev(s->nb_, 0, 0), s->d_sm_nptr, s->d_sm_npar, s->d_bdd, s->pack_width, s->small.n_packs,
                                        (uint32_t)src[ord[j]], (uint32_t)src_b[ord[j]], ord[j]};
                if (groups_.empty() || s->small_nw != m[ord[groups_.back().first]]->small_nw)
                    groups_.push_back(BsmGroup{sm_batch_fn<REAL>(s->small_nw), 64u * (uint32_t)s->small_nw, 0u, j, 0u});
                BsmGroup& g = groups_.back();
                g.lds = std::max(g.lds, s->small.n_packs * bsm_region_bytes(RS, s->pack_width));
                ++g.count;
            }
            for (const BsmGroup& g : groups_) {
                // (never taken for a fused_small member: it has at most SMALL_MAX_PACKS = 16 packs of 64 slots, the condition of the
                // second-generation resident records, so at most 16 x 3 840 B = 60 KiB in double, below every lds_cu the layout accepts)
                if (g.lds > m[0]->lds_cu) { err = "batch sum_marginals: the packs' arrays do not fit the LDS"; return BDDMMA_ERR_STATE; }
                if (int rc = raise_lds_limit(reinterpret_cast<const void*>(g.fn), g.lds)) return rc;
            }
            if (!d_bsm_items) HIPCHK(hipMalloc((void**)&d_bsm_items, n * sizeof(SmItem<REAL>)));
            HIPCHK(hipMemcpy(d_bsm_items, items.data(), n * sizeof(SmItem<REAL>), hipMemcpyHostToDevice));
            bsm_groups = std::move(groups_);
            bsm_layers = total;
            bsm_bdds = total_b;
            bsm_ready = true;
        }
        if (grad)
            if (int rc = bb_prepare(false, false)) return rc;
        if (host_arrays && !d_bsm_stage) HIPCHK(hipMalloc((void**)&d_bsm_stage, std::max<uint64_t>(bsm_bdds + 2 * bsm_layers, 1) * sizeof(REAL)));
        return BDDMMA_OK;
    }
    // One call of the family: `mode` the epilogue (kernels/batchsm.hpp: BSM_*), g the per-BDD gradient (BSM_GRAD only), o1 null for
    // BSM_SMOOTH.  The arguments are checked and bsm_prepare() has run.
    int bsm_run(const char* me, uint32_t mode, const void* g_in, void* out0, void* out1, int on_dev)
    {
        int rc;
        if ((rc = members_in())) return rc;   // (no costs-to-terminal are needed: the sweeps compute their own potentials)
        // ---- the members are touched from here on (F, T, d_tmp0 / d_tmp1)
        const REAL* g = (const REAL*)g_in;
        REAL *o0 = (REAL*)out0, *o1 = (REAL*)out1;
        hipError_t e = hipSuccess;
        if (!on_dev) {
            if (g) {
                e = hipMemcpyAsync(d_bsm_stage, g_in, bsm_bdds * sizeof(REAL), hipMemcpyHostToDevice, stream);
                g = d_bsm_stage;
            }
            o0 = d_bsm_stage + bsm_bdds;
            if (out1) o1 = o0 + bsm_layers;
        }
        for (size_t k = 0; k < bsm_groups.size() && e == hipSuccess; ++k) {
            const BsmGroup& G = bsm_groups[k];
            hipLaunchKernelGGL(G.fn, dim3(G.count), dim3(G.threads), G.lds, stream, (const SmItem<REAL>*)(d_bsm_items + G.first), mode, g, o0, o1);
            e = hipGetLastError();
        }
        // the host-side state after SolverT::sm_launch_fwd and sm_launch_bwd: the stored potentials are log-partition values
        for (S* s : m) {
            s->fwd_valid = s->bwd_valid = s->lb_valid = false;
            s->lb_cached = false;
            ++s->lb_gen;
        }
        if (!on_dev) {
            if (e == hipSuccess) e = hipMemcpyAsync(out0, o0, bsm_layers * sizeof(REAL), hipMemcpyDeviceToHost, stream);
            if (e == hipSuccess && out1) e = hipMemcpyAsync(out1, o1, bsm_layers * sizeof(REAL), hipMemcpyDeviceToHost, stream);
            if (e == hipSuccess) e = hipStreamSynchronize(stream);
        }
        const int rc2 = join_out();
        if (e != hipSuccess) { err = std::string(me) + ": " + hipGetErrorString(e); return BDDMMA_ERR_DEVICE; }
        return rc2;
    }
    int sum_marginals(int log_probs, void* sm0, void* sm1, int on_dev) override
    {
        int rc;
        const char* const me = "batch sum_marginals";
        if (!sm0 || !sm1) { err = std::string(me) + ": null output pointer"; return BDDMMA_ERR_INVALID_ARGUMENT; }
        if ((rc = check_state())) return rc;
        HIPCHK(hipSetDevice(device));
        if ((rc = bsm_prepare(false, !on_dev))) return rc;
        return bsm_run(me, log_probs ? BSM_LOG : BSM_PROB, nullptr, sm0, sm1, on_dev);
    }
    int smooth_solution(void* out, int on_dev) override
    {
        int rc;
        const char* const me = "batch smooth_solution";
        if (!out) { err = std::string(me) + ": null output pointer"; return BDDMMA_ERR_INVALID_ARGUMENT; }
        if ((rc = check_state())) return rc;
        HIPCHK(hipSetDevice(device));
        if ((rc = bsm_prepare(false, !on_dev))) return rc;
        return bsm_run(me, BSM_SMOOTH, nullptr, out, nullptr, on_dev);
    }
    int grad_smooth_lower_bound_per_bdd(const void* grad_lb, void* grad_lo, void* grad_hi, int on_dev) override
    {
        int rc;
        const char* const me = "batch grad_smooth_lower_bound_per_bdd";
        const uint32_t n = (uint32_t)m.size();
        if (!grad_lb || !grad_lo || !grad_hi) { err = std::string(me) + ": null pointer"; return BDDMMA_ERR_INVALID_ARGUMENT; }
        if ((rc = check_state())) return rc;
        HIPCHK(hipSetDevice(device));
        if ((rc = bsm_prepare(true, !on_dev))) return rc;
        // the argument check, before any member or output is touched: host values here, device values by one launch for all members
        // (k_small_grad_lb_check over the bound items: the same per-BDD offsets) and the call's one read
        uint32_t bad = 0xFFFFFFFFu;
        if (!on_dev) {
            const REAL* h = (const REAL*)grad_lb;
            for (uint32_t i = 0; i < n && bad == 0xFFFFFFFFu; ++i) {
                for (uint64_t b = 0; b < m[i]->n_bdds; ++b)
                    if (!std::isfinite(h[b])) { bad = i; break; }
                h += m[i]->n_bdds;
            }
        } else {
            HIPCHK(hipMemsetAsync(d_bb_bad, 0xFF, sizeof(uint32_t), stream));
            hipLaunchKernelGGL(bound_check_fn<REAL>(), dim3(n), dim3(256), 0, stream, (const BoundItem<REAL>*)d_bb_items, (const REAL*)grad_lb, d_bb_bad);
            HIPCHK(hipGetLastError());
            HIPCHK(hipMemcpyAsync(&bad, d_bb_bad, sizeof(bad), hipMemcpyDeviceToHost, stream));
            HIPCHK(hipStreamSynchronize(stream));
        }
        if (bad != 0xFFFFFFFFu) {
            err = "batch member " + std::to_string(bad) + ": some of its grad_lb_per_bdd are not finite";
            return BDDMMA_ERR_INVALID_ARGUMENT;
        }
        return bsm_run(me, BSM_GRAD, grad_lb, grad_lo, grad_hi, on_dev);
    }
    // ---- primal rounding, all members at once (kernels/batchround.hpp: k_small_round_batch; the kernel compiles in solver_br_f32.hip /
    // _f64.hip).  Items sorted by the members' wave count, as the min-marginal items are: one launch per wave count present.  The batch
    // owns one `done` word and four counters per member (br_words: n done words in item order, then 4 n counters) and their pinned
    // host copy; they, the items and every member's d_mm_consumed exist before any member is touched.
    struct BrGroup {
        RoundFn<REAL> fn;
        uint32_t threads, lds, first, count;
    };
    std::vector<BrGroup> br_groups;
    std::vector<uint32_t> br_ord;              // item j is member br_ord[j]
    RoundItem<REAL>* d_br_items = nullptr;
    uint32_t *d_br_words = nullptr, *h_br_words = nullptr;
    bool br_ready = false;

    int br_prepare()
    {
        if (br_ready) return BDDMMA_OK;
        const uint32_t n = (uint32_t)m.size();
        constexpr uint32_t RS = (uint32_t)sizeof(REAL);
        if (int rc = bb_prepare(true, false)) return rc;   // every member's d_mm_consumed; the items of distribute_delta
        std::vector<uint32_t> ord(n);
        for (uint32_t i = 0; i < n; ++i) ord[i] = i;
        std::stable_sort(ord.begin(), ord.end(), [&](uint32_t a, uint32_t b) { return m[a]->small_nw < m[b]->small_nw; });
        if (!d_br_words) HIPCHK(hipMalloc((void**)&d_br_words, 5 * (size_t)n * sizeof(uint32_t)));
        if (!h_br_words) HIPCHK(hipHostMalloc((void**)&h_br_words, 5 * (size_t)n * sizeof(uint32_t), hipHostMallocDefault));
        std::vector<RoundItem<REAL>> items(n);
        std::vector<BrGroup> groups_;
        for (uint32_t j = 0; j < n; ++j) {
            const S* s = m[ord[j]];
            const SmallDev& sm = s->small;
            RoundItem<REAL>& it = items[j];
            it.mm = MmItem<REAL>{sm.pack_hdr, sm.rec, sm.rec_off, sm.rec_words, sm.ns, sm.nl, sm.n_packs, (uint32_t)s->n_layers, 0u, ord[j],
                                 s->pack_width, s->ptrs(nullptr), s->pdev(s->nb_, 0, 0), nullptr, nullptr, nullptr};
            it.mm_consumed = s->d_mm_consumed;
            it.delta_var = s->d_delta_var; it.delta_lay = s->d_delta_lay; it.delta_c = s->d_delta_c;
            it.var_ptr = s->d_var_ptr; it.var_layers = s->d_var_layers; it.layer_var = s->d_var; it.nbdds = s->d_nbdds;
            it.done = d_br_words + j;
            it.counts = d_br_words + n + 4 * (size_t)j;
            it.n_vars = (uint32_t)s->n_vars;
            if (groups_.empty() || s->small_nw != m[ord[groups_.back().first]]->small_nw)
                groups_.push_back(BrGroup{round_fn<REAL>(s->small_nw), 64u * (uint32_t)s->small_nw, 0u, j, 0u});
            BrGroup& g = groups_.back();
            // the largest phase: a region of k_small_mmdiff_batch per pack (kernels/batchround.hpp: round_lds_bytes)
            g.lds = std::max(g.lds, round_lds_bytes(RS, sm.ns, sm.nl, sm.n_packs));
            ++g.count;
        }
        for (const BrGroup& g : groups_) {
            // (never taken for a fused_small member: the region is smaller than a pack's share of small_lds, kernels/batchmm.hpp)
            if (g.lds > m[0]->lds_cu) { err = "batch rounding: the packs' state does not fit the LDS"; return BDDMMA_ERR_STATE; }
            if (int rc = raise_lds_limit(reinterpret_cast<const void*>(g.fn), g.lds)) return rc;
        }
        if (!d_br_items) HIPCHK(hipMalloc((void**)&d_br_items, n * sizeof(RoundItem<REAL>)));
        HIPCHK(hipMemcpy(d_br_items, items.data(), n * sizeof(RoundItem<REAL>), hipMemcpyHostToDevice));
        br_ord = std::move(ord);
        br_groups = std::move(groups_);
        br_ready = true;
        return BDDMMA_OK;
    }
    // SolverT::rounding_round(delta, round, seed, apply_update = true) of every member whose entry of `active` is non-zero (null: every
    // member; the device's done words are then cleared first, else they are what the earlier rounds of the loop left: !active).
    // counts: 4 per member; sol / c0 / c1: the members' n_vars values one behind the other, c0 / c1 may be null; all in member order, on
    // the host.  A member's part of sol is written only if its min-marginals agree; an inactive member's outputs are left alone.
    // agreed (may be null): 1 where they did.
    int rounding_round(double delta, uint32_t round, uint32_t seed, const char* active, uint32_t* counts, char* sol, void* c0, void* c1, char* agreed = nullptr)
    {
        int rc;
        const char* const me = "batch perturb_primal_costs";
        const uint32_t n = (uint32_t)m.size();
        if (!counts || !sol) { err = std::string(me) + ": null output pointer"; return BDDMMA_ERR_INVALID_ARGUMENT; }
        if ((rc = check_state())) return rc;
        HIPCHK(hipSetDevice(device));
        if ((rc = br_prepare())) return rc;
        if ((rc = members_in())) return rc;   // (no costs-to-terminal are needed: the kernel runs its own backward sweep)
        // ---- the members are touched from here on
        hipError_t e = hipSuccess;
        if (!active) e = hipMemsetAsync(d_br_words, 0, n * sizeof(uint32_t), stream);
        for (size_t k = 0; k < br_groups.size() && e == hipSuccess; ++k) {
            const BrGroup& G = br_groups[k];
            hipLaunchKernelGGL(G.fn, dim3(G.count), dim3(G.threads), G.lds, stream, (const RoundItem<REAL>*)(d_br_items + G.first), delta, round, seed);
            e = hipGetLastError();
        }
        // one copy of all done words and counters, one host synchronisation
        if (e == hipSuccess) e = hipMemcpyAsync(h_br_words, d_br_words, 5 * (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost, stream);
        if (e == hipSuccess) e = hipStreamSynchronize(stream);
        std::vector<uint64_t> voff(n + 1, 0);
        for (uint32_t i = 0; i < n; ++i) voff[i + 1] = voff[i] + m[i]->n_vars;
        // the host-side state after SolverT::rounding_round: distribute_delta, forward_run, the BWD_MARGINALS launch, and update_costs
        // where the member did not agree.  Behind a failure nothing is known to be valid.
        const bool ok = e == hipSuccess;
        for (uint32_t j = 0; j < n; ++j) {
            const uint32_t i = br_ord[j];
            if (active && !active[i]) continue;
            S* s = m[i];
            const bool done = ok && h_br_words[j] != 0;
            s->mm_consumed_valid = true;
            s->delta_var_valid = true;
            s->costs_changed();
            s->lb_cached = false;
            ++s->lb_gen;
            if (done) s->fwd_valid = s->bwd_valid = s->lb_valid = true;
            else s->costs_changed();
            if (!ok) continue;
            for (int k = 0; k < 4; ++k) counts[4 * (size_t)i + k] = h_br_words[n + 4 * (size_t)j + k];
            if (agreed) agreed[i] = done ? 1 : 0;
            // the outputs the per-member call copies: both differences where asked for, the solution where the member agreed
            const size_t vb = s->n_vars * sizeof(REAL);
            if (c0 && e == hipSuccess) e = hipMemcpyAsync((REAL*)c0 + voff[i], s->d_delta_c, vb, hipMemcpyDeviceToHost, stream);
            if (c1 && e == hipSuccess) e = hipMemcpyAsync((REAL*)c1 + voff[i], s->d_delta_c + s->n_vars, vb, hipMemcpyDeviceToHost, stream);
            if (done && e == hipSuccess) e = hipMemcpyAsync(sol + voff[i], s->d_sol, s->n_vars, hipMemcpyDeviceToHost, stream);
        }
        if (e == hipSuccess) e = hipStreamSynchronize(stream);
        const int rc2 = join_out();
        if (e != hipSuccess) { err = std::string(me) + ": " + hipGetErrorString(e); return BDDMMA_ERR_DEVICE; }
        return rc2;
    }
    int perturb_primal_costs(double delta, uint32_t round, uint32_t seed, uint32_t* counts, char* sol, void* c0, void* c1) override
    {
        return rounding_round(delta, round, seed, nullptr, counts, sol, c0, c1);
    }
    // bddmma_incremental_mm_agreement_rounding (no L-BFGS wrapper, not verbose) of every member: its call sequence with every per-member
    // call replaced by the batch's — distribute_delta, lower_bound, then per round rounding_round over the members still looking and
    // run_plain(num_itr_lb, 1e-7, 0.0001, DBL_MAX) over the same.  A member whose min-marginals agree leaves both from then on.  (The
    // round's own distribute_delta is part of the kernel, so round 0 applies already-cleared differences as the per-member call does.)
    int rounding(double init_delta, double growth, uint64_t num_itr_lb, uint64_t num_rounds, uint32_t seed, char* sol, int* found, uint64_t* rounds) override
    {
        int rc;
        const uint32_t n = (uint32_t)m.size();
        if (!sol || !found) { err = "batch rounding: null output pointer"; return BDDMMA_ERR_INVALID_ARGUMENT; }
        if (!(growth > 0) || !(init_delta > 0)) { err = "batch rounding: init_delta and delta_growth_rate must be positive"; return BDDMMA_ERR_INVALID_ARGUMENT; }
        if ((rc = check_state())) return rc;
        HIPCHK(hipSetDevice(device));
        if ((rc = br_prepare())) return rc;
        // ---- the members and the outputs are touched from here on
        for (uint32_t i = 0; i < n; ++i) {
            found[i] = 0;
            if (rounds) rounds[i] = num_rounds;
        }
        if ((rc = distribute_delta())) return rc;
        std::vector<double> lb(n);
        if ((rc = lower_bounds(lb.data()))) return rc;
        std::vector<char> active(n, 1), agreed(n, 0), mask(n, 0);
        std::vector<uint32_t> counts(4 * (size_t)n);
        double cur_delta = init_delta / growth;
        uint32_t left = n;
        for (uint64_t round = 0; round < num_rounds && left; ++round) {
            cur_delta = std::min(cur_delta * growth, 1e6);
            if ((rc = rounding_round(cur_delta, (uint32_t)round, seed, round == 0 ? nullptr : active.data(), counts.data(), sol, nullptr, nullptr, agreed.data()))) return rc;
            for (uint32_t i = 0; i < n; ++i)
                if (active[i] && agreed[i]) {
                    active[i] = 0;
                    mask[i] = 1;
                    found[i] = 1;
                    if (rounds) rounds[i] = round;
                    --left;
                }
            if (!left) break;
            if ((rc = run_plain(num_itr_lb, 1e-7, 0.0001, std::numeric_limits<double>::max(), nullptr, mask.data()))) return rc;
        }
        return BDDMMA_OK;
    }
    // ---- per-BDD solutions, cost updates and the gradient of a cost perturbation, all members at once (kernels/batchsol.hpp:
    // k_small_solution_batch, k_small_update_batch, k_small_grad_perturb_batch; the kernels compile in solver_bp_f32.hip / _f64.hip).
    // The solution kernel takes the bound gradient's items, groups and LDS (bb_prepare: one launch per wave count present) and, for host
    // output, its staging buffer; the two per-variable kernels have items of their own in the caller's order, one launch for all.  Their
    // host arrays pass through one staging buffer the batch owns; it and the check word are allocated before any member is touched.
    std::vector<SolutionFn<REAL>> bp_sol_fn;   // per entry of bb_groups
    PerturbItem<REAL>* d_bp_items = nullptr;
    unsigned char* d_bp_stage = nullptr;
    uint32_t* d_bp_bad = nullptr;
    uint64_t bp_layers = 0, bp_vars = 0;       // values of all members' layers / variables
    bool bp_ready = false;

    int bp_sol_prepare(bool host_arrays)
    {
        if (int rc = bb_prepare(false, host_arrays)) return rc;   // (its staging buffer holds bb_bdds + 2 bb_layers values: more than bb_layers bytes)
        if (bp_sol_fn.size() == bb_groups.size()) return BDDMMA_OK;
        std::vector<SolutionFn<REAL>> fns;
        for (const BbGroup& g : bb_groups) {
            fns.push_back(solution_fn<REAL>((int)(g.threads / 64u)));
            // the pack's region is the bound gradient's (kernels/batchbound.hpp: bound_region_bytes), g.lds the group's largest n_packs of them
            if (int rc = raise_lds_limit(reinterpret_cast<const void*>(fns.back()), g.lds)) return rc;
        }
        bp_sol_fn = std::move(fns);
        return BDDMMA_OK;
    }
    int bdds_solution(char* sol, int on_dev) override
    {
        int rc;
        if (!sol) { err = "batch bdds_solution: null output pointer"; return BDDMMA_ERR_INVALID_ARGUMENT; }
        if ((rc = check_state())) return rc;
        HIPCHK(hipSetDevice(device));
        if ((rc = bp_sol_prepare(!on_dev))) return rc;
        if ((rc = join_in())) { (void)join_out(); return rc; }
        char* const o = on_dev ? sol : reinterpret_cast<char*>(d_bb_stage);
        hipError_t e = hipSuccess;
        for (size_t k = 0; k < bb_groups.size() && e == hipSuccess; ++k) {
            const BbGroup& G = bb_groups[k];
            hipLaunchKernelGGL(bp_sol_fn[k], dim3(G.count), dim3(G.threads), G.lds, stream, (const BoundItem<REAL>*)(d_bb_items + G.first), o);
            e = hipGetLastError();
        }
        if (!on_dev) {
            if (e == hipSuccess) e = hipMemcpyAsync(sol, o, bb_layers, hipMemcpyDeviceToHost, stream);
            if (e == hipSuccess) e = hipStreamSynchronize(stream);
        }
        const int rc2 = join_out();
        if (e != hipSuccess) { err = std::string("batch bdds_solution: ") + hipGetErrorString(e); return BDDMMA_ERR_DEVICE; }
        return rc2;
    }
    // host_arrays: the call needs the staging buffer — update_costs: lo | hi, bp_vars values of up to 8 bytes each; the gradient:
    // grad_lo | grad_hi | lo_pert | hi_pert
    int bp_prepare(bool host_arrays)
    {
        const uint32_t n = (uint32_t)m.size();
        if (!bp_ready) {
            uint64_t total = 0, total_v = 0;
            std::vector<PerturbItem<REAL>> items(n);
            for (uint32_t i = 0; i < n; ++i) {
                const S* s = m[i];
                items[i] = PerturbItem<REAL>{s->d_lohi, s->d_var, s->d_nbdds, s->d_var_ptr, s->d_var_layers, (uint32_t)s->n_layers, (uint32_t)s->n_vars,
                                             (uint32_t)total, (uint32_t)total_v};
                total += s->n_layers;
                total_v += s->n_vars;
            }
            if (total > 0xFFFFFFFFull || total_v > 0xFFFFFFFFull) { err = "batch update_costs: too many layers"; return BDDMMA_ERR_UNSUPPORTED; }
            if (!d_bp_items) HIPCHK(hipMalloc((void**)&d_bp_items, n * sizeof(PerturbItem<REAL>)));
            if (!d_bp_bad) HIPCHK(hipMalloc((void**)&d_bp_bad, sizeof(uint32_t)));
            HIPCHK(hipMemcpy(d_bp_items, items.data(), n * sizeof(PerturbItem<REAL>), hipMemcpyHostToDevice));
            bp_layers = total;
            bp_vars = total_v;
            bp_ready = true;
        }
        if (host_arrays && !d_bp_stage)
            HIPCHK(hipMalloc((void**)&d_bp_stage, std::max<uint64_t>(std::max<uint64_t>(2 * bp_vars * sizeof(double), 2 * (bp_layers + bp_vars) * sizeof(REAL)), 16)));
        return BDDMMA_OK;
    }
    template <typename TIN>
    int update_both(const void* lo, const void* hi, int on_dev)
    {
        const TIN* a[2] = {(const TIN*)lo, (const TIN*)hi};
        hipError_t e = hipSuccess;
        if (!on_dev)
            for (int k = 0; k < 2 && e == hipSuccess; ++k)
                if (a[k]) {
                    TIN* const st = reinterpret_cast<TIN*>(d_bp_stage) + (uint64_t)k * bp_vars;
                    e = hipMemcpyAsync(st, a[k], bp_vars * sizeof(TIN), hipMemcpyHostToDevice, stream);
                    a[k] = st;
                }
        if (e == hipSuccess) {
            hipLaunchKernelGGL((perturb_update_fn<REAL, TIN>()), dim3((uint32_t)m.size()), dim3(256), 0, stream, (const PerturbItem<REAL>*)d_bp_items, a[0], a[1]);
            e = hipGetLastError();
        }
        if (e == hipSuccess && !on_dev) e = hipStreamSynchronize(stream);   // the caller may reuse its arrays on return
        // the host-side state after SolverT::update_costs
        for (S* s : m) s->costs_changed();
        const int rc2 = join_out();
        if (e != hipSuccess) { err = std::string("batch update_costs: ") + hipGetErrorString(e); return BDDMMA_ERR_DEVICE; }
        return rc2;
    }
    int update_costs(const void* lo, const void* hi, int elem_precision, int on_dev) override
    {
        int rc;
        if ((rc = check_state())) return rc;
        if (!lo && !hi) return BDDMMA_OK;
        HIPCHK(hipSetDevice(device));
        if ((rc = bp_prepare(!on_dev))) return rc;
        if ((rc = members_in())) return rc;
        // ---- the members are touched from here on
        return elem_precision == BDDMMA_F64 ? update_both<double>(lo, hi, on_dev) : update_both<float>(lo, hi, on_dev);
    }
    int grad_cost_perturbation(const void* grad_lo, const void* grad_hi, void* lo_pert, void* hi_pert, int on_dev) override
    {
        int rc;
        const char* const me = "batch grad_cost_perturbation";
        const uint32_t n = (uint32_t)m.size();
        if (!grad_lo || !grad_hi || !lo_pert || !hi_pert) { err = std::string(me) + ": null pointer"; return BDDMMA_ERR_INVALID_ARGUMENT; }
        if ((rc = check_state())) return rc;
        HIPCHK(hipSetDevice(device));
        if ((rc = bp_prepare(!on_dev))) return rc;   // (the members' variable -> layer tables exist since their construction)
        // the argument check, before any output is touched: host values here, device values by one launch for all members (the batch
        // stream is behind whatever the caller ordered it behind: bddmma_stream_wait_batch) and the call's one read.  bad: 2 * member + array
        uint32_t bad = 0xFFFFFFFFu;
        if (!on_dev) {
            const REAL* h[2] = {(const REAL*)grad_lo, (const REAL*)grad_hi};
            uint64_t at = 0;
            for (uint32_t i = 0; i < n && bad == 0xFFFFFFFFu; ++i) {
                for (uint32_t k = 0; k < 2u && bad == 0xFFFFFFFFu; ++k)
                    for (uint64_t l = 0; l < m[i]->n_layers; ++l)
                        if (!std::isfinite(h[k][at + l])) { bad = 2u * i + k; break; }
                at += m[i]->n_layers;
            }
        } else {
            HIPCHK(hipMemsetAsync(d_bp_bad, 0xFF, sizeof(uint32_t), stream));
            hipLaunchKernelGGL(perturb_check_fn<REAL>(), dim3(n), dim3(256), 0, stream, (const PerturbItem<REAL>*)d_bp_items, (const REAL*)grad_lo, (const REAL*)grad_hi, d_bp_bad);
            HIPCHK(hipGetLastError());
            HIPCHK(hipMemcpyAsync(&bad, d_bp_bad, sizeof(bad), hipMemcpyDeviceToHost, stream));
            HIPCHK(hipStreamSynchronize(stream));
        }
        if (bad != 0xFFFFFFFFu) {
            err = "batch member " + std::to_string(bad / 2u) + ": some of its " + ((bad & 1u) ? "grad_hi" : "grad_lo") + " are not finite";
            return BDDMMA_ERR_INVALID_ARGUMENT;
        }
        if ((rc = members_in())) return rc;   // (no member's state is read beyond its layout; the order is that of every batch call)
        const REAL *glo = (const REAL*)grad_lo, *ghi = (const REAL*)grad_hi;
        REAL *olo = (REAL*)lo_pert, *ohi = (REAL*)hi_pert;
        hipError_t e = hipSuccess;
        if (!on_dev) {
            REAL* const st = reinterpret_cast<REAL*>(d_bp_stage);
            e = hipMemcpyAsync(st, grad_lo, bp_layers * sizeof(REAL), hipMemcpyHostToDevice, stream);
            if (e == hipSuccess) e = hipMemcpyAsync(st + bp_layers, grad_hi, bp_layers * sizeof(REAL), hipMemcpyHostToDevice, stream);
            glo = st;
            ghi = st + bp_layers;
            olo = st + 2 * bp_layers;
            ohi = olo + bp_vars;
        }
        if (e == hipSuccess) {
            hipLaunchKernelGGL(perturb_grad_fn<REAL>(), dim3(n), dim3(256), 0, stream, (const PerturbItem<REAL>*)d_bp_items, glo, ghi, olo, ohi);
            e = hipGetLastError();
        }
        if (!on_dev) {
            if (e == hipSuccess) e = hipMemcpyAsync(lo_pert, olo, bp_vars * sizeof(REAL), hipMemcpyDeviceToHost, stream);
            if (e == hipSuccess) e = hipMemcpyAsync(hi_pert, ohi, bp_vars * sizeof(REAL), hipMemcpyDeviceToHost, stream);
            if (e == hipSuccess) e = hipStreamSynchronize(stream);
        }
        const int rc2 = join_out();
        if (e != hipSuccess) { err = std::string(me) + ": " + hipGetErrorString(e); return BDDMMA_ERR_DEVICE; }
        return rc2;
    }
    int stream_wait(hipStream_t other) override
    {
        HIPCHK(hipSetDevice(device));
        if (!ev_order) HIPCHK(hipEventCreateWithFlags(&ev_order, hipEventDisableTiming));
        HIPCHK(hipEventRecord(ev_order, other));
        HIPCHK(hipStreamWaitEvent(stream, ev_order, 0));
        return BDDMMA_OK;
    }
    int stream_signal(hipStream_t other) override
    {
        HIPCHK(hipSetDevice(device));
        if (!ev_order) HIPCHK(hipEventCreateWithFlags(&ev_order, hipEventDisableTiming));
        HIPCHK(hipEventRecord(ev_order, stream));
        HIPCHK(hipStreamWaitEvent(other, ev_order, 0));
        return BDDMMA_OK;
    }

    // ---- the members' lower bounds, all at once (kernels/batchlb.hpp: k_small_bound_batch; the kernel compiles in solver_bl_f32.hip /
    // _f64.hip).  The items and the groups are those of the solver costs (bc_prepare); a call's flags (LB_SKIP / LB_SWEEP / LB_REDUCE) are
    // kernel arguments, a group of more than LB_LAUNCH_ITEMS members is launched in slices.  The results of a host call arrive in pinned
    // memory the batch owns, each with a sequence word behind it that the host polls (SolverT::wait_bound's reasons).
    struct BlGroup {
        BoundSumFn<REAL> fn;
        uint32_t threads, lds, first, count;
    };
    std::vector<BlGroup> bl_groups;
    std::vector<uint32_t> bl_modes;                    // item order
    uint32_t* d_bl_words = nullptr;                    // item j -> its member's index in the caller's order
    double *h_bl_out = nullptr, *d_bl_out = nullptr;   // pinned + its device address: n doubles, then n sequence words
    uint64_t bl_seq = 0;
    bool bl_ready = false;
    // run_plain only: lower_bounds has put the batch stream behind the members' streams and left the join_out to its caller
    bool bl_joined = false;
    static constexpr uint32_t BL_STATIC_LDS = SMALL_MAX_PACKS * (uint32_t)sizeof(double);   // the kernel's `part`

    int bl_prepare()
    {
        if (int rc = bc_prepare(false)) return rc;
        if (bl_ready) return BDDMMA_OK;
        const uint32_t n = (uint32_t)m.size();
        std::vector<BlGroup> groups_;
        for (const BcGroup& g : bc_groups) {
            if (g.lds + BL_STATIC_LDS > m[0]->lds_cu) { err = "batch lower_bound: the costs-to-terminal do not fit the LDS"; return BDDMMA_ERR_UNSUPPORTED; }
            groups_.push_back(BlGroup{bound_sum_fn<REAL>((int)(g.threads / 64u)), g.threads, g.lds, g.first, g.count});
            if (int rc = raise_lds_limit(reinterpret_cast<const void*>(groups_.back().fn), g.lds)) return rc;
        }
        if (!d_bl_words) HIPCHK(hipMalloc((void**)&d_bl_words, n * sizeof(uint32_t)));
        HIPCHK(hipMemcpy(d_bl_words, bc_order.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice));
        if (!h_bl_out) {
            HIPCHK(hipHostMalloc((void**)&h_bl_out, 2 * (size_t)n * sizeof(double), hipHostMallocMapped | hipHostMallocCoherent));
            HIPCHK(hipHostGetDevicePointer((void**)&d_bl_out, h_bl_out, 0));
            std::memset((void*)h_bl_out, 0, 2 * (size_t)n * sizeof(double));
        }
        bl_modes.assign(n, 0u);
        bl_groups = std::move(groups_);
        bl_ready = true;
        return BDDMMA_OK;
    }
    // SolverT::lower_bound of every member that run_plain's mask leaves in: a stale member (where backward_run() would launch) sweeps in its
    // workgroup, every member reduces.  A host call takes a cached bound from the cache, as the per-member call does (the reduction's
    // result equals it), and leaves every member with its bound cached.
    // leave_joined (run_plain, which joins out itself): the members' streams are not made to wait here; bl_joined says that this happened.
    int lower_bounds(double* out, int on_dev = 0, bool check_members = false) override { return lower_bounds_impl(out, on_dev, check_members, false); }
    int lower_bounds_impl(double* out, int on_dev, bool check_members, bool leave_joined)
    {
        int rc;
        if (check_members && (rc = check_state())) return rc;
        HIPCHK(hipSetDevice(device));
        if ((rc = bl_prepare())) return rc;
        const uint32_t n = (uint32_t)m.size();
        bool any = false;
        for (uint32_t j = 0; j < n; ++j) {
            const uint32_t i = bc_order[j];
            bl_modes[j] = masked(i) ? LB_SKIP : !m[i]->bwd_valid ? LB_SWEEP : LB_REDUCE;
            any = any || bl_modes[j] != LB_SKIP;
        }
        if (!any) return BDDMMA_OK;
        if ((rc = members_in())) return rc;
        // ---- the members are touched from here on
        hipError_t e = hipSuccess;
        double* const dst = on_dev ? out : d_bl_out;
        uint64_t* const seq_dev = on_dev ? nullptr : reinterpret_cast<uint64_t*>(d_bl_out + n);
        volatile uint64_t* const seq_host = reinterpret_cast<volatile uint64_t*>(h_bl_out + n);
        const uint64_t seq = ++bl_seq;
        for (size_t g = 0; g < bl_groups.size() && e == hipSuccess; ++g) {
            const BlGroup& G = bl_groups[g];
            for (uint32_t first = G.first; first < G.first + G.count && e == hipSuccess; first += LB_LAUNCH_ITEMS) {
                const uint32_t count = std::min(LB_LAUNCH_ITEMS, G.first + G.count - first);
                LbFlags flags{};
                uint32_t live = 0;
                for (uint32_t k = 0; k < count; ++k) {
                    flags.w[k >> 4] |= bl_modes[first + k] << ((k & 15u) * LB_MODE_BITS);
                    live += bl_modes[first + k] != LB_SKIP;
                }
                if (!live) continue;
                hipLaunchKernelGGL(G.fn, dim3(count), dim3(G.threads), G.lds, stream, (const CostsItem<REAL>*)(d_bc_items + first), (const uint32_t*)(d_bl_words + first), flags, dst,
                                   seq_dev, seq);
                e = hipGetLastError();
            }
        }
        if (e == hipSuccess && !on_dev) {   // the one wait: every member's word, then a blocking wait after 2 ms without them
            const auto t0 = std::chrono::steady_clock::now();
            uint32_t spins = 0;
            for (uint32_t j = 0; j < n && e == hipSuccess; ++j) {
                if (bl_modes[j] == LB_SKIP) continue;
                volatile uint64_t* w = seq_host + bc_order[j];
                while (*w != seq) {
                    cpu_relax();
                    if ((++spins & 1023u) == 0 && std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > 2e-3) {
                        e = hipStreamSynchronize(stream);
                        if (e == hipSuccess && *w != seq) e = hipErrorUnknown;
                        break;
                    }
                }
            }
            std::atomic_thread_fence(std::memory_order_acquire);
        }
        for (uint32_t j = 0; j < n; ++j) {
            const uint32_t i = bc_order[j], mode = bl_modes[j];
            if (mode == LB_SKIP) continue;   // (its entry of `out` stays)
            S* s = m[i];
            if (mode == LB_SWEEP) {   // launch_sweep(bwd) and backward_run(); behind a failure nothing is known to be valid
                s->lb_cached = false;
                ++s->lb_gen;
                s->bwd_valid = s->lb_valid = e == hipSuccess;
            }
            if (e == hipSuccess && !on_dev) {
                if (!s->lb_cached) {
                    s->lb_cache = ((volatile double*)h_bl_out)[i];
                    s->lb_cached = true;
                }
                out[i] = s->lb_cache;
            }
        }
        if (e == hipSuccess && leave_joined) {
            bl_joined = true;
            return BDDMMA_OK;
        }
        const int rc2 = join_out();
        if (e != hipSuccess) { err = std::string("batch lower_bound: ") + hipGetErrorString(e); return BDDMMA_ERR_DEVICE; }
        return rc2;
    }

    // SolverT::run_plain for every member at once.  Chunks of SMALL_CHUNK iterations, the tests in each member's workgroup after every
    // iteration against its own control block; a member that has stopped returns at once in later chunks (DevPtrs::stop).  At most two
    // chunks are outstanding; the host waits for the older one and reads what the members have published.
    // mask (member order, may be null): a member whose entry is non-zero takes no part — its control block starts as stopped at iteration
    // 0, so its workgroup returns at once; its sweep states, run_stop, cached bound and entry of `res` are left alone.
    int run_plain(uint64_t max_iter, double tolerance, double slope, double time_limit, bddmma_run_result* res, const char* mask = nullptr) override
    {
        struct MaskScope {
            BatchT* b;
            ~MaskScope()
            {
                b->run_mask = nullptr;
                if (b->bl_joined) {   // a return between lower_bounds and the run's own join_out
                    b->bl_joined = false;
                    (void)b->join_out();
                }
            }
        } scope{this};
        run_mask = mask;
        if (slope < 0.0 || slope >= 1.0 || time_limit < 0.0 || tolerance < 0.0) {
            err = "run_solver: invalid termination criteria";
            return BDDMMA_ERR_INVALID_ARGUMENT;
        }
        int rc;
        if ((rc = check_state())) return rc;
        HIPCHK(hipSetDevice(device));
        const auto t0 = std::chrono::steady_clock::now();
        auto elapsed = [&]() { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); };
        const uint32_t n = (uint32_t)m.size();
        std::vector<double> lb_initial(n);
        // (with iterations to run the bounds' launch leaves the members' streams to the run's join_out; the batch stream is behind them then)
        if ((rc = lower_bounds_impl(lb_initial.data(), 0, false, max_iter > 0))) return rc;
        constexpr uint64_t MASK = (1ull << 56) - 1;
        if (max_iter > 0) {
            for (uint32_t j = 0; j < n; ++j) {
                RunCtl c{};
                c.stop = masked(order[j]) ? 0u : RUN_NOT_STOPPED;
                c.lb_initial = lb_initial[order[j]];
                c.lb_first = std::numeric_limits<double>::max();
                c.lb_post = c.lb_initial;
                c.tolerance = tolerance;
                c.slope = slope;
                c.time_limit = time_limit;
                h_ctl[j] = c;
            }
            std::memset((void*)h_run, 0, n * sizeof(RunHost));
            // no member is stale behind lower_bounds, and nothing has been queued on a member's stream since its members_in()
            if (!bl_joined && (rc = join_in())) return rc;
            HIPCHK(hipMemcpyAsync(d_ctl, h_ctl, n * sizeof(RunCtl), hipMemcpyHostToDevice, stream));
            hipLaunchKernelGGL(k_run_begin_batch, dim3(cdiv(n, 256)), dim3(256), 0, stream, d_ctl, n, (uint64_t)(elapsed() * RUN_TICKS_PER_SECOND));
            HIPCHK(hipGetLastError());
            constexpr uint64_t SMALL_CHUNK = 64;
            static_assert(2 * SMALL_CHUNK < RUN_RING, "published bounds must not wrap before the host has read them");
            for (uint32_t j = 0; j < n; ++j)
                if (!masked(order[j])) m[order[j]]->run_stop = &d_ctl[j].stop;   // "run_solver in progress", as run_plain marks it
            volatile RunHost* hr = h_run;
            uint64_t queued = 0, chunks = 0, waited = 0;
            while (!rc) {
                while (!rc && queued < max_iter && chunks - waited < 2) {
                    const uint64_t n_launch = std::min<uint64_t>(SMALL_CHUNK, max_iter - queued);
                    if ((rc = refresh(true, (uint32_t)std::min<uint64_t>(queued, RUN_NOT_STOPPED - 1))) || (rc = launch(REAL(0.5), (uint32_t)n_launch))) break;
                    const hipError_t e = hipEventRecord(ev_chunk[chunks & 1], stream);
                    if (e != hipSuccess) { err = std::string("hipEventRecord: ") + hipGetErrorString(e); rc = BDDMMA_ERR_DEVICE; break; }
                    queued += n_launch;
                    ++chunks;
                }
                if (rc || waited == chunks) break;
                const hipError_t e = hipEventSynchronize(ev_chunk[waited & 1]);
                if (e != hipSuccess) { err = std::string("run_solver: ") + hipGetErrorString(e); rc = BDDMMA_ERR_DEVICE; break; }
                ++waited;
                bool all_done = true;
                for (uint32_t j = 0; j < n && all_done; ++j) {
                    const uint64_t st = hr[j].state;
                    all_done = masked(order[j]) || (st >> 56) != 0 || (st & MASK) >= max_iter;
                }
                if (all_done) break;
            }
            const hipError_t e = hipStreamSynchronize(stream);   // launches behind the last stop return at once
            for (size_t i = 0; i < m.size(); ++i)
                if (!masked(i)) m[i]->run_stop = nullptr;
            if (!rc && e != hipSuccess) { err = std::string("run_solver: ") + hipGetErrorString(e); rc = BDDMMA_ERR_DEVICE; }
            bl_joined = false;
            const int rc2 = join_out();
            if (rc || rc2) return rc ? rc : rc2;
            for (uint32_t j = 0; j < n; ++j) {
                const uint64_t st = hr[j].state;
                if (!masked(order[j]) && (st >> 56) == 0 && (st & MASK) < queued) {
                    err = "run_solver: queued iterations of batch member " + std::to_string(order[j]) + " did not complete";
                    return BDDMMA_ERR_DEVICE;
                }
            }
        }
        const double seconds = elapsed();
        for (uint32_t j = 0; j < n; ++j) {
            if (masked(order[j])) continue;
            S* s = m[order[j]];
            const uint64_t st = max_iter > 0 ? ((volatile RunHost*)h_run)[j].state : 0;
            const uint64_t done = st & MASK;
            const double lb_final = done ? ((volatile RunHost*)h_run)[j].lb[(done - 1) % RUN_RING] : lb_initial[order[j]];
            if (done) {  // the device's bound of the last iteration that ran is lower_bound() of the state it left (same sum, same order)
                s->lb_cache = lb_final;
                s->lb_cached = true;
            }
            if (res) {
                bddmma_run_result& r = res[order[j]];
                r.iterations = done;
                r.lb_initial = lb_initial[order[j]];
                r.lb_final = lb_final;
                r.seconds = seconds;
                r.stop_reason = (int32_t)(st >> 56);
            }
        }
        return BDDMMA_OK;
    }
};

}  // namespace bddmma
