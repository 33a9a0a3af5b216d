// kernels/smallstop.hpp — a batch's learned iterations that stop on the bound's slope inside the member's workgroup
// (k_learned_small_stop_batch, k_learned_small_hist_stop_batch: bddmma_learned_iterations_stop_batch; BatchT::learned_iterations_stop,
// solver_bt.hpp).  Behind kernels/smallhist.hpp; the rule itself is the STOP form of small_iterate (kernels/small.hpp).  The kernels compile in
// solver_ss_f32.hip / solver_ss_f64.hip only.
#pragma once

namespace bddmma {

// What a member's workgroup takes: the history item (the form without a history reads its learned part only) and the member's stop block.
template <typename REAL>
struct SmallStopItem {
    SmallHistItem<REAL> hi;
    SmallStopBlock* stop;
};
// The outputs and beta of a call with a history (k_hist_items_call for these items), in stream order before the call's first launch.
template <typename REAL>
__global__ void k_stop_items_call(SmallStopItem<REAL>* items, uint32_t n, REAL* sol_avg, REAL* lb_first, REAL* lb_second, REAL beta)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    items[i].hi.hm.sol_avg = sol_avg + items[i].hi.src_l;
    items[i].hi.hm.lb_first = lb_first + items[i].hi.src_b;
    items[i].hi.hm.lb_second = lb_second + items[i].hi.src_b;
    items[i].hi.hm.beta = beta;
}

// n_iters: the launch's iterations — what is left of the call's where that is less than a chunk.  Without a history
// (compute_history_for_itr = 0) ...
template <typename REAL, int NW, bool RL>
__global__ void __launch_bounds__(64 * NW) k_learned_small_stop_batch(const SmallStopItem<REAL>* items, REAL omega, uint32_t n_iters, uint32_t use_ov)
{
    const SmallStopItem<REAL>& item = items[blockIdx.x];
    SmallLearn<REAL> ln = item.hi.fw.ln;
    if (!use_ov) ln.omega_lay = nullptr;
    small_iterate<REAL, NW, RL, true, false, false, true>(item.hi.fw.sm, item.hi.fw.d, item.hi.fw.pk, omega, n_iters, RunStep{}, &ln, nullptr, nullptr, &item.stop);
}
// ... and with one: iteration g of the call is tracked when cfi >= num_itr - g or an earlier iteration's test has set `converged`
template <typename REAL, int NW, bool RL>
__global__ void __launch_bounds__(64 * NW) k_learned_small_hist_stop_batch(const SmallStopItem<REAL>* items, REAL omega, uint32_t n_iters, uint32_t use_ov)
{
    const SmallStopItem<REAL>& item = items[blockIdx.x];
    SmallLearn<REAL> ln = item.hi.fw.ln;
    if (!use_ov) ln.omega_lay = nullptr;
    const SmallHist<REAL> hs{&item.hi.hm, 0u, 0u};
    small_iterate<REAL, NW, RL, true, false, true, true>(item.hi.fw.sm, item.hi.fw.d, item.hi.fw.pk, omega, n_iters, RunStep{}, &ln, nullptr, &hs, &item.stop);
}

}  // namespace bddmma
