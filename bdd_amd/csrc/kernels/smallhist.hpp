// kernels/smallhist.hpp — a batch's learned iterations with their history inside the member's workgroup (k_learned_small_hist_batch:
// bddmma_learned_iterations_history_batch; BatchT::learned_iterations_history, solver_bt.hpp).  Behind kernels.hpp; the history step itself
// is the HISTORY form of small_iterate (kernels/small.hpp).  The kernels compile in solver_sh_f32.hip / solver_sh_f64.hip only.
#pragma once

namespace bddmma {

// What a member's workgroup takes: the learned item and what the history step reads from memory (SmallHistMem).  Of that, the outputs
// and beta belong to a call: k_hist_items_call writes them in stream order before the call's first launch.
template <typename REAL>
struct SmallHistItem {
    SmallLearnItem<REAL> fw;
    SmallHistMem<REAL> hm;
    uint32_t src_l, src_b;   // first layer / first BDD of the member in the caller's concatenated arrays
};
template <typename REAL>
__global__ void k_hist_items_call(SmallHistItem<REAL>* items, uint32_t n, REAL* sol_avg, REAL* lb_first, REAL* lb_second, REAL beta)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    items[i].hm.sol_avg = sol_avg + items[i].src_l;
    items[i].hm.lb_first = lb_first + items[i].src_b;
    items[i].hm.lb_second = lb_second + items[i].src_b;
    items[i].hm.beta = beta;
}

// hist_from: the launch's first tracked iteration; tracked: the history steps the call has made before this launch
template <typename REAL, int NW, bool RL>
__global__ void __launch_bounds__(64 * NW) k_learned_small_hist_batch(const SmallHistItem<REAL>* items, REAL omega, uint32_t n_iters, uint32_t use_ov, uint32_t hist_from,
                                                                      uint32_t tracked)
{
    const SmallHistItem<REAL>& item = items[blockIdx.x];
    SmallLearn<REAL> ln = item.fw.ln;
    if (!use_ov) ln.omega_lay = nullptr;
    const SmallHist<REAL> hs{&item.hm, hist_from, tracked};
    small_iterate<REAL, NW, RL, true, false, true>(item.fw.sm, item.fw.d, item.fw.pk, omega, n_iters, RunStep{}, &ln, nullptr, &hs);
}

}  // namespace bddmma
