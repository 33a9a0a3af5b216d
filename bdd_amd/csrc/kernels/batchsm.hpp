// kernels/batchsm.hpp — the log-sum-exp family of a batch, one launch per wave count present (solver_bt.hpp: BatchT::sum_marginals,
// smooth_solution, grad_smooth_lower_bound_per_bdd).  k_small_summarg_batch: the two sum-marginal sweeps of every member and one of four
// per-layer epilogues, one workgroup per member, wave p on pack p, no workgroup barrier (packs are independent).
// Not part of kernels.hpp: the kernel is instantiated in solver_bsm_f32.hip / solver_bsm_f64.hip only (solver_bsm.hpp); solver_bt.hpp
// includes this file for the item and the getter.  Behind kernels.hpp.
#pragma once
#include "summarg.hpp"   // the sweeps' bodies
#include "batchmm.hpp"   // bm_memory_sync; GsWaveBar through gradsmall.hpp

namespace bddmma {

// What a member's workgroup needs, one entry per member of the batch, read-only for the launches (MmItem's addressing).  Member i's
// values start at `src` in each concatenated layer array and at `src_b` in the concatenated per-BDD array.
template <typename REAL>
struct SmItem {
    DevPtrs<REAL> d;                 // the arc costs are read; F, T and the log sum-marginals (mm0_out / mm1_out: d_tmp0 / d_tmp1) are written
    PackDev pk;                      // the narrow packs' hop tables
    const uint32_t *par_ptr, *par;   // the narrow words' parent tables (SolverT::sm_prepare)
    const int32_t* layer_bdd;        // [n_layers]
    uint32_t ww;                     // slots of a narrow pack
    uint32_t n_packs;
    uint32_t src, src_b;
    uint32_t member;                 // its index in the caller's order (the items are sorted by wave count)
};
// A pack's LDS region: the arrays of the two pull sweeps (sm_lds_bytes; the backward sweep reuses the forward's), 2 048 B in float and
// 3 840 B in double at 64 slots.
__host__ __device__ inline uint32_t bsm_region_bytes(uint32_t real_size, uint32_t ww) { return ((uint32_t)sm_lds_bytes(real_size, ww) + 15u) & ~15u; }

// What the epilogue writes per layer l of the member, from the log sum-marginals (s_lo, s_hi) the sweeps left:
enum : uint32_t {
    BSM_LOG = 0,      // out0 = s_lo, out1 = s_hi                                  (sum_marginals, log_probs)
    BSM_PROB = 1,     // out0 = exp(s_lo), out1 = exp(s_hi)                        (k_exp_pair)
    BSM_SMOOTH = 2,   // out0 = x = the smooth solution; out1 is not written       (k_smooth_solution)
    BSM_GRAD = 3      // out0 = (1 - x) g, out1 = x g, g = g_bdd[src_b + bdd of l]  (k_smooth_solution, k_grad_lb)
};

// SolverT::sm_launch_fwd and sm_launch_bwd for every member at once, then the elementwise kernel(s) of sm_sum_marginals, sm_smooth_solution
// or gr_lower_bound_per_bdd (smooth) and the copy to the caller, as one epilogue.  The sweeps are the bodies of k_sm_fwd / k_sm_bwd
// (kernels/summarg.hpp) on the wave's pack with T = 64 and the wave's ordering point; the forward leaves the pack's F~ in the member's own
// array, where the backward reads it, and the backward leaves the log sum-marginals of the pack's layers in the member's d_tmp0 / d_tmp1,
// where the epilogue reads them.  The epilogue's expressions are the elementwise kernels' (ew_*, kernels/elementwise.hpp), so every value is
// the per-member path's bit for bit.  `mode` is uniform over the launch and read behind the sweeps, outside every hop loop.
template <typename REAL, int NW>
__global__ void __launch_bounds__(64 * NW) k_small_summarg_batch(const SmItem<REAL>* __restrict__ items, uint32_t mode, const REAL* __restrict__ g_bdd,
                                                                 REAL* out0, REAL* out1)
{
    constexpr uint32_t S = sizeof(REAL);
    extern __shared__ __attribute__((aligned(16))) unsigned char dyn_lds[];
    const SmItem<REAL>& it = items[blockIdx.x];
    const uint32_t tid = threadIdx.x;
    const uint32_t p = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6)), lane = tid & 63u;
    if (p >= it.n_packs) return;
    const PackDev& pk = it.pk;
    const uint32_t q0 = pk.pack_hop_ptr[p], q1 = pk.pack_hop_ptr[p + 1];
    if (q0 == q1) return;
    const PullPack<REAL> pc{reinterpret_cast<REAL*>(dyn_lds + p * bsm_region_bytes(S, it.ww)), q0, q1, pk.pack_word_off[p] - pk.hop_node_off[q0], it.ww, lane, 64u};
    sm_fwd_body<REAL, true, GsWaveBar>(it.d, pk, pc, it.par_ptr, it.par, it.ww);
    bm_memory_sync();   // F~ is in memory
    sm_bwd_body<REAL, true, GsWaveBar>(it.d, pk, pc, it.par_ptr, it.par, it.ww);
    bm_memory_sync();   // the log sum-marginals of the pack's layers are in memory
    // ---- the epilogue over the pack's own layers [l0, l1)
    const uint32_t l0 = pk.hop_layer_off[q0], l1 = pk.hop_layer_off[q1];
    const REAL *const s_lo = it.d.mm0_out, *const s_hi = it.d.mm1_out;
    REAL* const o0 = out0 + it.src;
    REAL* const o1 = mode == BSM_SMOOTH ? nullptr : out1 + it.src;   // (no second output there: the caller passes none)
    if (mode == BSM_LOG) {
        for (uint32_t l = l0 + lane; l < l1; l += 64u) {
            o0[l] = s_lo[l];
            o1[l] = s_hi[l];
        }
    } else if (mode == BSM_PROB) {
        for (uint32_t l = l0 + lane; l < l1; l += 64u) {
            o0[l] = ew_exp(s_lo[l]);
            o1[l] = ew_exp(s_hi[l]);
        }
    } else if (mode == BSM_SMOOTH) {
        for (uint32_t l = l0 + lane; l < l1; l += 64u) o0[l] = ew_smooth_solution(s_lo[l], s_hi[l]);
    } else {
        const REAL* const g = g_bdd + it.src_b;
        for (uint32_t l = l0 + lane; l < l1; l += 64u) {
            const REAL xl = ew_smooth_solution(s_lo[l], s_hi[l]), gb = g[it.layer_bdd[l]];
            o1[l] = ew_grad_lb_hi(xl, gb);
            o0[l] = ew_grad_lb_lo(xl, gb);
        }
    }
}

// The instantiations (defined in solver_bsm.hpp, compiled in solver_bsm_f32.hip / _f64.hip): the kernel for members of `nw` waves
template <typename REAL>
using SmBatchFn = void (*)(const SmItem<REAL>*, uint32_t, const REAL*, REAL*, REAL*);
template <typename REAL>
SmBatchFn<REAL> sm_batch_fn(int nw);

}  // namespace bddmma
