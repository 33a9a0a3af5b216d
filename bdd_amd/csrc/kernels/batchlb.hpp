// kernels/batchlb.hpp — a batch's lower bounds in one launch (solver_bt.hpp: BatchT::lower_bounds).  k_small_bound_batch: the plain
// backward sweep of every stale member and the reduction of every member's partial sums, one workgroup per member.  Not part of
// kernels.hpp: the kernel is instantiated in solver_bl_f32.hip / solver_bl_f64.hip only (solver_bl.hpp); solver_bt.hpp includes this file
// for the flags and the getter.
#pragma once
#include "batchcosts.hpp"

namespace bddmma {

// What an item's workgroup does in this call: two bits per item, the items of one launch in a block of words passed by value (a kernel
// argument: no copy and no buffer that a later call could overwrite under a launch still queued).
constexpr uint32_t LB_SKIP = 0u;     // a member run_plain masks: nothing is read but the flag, nothing is written
constexpr uint32_t LB_SWEEP = 1u;    // stale costs-to-terminal: SolverT::backward_run() in the workgroup, then the reduction
constexpr uint32_t LB_REDUCE = 2u;   // the partial sums the last backward sweep left are those of the current costs
constexpr uint32_t LB_MODE_BITS = 2u;
constexpr uint32_t LB_LAUNCH_ITEMS = 128u;   // items per launch: a group of more members is launched in slices
struct LbFlags {
    uint32_t w[LB_LAUNCH_ITEMS * LB_MODE_BITS / 32u];
};

// sweep: (b) of k_small_set_batch with the arc costs from the member's lohi — wave p on pack p, T and the pack's partial sum written back.
// reduce: behind one workgroup barrier wave 0 sums the member's partial sums in k_lb_reduce's shape — at most SMALL_MAX_PACKS of them, so
// thread i of that kernel's 1 024 holds pack i's (0.0 + it) and the other fifteen waves' results are 0.0: an in-wave tree over lane i's
// value (0.0 beyond n_packs), then t = 0.0; t += the tree's result — and lane 0 writes out[member].  A swept pack's sum goes through the
// static array `part`, which a pack that is not swept fills from lb_partial.
// member[j]: item j's index in the caller's order.  seq_out (pinned host memory, may be null): member i's word receives `seq` behind its
// bound, as k_lb_reduce's does — the host polls the words instead of waiting for the stream.
template <typename REAL, int NW>
__global__ void __launch_bounds__(64 * NW) k_small_bound_batch(const CostsItem<REAL>* __restrict__ items, const uint32_t* __restrict__ member, const LbFlags flags,
                                                               double* __restrict__ out, uint64_t* __restrict__ seq_out, uint64_t seq)
{
    constexpr uint32_t S = sizeof(REAL);
    using P2 = typename Pair<REAL>::type;
    static_assert(SMALL_MAX_PACKS <= 64, "lane i of wave 0 holds pack i's partial sum");
    extern __shared__ __attribute__((aligned(16))) unsigned char dyn_lds[];
    __shared__ double part[SMALL_MAX_PACKS];
    const uint32_t mode = (flags.w[blockIdx.x >> 4] >> ((blockIdx.x & 15u) * LB_MODE_BITS)) & ((1u << LB_MODE_BITS) - 1u);
    if (mode == LB_SKIP) return;   // (uniform over the workgroup)
    const CostsItem<REAL>& it = items[blockIdx.x];
    const uint32_t tid = threadIdx.x;
    const uint32_t p = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6));
    const uint32_t lane = tid & 63u;
    if (p < it.n_packs) {   // (wave-uniform; a member of n_packs <= NW waves' worth of packs)
        const uint32_t* const hp = it.pack_hdr + 8 * (size_t)p;
        const uint32_t nh = __builtin_amdgcn_readfirstlane(hp[5] & 0xFFFFu);
        double lb;
        if (mode == LB_SWEEP && nh != 0u) {
            const uint32_t slot0 = hp[0], layer0 = hp[2], nlayers = hp[3];
            const uint32_t rbase = __builtin_amdgcn_readfirstlane(it.rec_off[p]);
            const uint32_t wb = p * costs_region_bytes(S, it.ns, it.nl), wbC = wb + (it.ns + 4u) * S;
            const rsrc_t rr = make_rsrc(it.rec, it.rec_words);
            for (uint32_t j = lane; j < nlayers; j += 64u) lds_st<P2>(dyn_lds, wbC + j * (uint32_t)sizeof(P2), reinterpret_cast<const P2*>(it.lohi)[(size_t)layer0 + j]);
            if (lane < 2u) lds_st<REAL>(dyn_lds, wb + (it.ns + lane) * S, lane == 0u ? REAL(0) : inf_v<REAL>());  // sinks: cost to terminal 0 (top) / +inf (bot)
            wave_sync();
            lb = costs_backward<REAL>(dyn_lds, wb, wbC, rr, rbase, nh, lane, reinterpret_cast<unsigned char*>(it.T + slot0));
            if (lane == 0u) it.lb_partial[it.lb_base + p] = lb;
        } else {
            lb = it.lb_partial[it.lb_base + p];   // (a pack without a hop: what the member's own sweeps leave there)
        }
        if (lane == 0u) part[p] = lb;
    }
    __syncthreads();
    if (p == 0u) {
        double acc = lane < it.n_packs ? part[lane] : 0.0;
        for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off);
        if (lane == 0u) {
            double t = 0.0;
            t += acc;
            const uint32_t i = member[blockIdx.x];
            out[i] = t;
            if (seq_out != nullptr) {
                __threadfence_system();
                *reinterpret_cast<volatile uint64_t*>(seq_out + i) = seq;
            }
        }
    }
}

// The instantiations (defined in solver_bl.hpp, compiled in solver_bl_f32.hip / _f64.hip): the kernel for members of `nw` waves
template <typename REAL>
using BoundSumFn = void (*)(const CostsItem<REAL>*, const uint32_t*, LbFlags, double*, uint64_t*, uint64_t);
template <typename REAL>
BoundSumFn<REAL> bound_sum_fn(int nw);

}  // namespace bddmma
