// kernels/batchround.hpp — one round of primal rounding by cost perturbation for a batch, one launch (solver_bt.hpp:
// BatchT::rounding_round).  k_small_round_batch: SolverT::rounding_round(delta, round, seed, apply_update = true) of every member, one
// workgroup per member, wave p on pack p.  Not part of kernels.hpp: the kernel is instantiated in solver_br_f32.hip / solver_br_f64.hip
// only (solver_br.hpp); solver_bt.hpp includes this file for the item and the getter.  Behind kernels.hpp.
#pragma once
#include "batchcosts.hpp"   // costs_backward
#include "batchmm.hpp"      // MmItem, bm_pack, bm_forward, bm_memory_sync

namespace bddmma {

// What a member's workgroup needs, one entry per member of the batch, read-only for the launches (MmItem's addressing; `mm.d` carries the
// member's T, F, arc costs, deferred differences, lpos, lb_partial and the two minima arrays and the solution buffer of its own sweeps).
template <typename REAL>
struct RoundItem {
    MmItem<REAL> mm;
    REAL* mm_consumed;            // what bddmma_grad_distribute_delta of the member reads
    REAL* delta_var;              // 2 n_vars
    REAL* delta_lay;              // 2 n_layers
    REAL* delta_c;                // the member's rounding scratch: [0, V) cost_delta_0, [V, 2V) cost_delta_1
    const uint32_t* var_ptr;      // variable -> its range in var_layers
    const uint32_t* var_layers;
    const int32_t* layer_var;     // layer -> variable
    const int32_t* nbdds;         // variable -> number of its BDDs
    uint32_t* done;               // the member's word of the batch: set by the kernel once the member's min-marginals agree
    uint32_t* counts;             // the member's four counters of the batch: #one, #zero, #equal, #inconsistent
    uint32_t n_vars;
};
// The dynamic LDS of a member: the backward sweep, the forward pass and its minima live in the pack's region of k_small_mmdiff_batch
// (mmdiff_region_bytes; the backward sweep uses its costs-to-terminal and its layer pairs), the per-variable and the per-layer phases use
// the four counters in static LDS only.  The largest phase is therefore n_packs regions.
__host__ __device__ inline uint32_t round_lds_bytes(uint32_t real_size, uint32_t ns, uint32_t nl, uint32_t n_packs) { return n_packs * mmdiff_region_bytes(real_size, ns, nl); }

// Values one wave has written to global memory and another wave of the workgroup reads: release, the workgroup's barrier, acquire
__device__ __forceinline__ void round_group_sync()
{
    bm_memory_sync();
    __syncthreads();
}

// For member blockIdx.x, what SolverT::rounding_round does to it:
//  (1) nothing if its `done` word is set (uniform over the workgroup, in front of the first barrier);
//  (2) distribute_delta: k_small_distribute_batch's body (kernels/batchbound.hpp) over the workgroup's threads;
//  (3) the plain backward sweep out of LDS: costs_backward (kernels/batchcosts.hpp), the costs-to-terminal and the pack's bound as the
//      BWD_MARGINALS sweep leaves them;
//  (4) the plain forward pass with the two minima per layer: bm_forward<REAL, true> (kernels/batchmm.hpp); F to the member's array, the
//      minima to the arrays the member's own sweep writes;
//  (5) a thread per variable: ew_round_perturb (kernels/elementwise.hpp), the counters by LDS atomics;
//  (6) on the counters: all variables agree -> `done`; else update_costs(c0, c1) by ew_cost_quotient / ew_cost_add per layer.
// Every wave reaches every barrier: a wave without a pack (the member has fewer packs than NW) skips (3) and (4) only.
template <typename REAL, int NW>
__global__ void __launch_bounds__(64 * NW) k_small_round_batch(const RoundItem<REAL>* __restrict__ items, double delta, uint32_t round, uint32_t seed)
{
    constexpr uint32_t S = sizeof(REAL);
    constexpr uint32_t NT = 64 * NW;
    using P2 = typename Pair<REAL>::type;
    extern __shared__ __attribute__((aligned(16))) unsigned char dyn_lds[];
    __shared__ uint32_t cnt[4];
    const RoundItem<REAL>& it = items[blockIdx.x];
    const MmItem<REAL>& mi = it.mm;
    // ---- (1)
    if (*it.done != 0u) return;
    const uint32_t tid = threadIdx.x;
    const uint32_t p = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6)), lane = tid & 63u;
    const uint32_t n_layers = mi.n_layers, n_vars = it.n_vars;
    // ---- (2)
    for (uint32_t e = tid; e < n_layers; e += NT) it.mm_consumed[e] = mi.d.mm_binned[e];
    if (tid < 4u) cnt[tid] = 0u;
    round_group_sync();   // (the copy is by entry, the rest by layer)
    for (uint32_t l = tid; l < n_layers; l += NT) {
        const uint32_t e = mi.d.lpos[l];
        const REAL m = mi.d.mm_binned[e];
        if (m > 0) mi.d.lohi[2 * (size_t)l + 1] += m;
        else mi.d.lohi[2 * (size_t)l] -= m;
        mi.d.mm_binned[e] = REAL(0);
    }
    for (uint32_t k = tid; k < 2u * n_vars; k += NT) it.delta_var[k] = REAL(0);
    for (uint32_t k = tid; k < 2u * n_layers; k += NT) it.delta_lay[k] = REAL(0);
    round_group_sync();   // the arc costs: written by layer, read by pack
    // ---- (3), (4)
    BmPack pb{};
    if (p < mi.n_packs) pb = bm_pack(mi, p);
    if (p < mi.n_packs && pb.nh != 0u) {
        const uint32_t wb = p * mmdiff_region_bytes(S, mi.ns, mi.nl), wbC = wb + res2_c_off(S, mi.ns);
        for (uint32_t j = lane; j < pb.nlayers; j += 64u)
            lds_st<P2>(dyn_lds, wbC + j * (uint32_t)sizeof(P2), reinterpret_cast<const P2*>(mi.d.lohi)[(size_t)pb.layer0 + j]);
        if (lane < 2u) lds_st<REAL>(dyn_lds, wb + (mi.ns + lane) * S, lane == 0u ? REAL(0) : inf_v<REAL>());  // sinks: cost to terminal 0 (top) / +inf (bot)
        wave_sync();
        const double lb = costs_backward<REAL>(dyn_lds, wb, wbC, make_rsrc(mi.rec, mi.rec_words), pb.rbase, pb.nh, lane, reinterpret_cast<unsigned char*>(mi.d.T + pb.slot0));
        if (lane == 0u) mi.d.lb_partial[p] = lb;
        bm_memory_sync();   // T is in memory, where the forward pass reads it
        bm_forward<REAL, true>(dyn_lds, mi, pb, lane, wb);
        const uint32_t m0 = wb + res2_wave_bytes(S, mi.ns, mi.nl), m1 = m0 + mi.nl * S;
        for (uint32_t j = lane; j < pb.nlayers; j += 64u) {
            mi.d.mm0_out[(size_t)pb.layer0 + j] = lds_ld<REAL>(dyn_lds, m0 + j * S);
            mi.d.mm1_out[(size_t)pb.layer0 + j] = lds_ld<REAL>(dyn_lds, m1 + j * S);
        }
    }
    round_group_sync();   // the minima: written by pack, read by variable
    // ---- (5)
    REAL* const c0 = it.delta_c;
    REAL* const c1 = it.delta_c + n_vars;
    for (uint32_t v = tid; v < n_vars; v += NT) {
        REAL d0, d1;
        ew_round_perturb<REAL>(mi.d.mm0_out, mi.d.mm1_out, it.var_ptr, it.var_layers, v, delta, round, seed, d0, d1, [&](int type) {
            atomicAdd(&cnt[type], 1u);
            mi.d.sol_out[v] = type == 0 ? 1 : 0;
        });
        c0[v] = d0;
        c1[v] = d1;
    }
    round_group_sync();   // the counters; the cost differences: written by variable, read by layer
    // ---- (6)
    const uint32_t n_one = cnt[0], n_zero = cnt[1];
    if (tid < 4u) it.counts[tid] = cnt[tid];
    if (n_one + n_zero == n_vars) {   // all min-marginals agree: the solution stands, the costs stay
        if (tid == 0u) *it.done = 1u;
        return;
    }
    for (uint32_t l = tid; l < n_layers; l += NT) {
        const int v = it.layer_var[l];
        const double nb = (double)it.nbdds[v];
        P2 c = reinterpret_cast<P2*>(mi.d.lohi)[l];
        ew_cost_add<REAL>(c, CostQuot{ew_cost_quotient(c0[v], nb), ew_cost_quotient(c1[v], nb)}, 0u, 1u, 1u);   // both vectors full length: no flag
        reinterpret_cast<P2*>(mi.d.lohi)[l] = c;
    }
}

// The instantiations (defined in solver_br.hpp, compiled in solver_br_f32.hip / _f64.hip): the kernel for members of `nw` waves
template <typename REAL>
using RoundFn = void (*)(const RoundItem<REAL>*, double, uint32_t, uint32_t);
template <typename REAL>
RoundFn<REAL> round_fn(int nw);

}  // namespace bddmma
