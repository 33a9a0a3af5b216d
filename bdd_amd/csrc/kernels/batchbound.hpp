// kernels/batchbound.hpp — the tail of a training step's loss for a batch, one launch each (solver_bt.hpp: BatchT::lower_bound_per_bdd,
// grad_lower_bound_per_bdd, distribute_delta).  k_small_bounds_batch: lower_bound_per_bdd of every member; k_small_grad_lb_batch:
// grad_lower_bound_per_bdd (smooth = 0) of every member, one workgroup per member; k_small_distribute_batch: distribute_delta of every
// member.  Not part of kernels.hpp: the kernels are instantiated in solver_bb_f32.hip / solver_bb_f64.hip only (solver_bb.hpp);
// solver_bt.hpp includes this file for the item and the getters.  bound_path_pass, the arg-min path pass of a pack, is shared with
// k_small_solution_batch (kernels/batchsol.hpp).
#pragma once

namespace bddmma {

// What a member's workgroup needs, one entry per member of the batch, read-only for the launches (CostsItem's addressing: the item's
// address is uniform, its fields arrive by scalar loads).  Member i's values start at `src` in each concatenated layer array and at
// `src_b` in each concatenated per-BDD array.
template <typename REAL>
struct BoundItem {
    const uint32_t* pack_hdr;   // layout.hpp: struct Resident — 8 words per pack
    const uint32_t* rec;        // Res2Records
    const uint32_t* rec_off;
    const uint32_t* lpos;       // layer -> its entry in mm_binned
    const uint32_t* root_slot;  // [n_bdds]: the slot of BDD b's root (the order of bddmma_lower_bound_per_bdd)
    const int32_t* layer_bdd;   // [n_layers]
    const REAL* T;
    REAL* lohi;
    REAL* mm_binned;
    REAL* mm_consumed;          // null until the batch's first distribute_delta
    REAL* delta_var;
    REAL* delta_lay;
    uint32_t rec_words;
    uint32_t ns, nl;            // slot / layer capacity the records' offsets were built for
    uint32_t n_packs, n_layers, n_bdds, n_vars;
    uint32_t src, src_b;
    uint32_t member;            // its index in the caller's order (the items are sorted by wave count)
};
// A pack's LDS region of k_small_grad_lb_batch: the region of the second-generation resident records [T: (ns + 4) S | F: (ns + 64) S |
// {lo, hi}: nl 2 S] (res2_wave_bytes), then [marks: 64 S | decisions: nl S].
__host__ __device__ inline uint32_t bound_region_bytes(uint32_t real_size, uint32_t ns, uint32_t nl)
{
    return (res2_wave_bytes(real_size, ns, nl) + 64u * real_size + nl * real_size + 15u) & ~15u;
}

// out[src_b + b] = T[root_slot[b]] for every BDD b of every member (k_lb_per_bdd for every member at once)
template <typename REAL>
__global__ void __launch_bounds__(256) k_small_bounds_batch(const BoundItem<REAL>* __restrict__ items, REAL* __restrict__ out)
{
    const BoundItem<REAL>& it = items[blockIdx.x];
    for (uint32_t b = threadIdx.x; b < it.n_bdds; b += 256u) out[(size_t)it.src_b + b] = it.T[it.root_slot[b]];
}

// The argument check of the gradient: the first member (in the caller's order) with a value of grad_lb that is not finite -> *bad
template <typename REAL>
__global__ void __launch_bounds__(256) k_small_grad_lb_check(const BoundItem<REAL>* __restrict__ items, const REAL* __restrict__ grad_lb, uint32_t* __restrict__ bad)
{
    const BoundItem<REAL>& it = items[blockIdx.x];
    bool b = false;
    for (uint32_t k = threadIdx.x; k < it.n_bdds; k += 256u) b |= !rfinite(grad_lb[(size_t)it.src_b + k]);
    if (b) atomicMin(bad, it.member);
}

// The arg-min path of every BDD of one pack, by its wave (lane `lane` of wave p on pack p < n_packs): the path pass of
// k_small_grad_lb_batch and of k_small_solution_batch (kernels/batchsol.hpp), written once, so that both decide ties alike.  The pass is
// the history step's of small_iterate (kernels/small.hpp), which is FWD_SOLUTION's (kernels/narrow.hpp) out of LDS: a plain forward pass
// over the pack's hops from the costs-to-terminal in memory (valid: BatchT::join_in) and the arc costs, the second-generation resident
// records from the pack's first hop downwards.  Roots start with cost-from-root 0 and on the path; a node on the path decides
// take_lo = ((f + (th + hi)) - (f + (tl + lo))) > 0, writes the decision of its layer and marks the child taken; every node pushes
// f + cost into its children (a push into a sink or from a padding lane goes as +inf into the lane's own entry).  The on-path marks of a
// hop's nodes are 64 entries indexed by the node's slot modulo 64: a hop's slots are consecutive and at most 64.
// The pack's region of the dynamic LDS is bound_region_bytes; a wave reads and writes its own pack's region only: no workgroup barrier.
// Out: the pack's first layer and its number of layers, and `dc`, the LDS byte offset of the pack's decisions — REAL 0 / 1 per layer, 0
// where no node of the layer is on the path, as the memset of the solution buffer leaves it.  Returns false, with nothing in LDS, for a
// pack without a hop.
template <typename REAL>
__device__ __forceinline__ bool bound_path_pass(unsigned char* dyn_lds, const BoundItem<REAL>& it, uint32_t p, uint32_t lane, uint32_t& layer0, uint32_t& nlayers,
                                                uint32_t& dc)
{
    constexpr uint32_t S = sizeof(REAL);
    using P2 = typename Pair<REAL>::type;
    constexpr uint32_t P2S = (uint32_t)sizeof(P2);
    const uint32_t* const hp = it.pack_hdr + 8 * (size_t)p;
    const uint32_t slot0 = hp[0], nslots = hp[1];
    layer0 = hp[2];
    nlayers = hp[3];
    // (wave-uniform by construction; said so, or every record load's scalar offset is wrapped in a loop over its distinct values)
    const uint32_t nh = __builtin_amdgcn_readfirstlane(hp[5] & 0xFFFFu);
    if (nh == 0u) return false;
    const uint32_t rbase = __builtin_amdgcn_readfirstlane(it.rec_off[p]);
    const REAL INF = inf_v<REAL>();
    const uint32_t ns = it.ns;
    const uint32_t wb = p * bound_region_bytes(S, ns, it.nl), wbF = wb + res2_f_off(S, ns), wbC = wb + res2_c_off(S, ns);
    const uint32_t mk = wb + res2_wave_bytes(S, ns, it.nl);
    dc = mk + 64u * S;
    const uint32_t f_end = res2_f_off(S, ns) + ns * S;
    const rsrc_t rr = make_rsrc(it.rec, it.rec_words);
    // ---- the pack's state -> LDS
    for (uint32_t j = lane; j < nslots; j += 64u) lds_st<REAL>(dyn_lds, wb + j * S, it.T[(size_t)slot0 + j]);
    if (lane < 2u) lds_st<REAL>(dyn_lds, wb + (ns + lane) * S, lane == 0u ? REAL(0) : INF);  // sinks: cost to terminal 0 (top) / +inf (bot)
    for (uint32_t o = lane; o < ns + 64u; o += 64u) lds_st<REAL>(dyn_lds, wbF + o * S, INF);    // costs-from-root and the lanes' own entries
    lds_st<REAL>(dyn_lds, mk + lane * S, REAL(0));
    for (uint32_t j = lane; j < nlayers; j += 64u) {
        lds_st<P2>(dyn_lds, wbC + j * P2S, reinterpret_cast<const P2*>(it.lohi)[(size_t)layer0 + j]);
        lds_st<REAL>(dyn_lds, dc + j * S, REAL(0));   // 0 where no node of the layer is on the path, as the memset of the solution buffer leaves it
    }
    wave_sync();
    auto hop = [&](const u4v& r, bool first) {
        const bool real = r[3] != RES2_PAD;
        const uint32_t ll = r[2] & 0xFFFFu, fs = r[2] >> 16;
        const uint32_t own_mark = mk + ((fs / S) & 63u) * S;
        // every node of hop 0 is a root: cost-from-root 0 and on the path (flush_costs_from_root; FWD_SOLUTION's `j == rt`)
        const REAL f = first ? (real ? REAL(0) : INF) : lds_ld<REAL>(dyn_lds, wbF + fs);
        const bool on = real && (first || lds_ld<REAL>(dyn_lds, own_mark) != REAL(0));
        const REAL tl = lds_ld<REAL>(dyn_lds, wb + (r[0] & 0xFFFFu)), th = lds_ld<REAL>(dyn_lds, wb + (r[0] >> 16));
        const P2 cc = lds_ld<P2>(dyn_lds, wbC + ll);
        if (on) lds_st<REAL>(dyn_lds, own_mark, REAL(0));   // (before the marks of the next hop: its slots may have the same index)
        wave_sync();
        // compute_bdd_sol_func as FWD_SOLUTION evaluates it (kernels/narrow.hpp): this parenthesisation, not the solve sweeps'
        const REAL hi_path = f + (th + cc.y);
        const REAL lo_path = f + (tl + cc.x);
        const bool take_lo = (hi_path - lo_path) > 0;
        if (on) {
            lds_st<REAL>(dyn_lds, dc + (ll >> 1), take_lo ? REAL(0) : REAL(1));
            const uint32_t ct = take_lo ? (r[0] & 0xFFFFu) : (r[0] >> 16);   // the child taken: its slot, or a sink's entry
            if (ct < ns * S) lds_st<REAL>(dyn_lds, mk + ((ct / S) & 63u) * S, REAL(1));
        }
        // the pushes; into a sink or from a padding lane: +inf into the lane's own entry
        const uint32_t plo = r[1] & 0xFFFFu, phi = r[1] >> 16;
        const bool blo = plo < f_end, bhi = phi < f_end;   // (a padding lane's two targets are its own entry, past f_end)
        lds_min(reinterpret_cast<REAL*>(dyn_lds + (blo ? wb + plo : wbF + fs)), blo ? f + cc.x : INF);
        lds_min(reinterpret_cast<REAL*>(dyn_lds + (bhi ? wb + phi : wbF + fs)), bhi ? f + cc.y : INF);
        wave_sync();
    };
    // hop k's record requested eight hops ahead; past the last hop: any record (never used)
    auto ldrec = [&](uint32_t k) -> u4v {
        const uint32_t h = k < nh ? k : 0u;
        return __builtin_amdgcn_raw_buffer_load_b128(rr, lane * 16u, (rbase + h * 64u) * 16u, 0);
    };
    u4v r0 = ldrec(0), r1 = ldrec(1), r2 = ldrec(2), r3 = ldrec(3), r4 = ldrec(4), r5 = ldrec(5), r6 = ldrec(6), r7 = ldrec(7);
#define BOUND_HOP(RK, HK)           \
    hop(RK, k + (HK) == 0u);        \
    RK = ldrec(k + (HK) + 8);       \
    if (k + (HK) + 1 >= nh) break;
    for (uint32_t k = 0; k < nh; k += 8) {
        BOUND_HOP(r0, 0) BOUND_HOP(r1, 1) BOUND_HOP(r2, 2) BOUND_HOP(r3, 3) BOUND_HOP(r4, 4) BOUND_HOP(r5, 5) BOUND_HOP(r6, 6) BOUND_HOP(r7, 7)
    }
#undef BOUND_HOP
    return true;
}

// grad_lower_bound_per_bdd (smooth = 0) of every member, wave p on pack p (n_packs <= NW): the path pass above and k_grad_lb's two
// products per layer.  A wave reads and writes its own pack's layers only and fetches grad_lb per layer: the kernel has no workgroup
// barrier.
template <typename REAL, int NW>
__global__ void __launch_bounds__(64 * NW) k_small_grad_lb_batch(const BoundItem<REAL>* __restrict__ items, const REAL* __restrict__ grad_lb, REAL* __restrict__ grad_lo,
                                                                 REAL* __restrict__ grad_hi)
{
    constexpr uint32_t S = sizeof(REAL);
    extern __shared__ __attribute__((aligned(16))) unsigned char dyn_lds[];
    const BoundItem<REAL>& it = items[blockIdx.x];
    const uint32_t tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane((int)(tid >> 6));
    const uint32_t lane = tid & 63u;
    const uint32_t p = (uint32_t)wave;
    if (p >= it.n_packs) return;
    uint32_t layer0, nlayers, dc;
    if (!bound_path_pass<REAL>(dyn_lds, it, p, lane, layer0, nlayers, dc)) return;
    // k_grad_lb (kernels/elementwise.hpp), its two expressions, for the pack's layers
    const REAL* const gm = grad_lb + it.src_b;
    REAL* const olo = grad_lo + (size_t)it.src + layer0;
    REAL* const ohi = grad_hi + (size_t)it.src + layer0;
    for (uint32_t j = lane; j < nlayers; j += 64u) {
        const REAL xl = lds_ld<REAL>(dyn_lds, dc + j * S), gb = gm[it.layer_bdd[(size_t)layer0 + j]];
        ohi[j] = xl * gb;
        olo[j] = (REAL(1) - xl) * gb;
    }
}

// distribute_delta of every member, a workgroup of 256 threads each: the copy of the deferred differences into mm_consumed (what a later
// grad_distribute_delta of the member reads), k_distribute_delta's arithmetic per layer, the zero-fill of the two delta arrays.
template <typename REAL>
__global__ void __launch_bounds__(256) k_small_distribute_batch(const BoundItem<REAL>* __restrict__ items)
{
    const BoundItem<REAL>& it = items[blockIdx.x];
    const uint32_t tid = threadIdx.x;
    for (uint32_t e = tid; e < it.n_layers; e += 256u) it.mm_consumed[e] = it.mm_binned[e];
    __syncthreads();   // (the copy is by entry, the rest by layer)
    for (uint32_t l = tid; l < it.n_layers; l += 256u) {
        const uint32_t e = it.lpos[l];
        const REAL m = it.mm_binned[e];
        if (m > 0) it.lohi[2 * (size_t)l + 1] += m;
        else it.lohi[2 * (size_t)l] -= m;
        it.mm_binned[e] = REAL(0);
    }
    for (uint32_t k = tid; k < 2u * it.n_vars; k += 256u) it.delta_var[k] = REAL(0);
    for (uint32_t k = tid; k < 2u * it.n_layers; k += 256u) it.delta_lay[k] = REAL(0);
}

// The instantiations (defined in solver_bb.hpp, compiled in solver_bb_f32.hip / _f64.hip): the gradient kernel for members of `nw` waves
template <typename REAL>
using BoundGradFn = void (*)(const BoundItem<REAL>*, const REAL*, REAL*, REAL*);
template <typename REAL>
using BoundGetFn = void (*)(const BoundItem<REAL>*, REAL*);
template <typename REAL>
using BoundCheckFn = void (*)(const BoundItem<REAL>*, const REAL*, uint32_t*);
template <typename REAL>
using BoundDistFn = void (*)(const BoundItem<REAL>*);
template <typename REAL>
BoundGradFn<REAL> bound_grad_fn(int nw);
template <typename REAL>
BoundGetFn<REAL> bound_get_fn();
template <typename REAL>
BoundCheckFn<REAL> bound_check_fn();
template <typename REAL>
BoundDistFn<REAL> bound_dist_fn();

}  // namespace bddmma
