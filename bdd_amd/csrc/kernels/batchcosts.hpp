// kernels/batchcosts.hpp — a batch's solver costs in one launch each way (solver_bt.hpp: BatchT::set_solver_costs / get_solver_costs).
// k_small_set_batch: set_solver_costs + backward_run of every member, one workgroup per member; k_small_get_batch: get_solver_costs of
// every member.  Not part of kernels.hpp: the kernels are instantiated in solver_bc_f32.hip / solver_bc_f64.hip only (solver_bc.hpp);
// solver_bt.hpp includes this file for the item and the two getters.
#pragma once

namespace bddmma {

// What a member's workgroup needs, one entry per member of the batch, read-only for the launches: the item's address is uniform, so its
// fields arrive by scalar loads as kernel arguments do (k_iterate_small_batch).  Member i's values start at `src` in each of the
// concatenated arrays (LearnLoad's addressing).
template <typename REAL>
struct CostsItem {
    const uint32_t* pack_hdr;   // layout.hpp: struct Resident — 8 words per pack
    const uint32_t* rec;        // Res2Records
    const uint32_t* rec_off;
    const uint32_t* lpos;       // layer -> its entry in mm_binned
    REAL* T;
    REAL* lohi;
    REAL* mm_binned;
    double* lb_partial;
    uint32_t rec_words;
    uint32_t ns, nl;            // slot / layer capacity the records' offsets were built for
    uint32_t n_packs, lb_base, n_layers;
    uint32_t src;               // first value of the member in the concatenated arrays
};
// A pack's LDS region of k_small_set_batch: [T: (ns + 4) S | {lo, hi}: nl 2 S] — the records' offsets of the costs-to-terminal (the two
// sinks at ns and ns + 1) and of the layer pairs are those of res2_wave_bytes' region without its costs-from-root.
__host__ __device__ inline uint32_t costs_region_bytes(uint32_t real_size, uint32_t ns, uint32_t nl) { return ((ns + 4u) * real_size + nl * 2u * real_size + 15u) & ~15u; }

// (b) of k_small_set_batch for one pack, by its wave: the region's costs-to-terminal at byte `wb` of the dynamic LDS (the two sinks
// filled), its layer pairs at `wbC`; T goes to LDS and to `Tg` (the pack's first slot in the member's array).  Returns the pack's bound
// on lane 0.  Shared with the round kernel of a batch (kernels/batchround.hpp).
template <typename REAL>
__device__ __forceinline__ double costs_backward(unsigned char* dyn_lds, uint32_t wb, uint32_t wbC, const rsrc_t& rr, uint32_t rbase, uint32_t nh, uint32_t lane,
                                                 unsigned char* Tg)
{
    using P2 = typename Pair<REAL>::type;
    auto hop = [&](const u4v& r) {
        const bool real = r[3] != RES2_PAD;   // padding lanes: both children the bot sink, layer 0 of the pack; their result goes nowhere
        const uint32_t ll = r[2] & 0xFFFFu, fs = r[2] >> 16;
        const REAL tl = lds_ld<REAL>(dyn_lds, wb + (r[0] & 0xFFFFu)), th = lds_ld<REAL>(dyn_lds, wb + (r[0] >> 16));
        const P2 cc = lds_ld<P2>(dyn_lds, wbC + ll);
        const REAL t = rmin(th + cc.y, tl + cc.x);
        if (real) {
            lds_st<REAL>(dyn_lds, wb + fs, t);
            *reinterpret_cast<REAL*>(Tg + fs) = t;
        }
        wave_sync();
    };
    // k-th hop processed = hop nh - 1 - k of the pack, its record requested eight hops ahead; past the first hop: any record (never used)
    const uint32_t nhm1 = nh - 1u;
    auto ldrec = [&](uint32_t k) -> u4v {
        const uint32_t h = k < nhm1 ? nhm1 - k : 0u;
        return __builtin_amdgcn_raw_buffer_load_b128(rr, lane * 16u, (rbase + h * 64u) * 16u, 0);
    };
    u4v r0 = ldrec(0), r1 = ldrec(1), r2 = ldrec(2), r3 = ldrec(3), r4 = ldrec(4), r5 = ldrec(5), r6 = ldrec(6), r7 = ldrec(7);
#define COSTS_HOP(RK, HK)           \
    hop(RK);                        \
    RK = ldrec(k + (HK) + 8);       \
    if (k + (HK) + 1 >= nh) break;
    for (uint32_t k = 0; k < nh; k += 8) {
        COSTS_HOP(r0, 0) COSTS_HOP(r1, 1) COSTS_HOP(r2, 2) COSTS_HOP(r3, 3) COSTS_HOP(r4, 4) COSTS_HOP(r5, 5) COSTS_HOP(r6, 6) COSTS_HOP(r7, 7)
    }
#undef COSTS_HOP
    // lower bound contribution of this pack: the double sum of the first hop's roots, small_iterate's tree
    const u4v rroot = __builtin_amdgcn_raw_buffer_load_b128(rr, lane * 16u, rbase * 16u, 0);
    double lb = rroot[3] != RES2_PAD ? (double)lds_ld<REAL>(dyn_lds, wb + (rroot[2] >> 16)) : 0.0;
    for (int off2 = 32; off2 > 0; off2 >>= 1) lb += __shfl_down(lb, off2);
    return lb;
}

// (a) the member's part of lo / hi / mm -> lohi (stride 2) and mm_binned (through lpos): k_strided_copy and k_layers_to_entries for every
//     member at once; a null array is skipped.  No value is checked, as the per-member call checks none.
// (b) a plain backward sweep of the member, wave p on pack p (n_packs <= NW): the pack's costs-to-terminal and its arc costs in LDS, the
//     second-generation resident records from the pack's last hop upwards, t = min(hi + T[hi child], lo + T[lo child]) in BWD_PLAIN's
//     operand order (bwd_narrow_body), T written back for the real lanes, the pack's bound as small_iterate sums it.
// A wave takes its pack's arc costs from the inputs themselves (from lohi where an input is null: this launch does not write those
// then), so (b) does not wait for another wave's part of (a): the kernel has no workgroup barrier.
template <typename REAL, int NW>
__global__ void __launch_bounds__(64 * NW) k_small_set_batch(const CostsItem<REAL>* __restrict__ items, const REAL* __restrict__ lo, const REAL* __restrict__ hi,
                                                             const REAL* __restrict__ mm)
{
    constexpr uint32_t S = sizeof(REAL);
    constexpr uint32_t NT = 64 * NW;
    using P2 = typename Pair<REAL>::type;
    extern __shared__ __attribute__((aligned(16))) unsigned char dyn_lds[];
    const CostsItem<REAL>& it = items[blockIdx.x];
    const uint32_t tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane((int)(tid >> 6));
    const int lane = tid & 63;
    const REAL* const lo_m = lo != nullptr ? lo + it.src : nullptr;
    const REAL* const hi_m = hi != nullptr ? hi + it.src : nullptr;
    const REAL* const mm_m = mm != nullptr ? mm + it.src : nullptr;
    // ---- (a)
    for (uint32_t l = tid; l < it.n_layers; l += NT) {
        if (lo_m != nullptr && hi_m != nullptr) {
            P2 c;
            c.x = lo_m[l];
            c.y = hi_m[l];
            reinterpret_cast<P2*>(it.lohi)[l] = c;
        } else if (lo_m != nullptr) {
            it.lohi[2 * (size_t)l] = lo_m[l];
        } else if (hi_m != nullptr) {
            it.lohi[2 * (size_t)l + 1] = hi_m[l];
        }
        if (mm_m != nullptr) it.mm_binned[it.lpos[l]] = mm_m[l];
    }
    // ---- (b)
    const uint32_t p = (uint32_t)wave;
    if (p >= it.n_packs) return;
    const uint32_t* const hp = it.pack_hdr + 8 * (size_t)p;
    const uint32_t slot0 = hp[0], layer0 = hp[2], nlayers = hp[3];
    // (wave-uniform by construction; said so, or every record load's scalar offset is wrapped in a loop over its distinct values)
    const uint32_t nh = __builtin_amdgcn_readfirstlane(hp[5] & 0xFFFFu);
    if (nh == 0u) return;
    const uint32_t rbase = __builtin_amdgcn_readfirstlane(it.rec_off[p]);
    const uint32_t wb = p * costs_region_bytes(S, it.ns, it.nl), wbC = wb + (it.ns + 4u) * S;
    const rsrc_t rr = make_rsrc(it.rec, it.rec_words);
    for (uint32_t j = (uint32_t)lane; j < nlayers; j += 64u) {
        const size_t l = (size_t)layer0 + j;
        P2 c;
        c.x = lo_m != nullptr ? lo_m[l] : it.lohi[2 * l];
        c.y = hi_m != nullptr ? hi_m[l] : it.lohi[2 * l + 1];
        lds_st<P2>(dyn_lds, wbC + j * (uint32_t)sizeof(P2), c);
    }
    if (lane < 2) lds_st<REAL>(dyn_lds, wb + (it.ns + (uint32_t)lane) * S, lane == 0 ? REAL(0) : inf_v<REAL>());  // sinks: cost to terminal 0 (top) / +inf (bot)
    wave_sync();
    const double lb = costs_backward<REAL>(dyn_lds, wb, wbC, rr, rbase, nh, (uint32_t)lane, reinterpret_cast<unsigned char*>(it.T + slot0));
    if (lane == 0) it.lb_partial[it.lb_base + p] = lb;
}

// The reverse: lohi (stride 2) -> lo and hi, mm_binned[lpos[l]] -> mm[l], into the concatenated outputs; a null output is skipped
// (k_strided_copy / k_entries_to_layers for every member at once).
template <typename REAL>
__global__ void __launch_bounds__(256) k_small_get_batch(const CostsItem<REAL>* __restrict__ items, REAL* __restrict__ lo, REAL* __restrict__ hi, REAL* __restrict__ mm)
{
    using P2 = typename Pair<REAL>::type;
    const CostsItem<REAL>& it = items[blockIdx.x];
    for (uint32_t l = threadIdx.x; l < it.n_layers; l += 256u) {
        if (lo != nullptr || hi != nullptr) {
            const P2 c = reinterpret_cast<const P2*>(it.lohi)[l];
            if (lo != nullptr) lo[(size_t)it.src + l] = c.x;
            if (hi != nullptr) hi[(size_t)it.src + l] = c.y;
        }
        if (mm != nullptr) mm[(size_t)it.src + l] = it.mm_binned[it.lpos[l]];
    }
}

// The instantiations (defined in solver_bc.hpp, compiled in solver_bc_f32.hip / _f64.hip): the set kernel for members of `nw` waves
template <typename REAL>
using CostsSetFn = void (*)(const CostsItem<REAL>*, const REAL*, const REAL*, const REAL*);
template <typename REAL>
using CostsGetFn = void (*)(const CostsItem<REAL>*, REAL*, REAL*, REAL*);
template <typename REAL>
CostsSetFn<REAL> costs_set_fn(int nw);
template <typename REAL>
CostsGetFn<REAL> costs_get_fn();

}  // namespace bddmma
