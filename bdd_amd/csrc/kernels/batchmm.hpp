// kernels/batchmm.hpp — the min-marginal differences of a batch and their gradient, one launch each (solver_bt.hpp:
// BatchT::min_marginal_diff, grad_min_marginal_diff).  k_small_mmdiff_batch: min_marginal_diff of every member; k_small_grad_mm_batch:
// grad_min_marginal_diff of every member; both one workgroup per member, wave p on pack p, no workgroup barrier (packs are independent).
// Not part of kernels.hpp: the kernels are instantiated in solver_bm_f32.hip / solver_bm_f64.hip only (solver_bm.hpp); solver_bt.hpp
// includes this file for the item and the getters.  Behind kernels.hpp.
#pragma once
#include "gradsmall.hpp"   // GsWaveBar; gradmm.hpp's bodies through graditer.hpp

namespace bddmma {

// What a member's workgroup needs, one entry per member of the batch, read-only for the launches (BoundItem's addressing).  Member i's
// values start at `src` in each concatenated layer array.
template <typename REAL>
struct MmItem {
    const uint32_t* pack_hdr;   // layout.hpp: struct Resident — 8 words per pack
    const uint32_t* rec;        // Res2Records
    const uint32_t* rec_off;
    uint32_t rec_words;
    uint32_t ns, nl;            // slot / layer capacity the records' offsets were built for
    uint32_t n_packs, n_layers;
    uint32_t src;
    uint32_t member;            // its index in the caller's order (the items are sorted by wave count)
    uint32_t ww;                // slots of a narrow pack
    DevPtrs<REAL> d;            // T and the arc costs are read, F is written
    PackDev pk;                 // the narrow packs' hop tables
    // the gradient's: null until the batch's first gradient call (SolverT::gr_prepare)
    const uint32_t *par_ptr, *par;   // the narrow words' parent tables (SolverT::sm_prepare)
    uint32_t* arg;                   // the member's d_gr_arg: what the down sweep hands to the up sweep
};
// A pack's LDS region: the region of the second-generation resident records [T: (ns + 4) S | F: (ns + 64) S | {lo, hi}: nl 2 S]
// (res2_wave_bytes); the differences add the two minima per layer [lo: nl S | hi: nl S]; the gradient reuses the region for the arrays of
// its two pull sweeps (gr_lds_bytes of a 64-slot pack), which are live behind the forward phase: the larger of the two, not their sum.
// Both are smaller than the pack's share of small_lds (its region and its staging area of nl pairs), so every fused_small member fits.
__host__ __device__ inline uint32_t mmdiff_region_bytes(uint32_t real_size, uint32_t ns, uint32_t nl)
{
    return (res2_wave_bytes(real_size, ns, nl) + 2u * nl * real_size + 15u) & ~15u;
}
__host__ __device__ inline uint32_t mmgrad_region_bytes(uint32_t real_size, uint32_t ns, uint32_t nl)
{
    const uint32_t fw = res2_wave_bytes(real_size, ns, nl), gr = (uint32_t)gr_lds_bytes(real_size, 64u);
    return ((fw > gr ? fw : gr) + 15u) & ~15u;
}

struct BmPack {
    uint32_t slot0, nslots, layer0, nlayers, nh, rbase;
};
template <typename REAL>
__device__ __forceinline__ BmPack bm_pack(const MmItem<REAL>& it, uint32_t p)
{
    const uint32_t* const hp = it.pack_hdr + 8 * (size_t)p;
    // (wave-uniform by construction; said so, or every record load's scalar offset is wrapped in a loop over its distinct values)
    return {hp[0], hp[1], hp[2], hp[3], (uint32_t)__builtin_amdgcn_readfirstlane(hp[5] & 0xFFFFu), (uint32_t)__builtin_amdgcn_readfirstlane(it.rec_off[p])};
}
// Global memory the wave has written, read back by other lanes of the same wave: the stores have arrived before the loads are issued
__device__ __forceinline__ void bm_memory_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// The costs-from-root of pack `pb` by a plain forward pass out of LDS, the region at byte `wb` of the dynamic LDS: FWD_PLAIN's values
// (kernels/narrow.hpp) with k_small_grad_lb_batch's pass (kernels/batchbound.hpp) — roots (every node of hop 0) start at 0, every node
// pushes f + cost into its children by lds_min, a push into a sink or from a padding lane goes as +inf into the lane's own entry.  The
// costs-to-terminal come from memory (valid: BatchT::join_in).  At the end the pack's F stands in LDS and in the member's own array.
// MINS: the two minima per layer of F + (T_lo + c_lo) and F + (T_hi + c_hi) — BWD_MARGINALS' parenthesisation — at `wb + mins`, nl values each.
template <typename REAL, bool MINS>
__device__ __forceinline__ void bm_forward(unsigned char* dyn_lds, const MmItem<REAL>& it, const BmPack& pb, uint32_t lane, uint32_t wb)
{
    constexpr uint32_t S = sizeof(REAL);
    using P2 = typename Pair<REAL>::type;
    constexpr uint32_t P2S = (uint32_t)sizeof(P2);
    const REAL INF = inf_v<REAL>();
    const uint32_t ns = it.ns;
    const uint32_t wbF = wb + res2_f_off(S, ns), wbC = wb + res2_c_off(S, ns);
    const uint32_t m0 = wb + res2_wave_bytes(S, ns, it.nl), m1 = m0 + it.nl * S;
    const uint32_t f_end = res2_f_off(S, ns) + ns * S;
    const rsrc_t rr = make_rsrc(it.rec, it.rec_words);
    // ---- the pack's state -> LDS
    for (uint32_t j = lane; j < pb.nslots; j += 64u) lds_st<REAL>(dyn_lds, wb + j * S, it.d.T[(size_t)pb.slot0 + j]);
    if (lane < 2u) lds_st<REAL>(dyn_lds, wb + (ns + lane) * S, lane == 0u ? REAL(0) : INF);  // sinks: cost to terminal 0 (top) / +inf (bot)
    for (uint32_t o = lane; o < ns + 64u; o += 64u) lds_st<REAL>(dyn_lds, wbF + o * S, INF);    // costs-from-root and the lanes' own entries
    for (uint32_t j = lane; j < pb.nlayers; j += 64u) {
        lds_st<P2>(dyn_lds, wbC + j * P2S, reinterpret_cast<const P2*>(it.d.lohi)[(size_t)pb.layer0 + j]);
        if constexpr (MINS) {
            lds_st<REAL>(dyn_lds, m0 + j * S, INF);
            lds_st<REAL>(dyn_lds, m1 + j * S, INF);
        }
    }
    wave_sync();
    auto hop = [&](const u4v& r, bool first) {
        const bool real = r[3] != RES2_PAD;
        const uint32_t ll = r[2] & 0xFFFFu, fs = r[2] >> 16;
        // every node of hop 0 is a root: cost-from-root 0 (flush_costs_from_root); below, every parent has pushed by now
        const REAL f = first ? (real ? REAL(0) : INF) : lds_ld<REAL>(dyn_lds, wbF + fs);
        const P2 cc = lds_ld<P2>(dyn_lds, wbC + ll);
        if (first && real) lds_st<REAL>(dyn_lds, wbF + fs, REAL(0));
        if constexpr (MINS) {
            const REAL tl = lds_ld<REAL>(dyn_lds, wb + (r[0] & 0xFFFFu)), th = lds_ld<REAL>(dyn_lds, wb + (r[0] >> 16));
            if (real) {   // (ll is the byte offset of the layer's pair: 2 S per layer)
                lds_min(reinterpret_cast<REAL*>(dyn_lds + m0 + (ll >> 1)), f + (tl + cc.x));
                lds_min(reinterpret_cast<REAL*>(dyn_lds + m1 + (ll >> 1)), f + (th + cc.y));
            }
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
        const uint32_t h = k < pb.nh ? k : 0u;
        return __builtin_amdgcn_raw_buffer_load_b128(rr, lane * 16u, (pb.rbase + h * 64u) * 16u, 0);
    };
    u4v r0 = ldrec(0), r1 = ldrec(1), r2 = ldrec(2), r3 = ldrec(3), r4 = ldrec(4), r5 = ldrec(5), r6 = ldrec(6), r7 = ldrec(7);
#define BM_HOP(RK, HK)              \
    hop(RK, k + (HK) == 0u);        \
    RK = ldrec(k + (HK) + 8);       \
    if (k + (HK) + 1 >= pb.nh) break;
    for (uint32_t k = 0; k < pb.nh; k += 8) {
        BM_HOP(r0, 0) BM_HOP(r1, 1) BM_HOP(r2, 2) BM_HOP(r3, 3) BM_HOP(r4, 4) BM_HOP(r5, 5) BM_HOP(r6, 6) BM_HOP(r7, 7)
    }
#undef BM_HOP
    for (uint32_t j = lane; j < pb.nslots; j += 64u) it.d.F[(size_t)pb.slot0 + j] = lds_ld<REAL>(dyn_lds, wbF + j * S);
}

// out[src + l] = (min over the nodes of l of F + (T_hi + c_hi)) - (... lo ...) for every layer l of every member: SolverT::min_marginal_diff
// (forward_run, the BWD_MARGINALS sweep, k_diff) for every member at once.  Minima are exact in any order, so the values are that path's
// bit for bit; a layer with both sides infinite gives inf - inf, as k_diff does.
template <typename REAL, int NW>
__global__ void __launch_bounds__(64 * NW) k_small_mmdiff_batch(const MmItem<REAL>* __restrict__ items, REAL* __restrict__ out)
{
    constexpr uint32_t S = sizeof(REAL);
    extern __shared__ __attribute__((aligned(16))) unsigned char dyn_lds[];
    const MmItem<REAL>& it = items[blockIdx.x];
    const uint32_t tid = threadIdx.x;
    const uint32_t p = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6)), lane = tid & 63u;
    if (p >= it.n_packs) return;
    const BmPack pb = bm_pack(it, p);
    if (pb.nh == 0u) return;
    const uint32_t wb = p * mmdiff_region_bytes(S, it.ns, it.nl);
    bm_forward<REAL, true>(dyn_lds, it, pb, lane, wb);
    const uint32_t m0 = wb + res2_wave_bytes(S, it.ns, it.nl), m1 = m0 + it.nl * S;
    REAL* const o = out + (size_t)it.src + pb.layer0;
    for (uint32_t j = lane; j < pb.nlayers; j += 64u) o[j] = lds_ld<REAL>(dyn_lds, m1 + j * S) - lds_ld<REAL>(dyn_lds, m0 + j * S);
}

// The argument check of the gradient: the first member (in the caller's order) with a value of grad_mm that is not finite -> *bad
template <typename REAL>
__global__ void __launch_bounds__(256) k_small_grad_mm_check(const MmItem<REAL>* __restrict__ items, const REAL* __restrict__ grad_mm, uint32_t* __restrict__ bad)
{
    const MmItem<REAL>& it = items[blockIdx.x];
    bool b = false;
    for (uint32_t k = threadIdx.x; k < it.n_layers; k += 256u) b |= !rfinite(grad_mm[(size_t)it.src + k]);
    if (b) atomicMin(bad, it.member);
}

// SolverT::gr_min_marginal_diff (forward_run, k_gr_down, k_gr_up; the costs-to-terminal are valid) for every member at once.  The
// forward phase leaves the pack's F in the member's own array, where the two sweeps' bodies (kernels/gradmm.hpp) read it; they run on
// the wave's pack with T = 64 and the wave's ordering point, in the LDS the forward phase has left.  The arg-min slots go from the
// down sweep to the up sweep through the member's d_gr_arg.  The routing steps and the layer folds are the narrow kernels', so the
// values are theirs bit for bit, ties included.
template <typename REAL, int NW>
__global__ void __launch_bounds__(64 * NW) k_small_grad_mm_batch(const MmItem<REAL>* __restrict__ items, const REAL* __restrict__ grad_mm, REAL* __restrict__ grad_lo,
                                                                 REAL* __restrict__ grad_hi)
{
    constexpr uint32_t S = sizeof(REAL);
    extern __shared__ __attribute__((aligned(16))) unsigned char dyn_lds[];
    const MmItem<REAL>& it = items[blockIdx.x];
    const uint32_t tid = threadIdx.x;
    const uint32_t p = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6)), lane = tid & 63u;
    if (p >= it.n_packs) return;
    const BmPack pb = bm_pack(it, p);
    if (pb.nh == 0u) return;
    const uint32_t wb = p * mmgrad_region_bytes(S, it.ns, it.nl);
    bm_forward<REAL, false>(dyn_lds, it, pb, lane, wb);
    bm_memory_sync();   // F is in memory; the forward's LDS is dead
    const PackDev& pk = it.pk;
    const uint32_t q0 = pk.pack_hop_ptr[p];
    const PullPack<REAL> pc{reinterpret_cast<REAL*>(dyn_lds + wb), q0, pk.pack_hop_ptr[p + 1], pk.pack_word_off[p] - pk.hop_node_off[q0], it.ww, lane, 64u};
    const REAL* const g = grad_mm + it.src;
    REAL *const lo = grad_lo + it.src, *const hi = grad_hi + it.src;
    gr_down_body<REAL, true, GsWaveBar>(it.d, pk, pc, it.par_ptr, it.par, it.ww, g, lo, hi, it.arg);
    bm_memory_sync();   // the arg-min slots and the down sweep's part of the outputs
    gr_up_body<REAL, true, GsWaveBar>(it.d, pk, pc, it.par_ptr, it.par, it.ww, g, lo, hi, it.arg);
}

// The instantiations (defined in solver_bm.hpp, compiled in solver_bm_f32.hip / _f64.hip): the kernels for members of `nw` waves
template <typename REAL>
using MmDiffFn = void (*)(const MmItem<REAL>*, REAL*);
template <typename REAL>
using MmGradFn = void (*)(const MmItem<REAL>*, const REAL*, REAL*, REAL*);
template <typename REAL>
using MmCheckFn = void (*)(const MmItem<REAL>*, const REAL*, uint32_t*);
template <typename REAL>
MmDiffFn<REAL> mm_diff_fn(int nw);
template <typename REAL>
MmGradFn<REAL> mm_grad_fn(int nw);
template <typename REAL>
MmCheckFn<REAL> mm_check_fn();

}  // namespace bddmma
