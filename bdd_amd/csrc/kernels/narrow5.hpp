// kernels/narrow5.hpp — narrow packs, solve sweeps of iteration() with a lane per BDD: the on-chip sweeps of kernels/narrow4.hpp with both
// walks in registers (k_fwd_narrow5 / k_bwd_narrow5).  Part of kernels.hpp (include that, not this file: the parts build on each other in
// its order).
#pragma once

namespace bddmma {

// =============================================================================================
// narrow packs, on-chip solve sweeps whose walks stay in one lane's registers (round 23)
// =============================================================================================
// k_fwd_narrow4 / k_bwd_narrow4 route a hop's potentials through per-hop LDS buffers by the records' offsets: gathers of the four children's
// costs-from-terminal, scatters of the layer's own, lds_min pushes into the next frontier, two wave_sync() per hop — a serial chain of LDS
// round trips, ten hops long, twice per sweep.  In a LANE-AFFINE structure template (layout.hpp: LaneCodes; packs whose BDDs are ordered
// longest first, i.e. every pack the default order builds from rows) that routing is the identity: every arc of the lane's layer ends at
// node a or b of the lane's own layer one hop down or at the lane's own TOP / BOT entry.  These kernels therefore keep (ta, tb) and (fa, fb)
// of the lane's layer in registers and select each child's value by a two-bit code {A, B, TOP, BOT} from {ta', tb', 0, +inf}; the codes and
// the two flag bits of all hops arrive in ONE 16-byte load per lane before the walks (10 bits per hop, LCODE_HOPS = 12 hops).  No hop
// buffers, no per-hop record loads, no wave_sync() inside the walks, no F or T traffic; the lane touches LDS at its own staging slot alone
// (the window of hop offsets aside).  Prologue, staging and flush are narrow4's, called as they are.
//   forward:  upward walk, hops hops - 1 .. 1 — (ta, tb) = rmin(c.y + th, c.x + tl) per node into T[h], c = L[h]; then fwd_narrow4_body's hop
//             arithmetic with the children's T selected again from T[h + 1] (two registers per hop where G[h] took four), the next frontier
//             pair as the minimum, from +inf, of those of fa + nc.x, fa + nc.y, fb + nc.x, fb + nc.y whose code names that node;
//   backward: downward walk of f + c into F[h] (masked by the hop's flags, as bwd_narrow4_body masks on use), then its hop arithmetic with
//             (ta', tb') of the hop below carried in registers; lb_partial from hop 0's ta in the same double sum and shuffle tree.
// Why the bits cannot differ from narrow4's:
//   - gathers and scatters move values unchanged, and so do the selects: code A / B names exactly the entry the record's offset named (the
//     predicate of build_lane_codes), TOP / BOT the constants 0 / +inf that the sink entries held; every addition has the operands and
//     order it had, rmin is the same instruction on the same operands;
//   - the frontier: narrow4 formed an entry as ds_min_f32 pushes onto +inf in the order a.lo, a.hi, b.lo, b.hi, here it is v_min_f32 in that
//     order.  The two instructions differ on signed zeros (ds_min keeps the entry unless the pushed value compares less, so the zero
//     pushed first stays; v_min orders -0 below +0) and agree elsewhere.  No frontier value is -0: the roots are +0, a sum x + y is -0
//     only if both operands are, so by induction over the hops no pushed fa + c is, in either kernel;
//   - NaN: a blocked arc is c = +inf, and inf - inf arises only in mm_diff1's product, which the same select discards in both kernels.  A
//     pushed NaN (fa = +inf on a cost of -inf) is dropped by both forms of the minimum: ds_min's compare fails, fminf returns the other
//     operand, and the entry started from +inf, never NaN (tests/test_gpu_lane_sweeps.py: blocked arcs against the twin);
//   - pushes to the sink entries and from idle lanes went to dummy entries nobody read; here they are not formed.  An entry nobody pushed
//     to stayed +inf; so does a minimum over no candidate;
//   - lanes without a layer compute on +inf and on whatever {lo, hi} their load returned, as in narrow4; nothing selects their values (the
//     predicate: A / B only where the lane has that node one hop down) and their stores are dropped by the same flags and descriptors;
//   - the bound: hop 0 holds one-node layers at slots 0 .. n0 - 1 and nothing else (the predicate), so the slot-order sum of narrow4 adds
//     lane l's ta for l < n0, the second half of its loop adds nothing, and the shuffle tree is the same.
// Registers: L[HC] and T[HC] / F[HC] pairs, four code words, the staging tables' 20 and the hop's working set — 88 VGPRs at 10 hops, 96 at 12,
// both directions: five waves per SIMD (narrow4: 114 / 94 and 126 / 118, four); capped at six waves (80 VGPRs) the first version spilled
// 104-156 B per lane, not pursued.  3 KB of static LDS at four packs (the hop window; narrow4: 19 456 / 11 264 B), so LDS holds the staging
// area alone.  No scratch in any instantiation (profiles/r23_lane_sweeps/resources.txt).
// BDDMMA_N5_WAVES: least waves per SIMD the 10-hop pair is compiled for (A/B builds, tools/build_variant.sh).
#ifndef BDDMMA_N5_WAVES
#define BDDMMA_N5_WAVES 5
#endif
constexpr int n5_waves(int hc) { return hc <= 10 ? BDDMMA_N5_WAVES : 4; }

// the 10 bits of hop h: codes of a.lo, a.hi, b.lo, b.hi from bit 0 up, then LREC_TWO, LREC_REAL (h is a constant after unrolling)
__device__ __forceinline__ uint32_t lane_hop_code(const u4v& cw, int h) { return (cw[h / 3] >> (10 * (h % 3))) & 0x3FFu; }
// The code words again, opaque to the compiler: between the walks.  Otherwise it keeps the first walk's extracted bits and masks of every
// hop alive for the second one (76 B of scratch per lane in the 10-hop forward kernel, 128 VGPRs in the 12-hop one).
__device__ __forceinline__ u4v lane_codes_again(const u4v& cw)
{
    uint32_t a = cw[0], b = cw[1], c = cw[2], e = cw[3];
    asm volatile("" : "+v"(a), "+v"(b), "+v"(c), "+v"(e));
    return u4v{a, b, c, e};
}
// Selects by bit masks (0 / ~0 from a sign-extending bit-field extract of the code): a value's bits pass unchanged.  The selects are what a
// hop costs now — about 60 of its 100 VALU instructions (NOTES round 23).
__device__ __forceinline__ uint32_t lane_bit(uint32_t code, uint32_t bit) { return (uint32_t)__builtin_amdgcn_sbfe((int)code, bit, 1u); }
__device__ __forceinline__ float lane_pick(uint32_t m, float a, float b)  // m ? a : b, all bits of m alike
{
    return __builtin_bit_cast(float, (m & __builtin_bit_cast(uint32_t, a)) | (~m & __builtin_bit_cast(uint32_t, b)));
}
// the child's cost-to-terminal its code (bits k, k + 1 of `code`) names: node a / b of the lane's layer one hop down, 0 at TOP, +inf at BOT
__device__ __forceinline__ float lane_child(uint32_t code, uint32_t k, float ta, float tb)
{
    const uint32_t odd = lane_bit(code, k), snk = lane_bit(code, k + 1);
    const float node = lane_pick(odd, tb, ta);
    const float sink = __builtin_bit_cast(float, odd & 0x7F800000u);  // BOT: +inf, TOP: 0
    return lane_pick(snk, sink, node);
}
// the next frontier pair: per node the pushes that name it (LCODE_A / LCODE_B), in narrow4's order, onto +inf
__device__ __forceinline__ void lane_push(float& fa, float& fb, uint32_t code, float p0, float p1, float p2, float p3)
{
    const float INF = inf_v<float>();
    const float pv[4] = {p0, p1, p2, p3};
    fa = fb = INF;
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) {
        const uint32_t odd = lane_bit(code, 2 * k), snk = lane_bit(code, 2 * k + 1);
        fa = rmin(fa, lane_pick(odd | snk, INF, pv[k]));   // code A = 0
        fb = rmin(fb, lane_pick(odd & ~snk, pv[k], INF));  // code B = 1
    }
}

template <typename REAL, int WPB, int HC>
__device__ __forceinline__ void fwd_narrow5_body(const DevPtrs<REAL>& d, const PackDev& pk, const uint32_t* __restrict__ lcode,
                                                 const uint32_t* __restrict__ lcode_off, uint32_t lcode_words, REAL omega, uint32_t block_id)
{
    static_assert(HC + 1 <= (int)HOP_WIN, "one window of hop offsets has to hold the pack");
    static_assert(HC <= (int)LCODE_HOPS, "a lane's code words hold LCODE_HOPS hops");
    using P2 = typename Pair<REAL>::type;
    extern __shared__ __attribute__((aligned(16))) unsigned char dyn_lds[];
    P2* sD = reinterpret_cast<P2*>(dyn_lds);
    __shared__ uint32_t sOffN_[WPB][HOP_WIN], sOffL_[WPB][HOP_WIN], sOffR_[WPB][HOP_WIN];
    const uint32_t tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane((int)(tid >> 6));
    const int lane = tid & 63;
    const uint32_t n_quads = (pk.n_packs + WPB - 1) / WPB;
    const uint32_t quad = block_to_pack(block_id, n_quads, pk.xcd_chunk);
    BDDMMA_EXIT_IF(quad >= n_quads, d)
    const uint32_t p = quad * WPB + wave;
    const bool has_pack = p < pk.n_packs;
    const uint32_t* const hp = pk.hdr_pack + 8 * (size_t)(has_pack ? p : 0);  // resident headers: the rule of SolverT::onchip_hc
    const uint32_t q0 = !has_pack ? 0 : hp[4];
    const uint32_t hops = !has_pack ? 0 : (hp[5] & 0xFFFFu);  // <= HC
    const uint32_t q1 = q0 + hops;
    const uint32_t cbase = has_pack ? lcode_off[p] : 0;
    const uint32_t c0_h = pk.hdr_quad[4 * (size_t)quad], cnt = pk.hdr_quad[4 * (size_t)quad + 1];
    BDDMMA_STAMP(p, 0);
    const REAL INF = inf_v<REAL>();
    const uint32_t slot_first = !has_pack ? 0 : hp[0], l0 = !has_pack ? 0 : hp[2];
    NarrowRs<REAL> rs(d);
    rs.rebase_layers(d, l0);
    uint32_t ent[STAGE_ITERS], esl[STAGE_ITERS];
    stage_load_tables<REAL, WPB, BDDMMA_LD_TAB_AUX>(ent, esl, rs, c0_h, cnt, tid);  // on their way while the costs-to-terminal are rebuilt
    const REAL* const lohi_p = d.lohi + 2 * (size_t)l0;
    const rsrc_t rc = make_rsrc(lcode, lcode_words);
    HopWindow hw{sOffN_[wave], sOffL_[wave], sOffR_[wave], q0, q1, slot_first, l0};
    // A wave without a pack (the last workgroup's) runs the same straight line on hops = 0 — a window of record 0, loads past their
    // descriptors, no hop: with the walks under `if (has_pack)` the compiler kept lb[] in vector registers behind the merge (11 VGPRs) and
    // wrapped every hop's store in a loop over the descriptor's values.
    uint32_t lb[HC + 1];  // first layer of hops 0 .. HC
    P2 L[HC];             // {lo, hi} of the lane's layer in every hop
    P2 T[HC + 1];         // costs-to-terminal (ta, tb) of the lane's layer in hops 1 .. HC - 1 ([HC]: no hop, never selected)
#pragma unroll
    for (int i = 0; i < HC + 1; ++i) T[i] = P2{REAL(0), REAL(0)};
    const uint32_t db = (uint32_t)wave * pk.stage_cap * (uint32_t)sizeof(P2);  // this wave's slots of the staging area
    hw.fill(pk, q0, lane);
#pragma unroll
    for (int i = 0; i < HC + 1; ++i) lb[i] = hw.layer_off(q0 + i);
    // every hop's arc costs at once (hops the pack does not have: past the descriptor, no traffic), and the lane's codes
#pragma unroll
    for (int h = 0; h < HC; ++h)
        hop_load(L[h], rs.lohi, (uint32_t)h < hops ? (uint32_t)lane * (uint32_t)sizeof(P2) : OOB, lb[h] * (uint32_t)sizeof(P2));
    u4v cw = __builtin_amdgcn_raw_buffer_load_b128(rc, (uint32_t)lane * 16u, cbase * 16u, 0);
    {
        // ---- upward walk: (ta, tb) of hops hops - 1 .. 1 (hop 0's own T is not read by a forward sweep)
        REAL ta = REAL(0), tb = REAL(0);
#pragma unroll
        for (int h = HC - 1; h >= 1; --h) {
            if ((uint32_t)h < hops) {  // uniform
                const uint32_t code = lane_hop_code(cw, h);
                const REAL tla = lane_child(code, 0, ta, tb), tha = lane_child(code, 2, ta, tb);
                const REAL tlb = lane_child(code, 4, ta, tb), thb = lane_child(code, 6, ta, tb);
                const P2 c = L[h];
                ta = rmin(c.y + tha, c.x + tla);
                tb = rmin(c.y + thb, c.x + tlb);
                T[h] = P2{ta, tb};
            }
        }
        BDDMMA_STAMP(p, 5);
    }
    cw = lane_codes_again(cw);
    stage_load_pairs<REAL, WPB>(sD, ent, esl, rs, cnt, tid);
    if (WPB > 1) __syncthreads(); else wave_sync();
    BDDMMA_STAMP(p, 1);
    // ---- downward walk: fwd_narrow4_body's hop
    REAL fa = (lane_hop_code(cw, 0) & (LREC_REAL << 8)) ? REAL(0) : INF, fb = INF;  // every slot of hop 0 is a root (flush_costs_from_root)
#pragma unroll
    for (int h = 0; h < HC; ++h) {
        if ((uint32_t)h < hops) {  // uniform
            const uint32_t code = lane_hop_code(cw, h), flags = code >> 8;
            const uint32_t lbh = lb[h], lbn = lb[h + 1];
            const uint32_t stg = db + (lbh + (uint32_t)lane) * (uint32_t)sizeof(P2);  // the lane's layer inside the wave's staging slots
            const P2 c = L[h];
            const P2 tn = T[h + 1];
            const REAL tla = lane_child(code, 0, tn.x, tn.y), tha = lane_child(code, 2, tn.x, tn.y);
            const REAL tlb = lane_child(code, 4, tn.x, tn.y), thb = lane_child(code, 6, tn.x, tn.y);
            const P2 dd = lds_ld<P2>(dyn_lds, stg);
            // ---- arithmetic: the layer's two candidates per side, their minimum, the deferred difference, the new arc costs
            // (narrow4 masks fa / fb by the hop's flags here: a no-op for these packs — a code names A only where the lane has a layer one hop
            // down and B only where that layer has two nodes, so an absent node's entry is the minimum over no candidate, +inf)
            const REAL m0 = rmin((fa + c.x) + tla, (fb + c.x) + tlb);
            const REAL m1 = rmin((fa + c.y) + tha, (fb + c.y) + thb);
            const REAL mm = mm_diff1(m0, m1, omega);
            P2 nc;
            nc.x = (c.x + min0(mm)) + dd.x;
            nc.y = (c.y + min0_neg(mm)) + dd.y;
            // ---- writes: new arc costs, staged difference; the next frontier pair
            const rsrc_t rl = hop_rsrc(reinterpret_cast<const P2*>(lohi_p), lbh, lbn - lbh);  // ends with the hop's layers: idle lanes are dropped
            hop_store(nc, rl, (uint32_t)lane * (uint32_t)sizeof(P2), lbh * (uint32_t)sizeof(P2));
            if (flags & LREC_REAL) lds_st<REAL>(dyn_lds, stg, mm);
            const REAL p0 = fa + nc.x, p1 = fa + nc.y, p2 = fb + nc.x, p3 = fb + nc.y;
            lane_push(fa, fb, code, p0, p1, p2, p3);
        }
    }
    BDDMMA_STAMP(p, 3);
    if (WPB > 1) __syncthreads(); else wave_sync();
    BDDMMA_STAMP(p, 2);
    stage_flush<REAL, WPB>(sD, ent, esl, rs, cnt, tid);  // min-marginal differences of the round -> entry array
    BDDMMA_STAMP(p, 4);
}

template <typename REAL, int WPB, int HC>
__global__ void __launch_bounds__(64 * WPB) __attribute__((amdgpu_waves_per_eu(n5_waves(HC)))) k_fwd_narrow5(DevPtrs<REAL> d, PackDev pk, const uint32_t* __restrict__ lcode, const uint32_t* __restrict__ lcode_off,
                                                          uint32_t lcode_words, REAL omega)
{
    fwd_narrow5_body<REAL, WPB, HC>(d, pk, lcode, lcode_off, lcode_words, omega, blockIdx.x);
}

template <typename REAL, int WPB, int HC>
__device__ __forceinline__ void bwd_narrow5_body(const DevPtrs<REAL>& d, const PackDev& pk, const uint32_t* __restrict__ lcode,
                                                 const uint32_t* __restrict__ lcode_off, uint32_t lcode_words, REAL omega, uint32_t block_id)
{
    static_assert(HC + 1 <= (int)HOP_WIN, "one window of hop offsets has to hold the pack");
    static_assert(HC <= (int)LCODE_HOPS, "a lane's code words hold LCODE_HOPS hops");
    using P2 = typename Pair<REAL>::type;
    extern __shared__ __attribute__((aligned(16))) unsigned char dyn_lds[];
    P2* sD = reinterpret_cast<P2*>(dyn_lds);
    __shared__ uint32_t sOffN_[WPB][HOP_WIN], sOffL_[WPB][HOP_WIN], sOffR_[WPB][HOP_WIN];
    const uint32_t tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane((int)(tid >> 6));
    const int lane = tid & 63;
    const uint32_t n_quads = (pk.n_packs + WPB - 1) / WPB;
    const uint32_t quad = block_to_pack(block_id, n_quads, pk.xcd_chunk);
    BDDMMA_EXIT_IF(quad >= n_quads, d)
    const uint32_t p = quad * WPB + wave;
    const bool has_pack = p < pk.n_packs;
    const uint32_t* const hp = pk.hdr_pack + 8 * (size_t)(has_pack ? p : 0);  // resident headers, see fwd_narrow4_body
    const uint32_t q0 = !has_pack ? 0 : hp[4];
    const uint32_t hops = !has_pack ? 0 : (hp[5] & 0xFFFFu);  // <= HC
    const uint32_t q1 = q0 + hops;
    const uint32_t cbase = has_pack ? lcode_off[p] : 0;
    const uint32_t c0_h = pk.hdr_quad[4 * (size_t)quad], cnt = pk.hdr_quad[4 * (size_t)quad + 1];
    BDDMMA_STAMP(p, 0);
    const REAL INF = inf_v<REAL>();
    const uint32_t slot_first = !has_pack ? 0 : hp[0], l0 = !has_pack ? 0 : hp[2];
    NarrowRs<REAL> rs(d);
    rs.rebase_layers(d, l0);
    uint32_t ent[STAGE_ITERS], esl[STAGE_ITERS];
    stage_load_tables<REAL, WPB, BDDMMA_LD_TAB_AUX>(ent, esl, rs, c0_h, cnt, tid);
    const REAL* const lohi_p = d.lohi + 2 * (size_t)l0;
    const rsrc_t rc = make_rsrc(lcode, lcode_words);
    HopWindow hw{sOffN_[wave], sOffL_[wave], sOffR_[wave], q0, q1, slot_first, l0};
    uint32_t lb[HC + 1];  // first layer of hops 0 .. HC
    P2 L[HC];             // {lo, hi} of the lane's layer in every hop
    P2 F[HC];             // costs-from-root of the lane's layer (nodes a, b) in hops 1 .. HC - 1, +inf where the layer has no such node ([0]: unused,
                          // hop 0's are the roots' constants)
#pragma unroll
    for (int i = 0; i < HC; ++i) F[i] = P2{INF, INF};
    const uint32_t db = (uint32_t)wave * pk.stage_cap * (uint32_t)sizeof(P2);
    hw.fill(pk, q0, lane);  // (waves without a pack too, on hops = 0: see fwd_narrow5_body)
#pragma unroll
    for (int i = 0; i < HC + 1; ++i) lb[i] = hw.layer_off(q0 + i);
#pragma unroll
    for (int h = 0; h < HC; ++h)
        hop_load(L[h], rs.lohi, (uint32_t)h < hops ? (uint32_t)lane * (uint32_t)sizeof(P2) : OOB, lb[h] * (uint32_t)sizeof(P2));
    u4v cw = __builtin_amdgcn_raw_buffer_load_b128(rc, (uint32_t)lane * 16u, cbase * 16u, 0);
    {
        // ---- downward walk: the frontier of every hop, from 0 at the roots (every slot of hop 0 is one)
        REAL fa = (lane_hop_code(cw, 0) & (LREC_REAL << 8)) ? REAL(0) : INF, fb = INF;
#pragma unroll
        for (int h = 0; h < HC; ++h) {
            if ((uint32_t)h < hops) {  // uniform
                const uint32_t code = lane_hop_code(cw, h);
                if (h >= 1) F[h] = P2{fa, fb};  // (an absent node's is +inf already, see fwd_narrow5_body)
                if ((uint32_t)h + 1 < hops) {  // uniform
                    const P2 c = L[h];
                    const REAL p0 = fa + c.x, p1 = fa + c.y, p2 = fb + c.x, p3 = fb + c.y;
                    lane_push(fa, fb, code, p0, p1, p2, p3);
                }
            }
        }
        BDDMMA_STAMP(p, 5);
    }
    cw = lane_codes_again(cw);
    stage_load_pairs<REAL, WPB>(sD, ent, esl, rs, cnt, tid);
    if (WPB > 1) __syncthreads(); else wave_sync();
    BDDMMA_STAMP(p, 1);
    // ---- upward walk: bwd_narrow4_body's hop
    REAL ta = REAL(0), tb = REAL(0);  // of the lane's layer one hop down
#pragma unroll
    for (int h = HC - 1; h >= 0; --h) {
        if ((uint32_t)h < hops) {  // uniform
            const uint32_t code = lane_hop_code(cw, h), flags = code >> 8;
            const uint32_t lbh = lb[h], lbn = lb[h + 1];
            const uint32_t stg = db + (lbh + (uint32_t)lane) * (uint32_t)sizeof(P2);
            const P2 c = L[h];
            const REAL tla = lane_child(code, 0, ta, tb), tha = lane_child(code, 2, ta, tb);
            const REAL tlb = lane_child(code, 4, ta, tb), thb = lane_child(code, 6, ta, tb);
            const P2 dd = lds_ld<P2>(dyn_lds, stg);
            // ---- arithmetic
            const REAL fa = h >= 1 ? F[h].x : (flags & LREC_REAL) ? REAL(0) : INF;  // hop 0: one-node layers, every one a root
            const REAL fb = h >= 1 ? F[h].y : INF;
            const REAL m0 = rmin((fa + c.x) + tla, (fb + c.x) + tlb);
            const REAL m1 = rmin((fa + c.y) + tha, (fb + c.y) + thb);
            const REAL mm = mm_diff1(m0, m1, omega);
            P2 nc;
            nc.x = (c.x + min0(mm)) + dd.x;
            nc.y = (c.y + min0_neg(mm)) + dd.y;
            ta = rmin(nc.y + tha, nc.x + tla);
            tb = rmin(nc.y + thb, nc.x + tlb);
            // ---- writes
            const rsrc_t rl = hop_rsrc(reinterpret_cast<const P2*>(lohi_p), lbh, lbn - lbh);
            hop_store(nc, rl, (uint32_t)lane * (uint32_t)sizeof(P2), lbh * (uint32_t)sizeof(P2));
            if (flags & LREC_REAL) lds_st<REAL>(dyn_lds, stg, mm);
        }
    }
    BDDMMA_STAMP(p, 3);
    if (WPB > 1) __syncthreads(); else wave_sync();
    BDDMMA_STAMP(p, 2);
    stage_flush<REAL, WPB>(sD, ent, esl, rs, cnt, tid);
    BDDMMA_STAMP(p, 4);
    if (!has_pack) return;
    // lower bound contribution of this pack: sum of root costs-from-terminal (bdd_cuda_base.cu:1243-1251); hop 0's slots are its n0 one-node
    // layers, slot l in lane l
    const uint32_t n0 = lb[1] - lb[0];
    double s = 0.0;
    if ((uint32_t)lane < n0) s += (double)ta;
    for (int off2 = 32; off2 > 0; off2 >>= 1) s += __shfl_down(s, off2);
    if (lane == 0) d.lb_partial[pk.lb_base + p] = s;
}

template <typename REAL, int WPB, int HC>
__global__ void __launch_bounds__(64 * WPB) __attribute__((amdgpu_waves_per_eu(n5_waves(HC)))) k_bwd_narrow5(DevPtrs<REAL> d, PackDev pk, const uint32_t* __restrict__ lcode, const uint32_t* __restrict__ lcode_off,
                                                          uint32_t lcode_words, REAL omega)
{
    bwd_narrow5_body<REAL, WPB, HC>(d, pk, lcode, lcode_off, lcode_words, omega, blockIdx.x);
}

}  // namespace bddmma
