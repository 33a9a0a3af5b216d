// kernels/narrow4.hpp — narrow packs, streaming solve sweeps of iteration(): the third generation's hop with the potentials kept on chip
// (k_fwd_narrow4 / k_bwd_narrow4).  Part of kernels.hpp (include that, not this file: the parts build on each other in its order).
#pragma once

namespace bddmma {

// =============================================================================================
// narrow packs, streaming solve sweeps with F and T rebuilt in registers (round 10)
// =============================================================================================
// Inside the iteration loop the costs-to-terminal a forward solve sweep reads are a function of the {lo, hi} it loads anyway: the backward
// sweep computed them as rmin(nc.y + th, nc.x + tl) from exactly the nc it stored, and the exchange in between writes delta_lay only.  Likewise
// the costs-from-root a backward sweep reads are the running minimum of f + nc over the {lo, hi} the forward sweep stored, from 0 at the
// roots.  Additions and minima only, nothing to contract: both are rebuilt here bit for bit, and the 2 x 42 MB (10.5 M nodes, float) that each
// sweep moved for them stay on chip.
// A pack of at most HC hops keeps the {lo, hi} of the lane's layer of EVERY hop in registers (L[HC], all loads issued at once behind the
// header reads: they do not depend on the staging tables) and walks its records twice:
//   forward:  upward first, hops hops - 1 .. 0 — the four children's entries {lo a, hi a, lo b, hi b} of the lane's layer gathered from the
//             sT buffer of hop h + 1 and KEPT, G[h]; for h >= 1 (ta, tb) of the layer formed from them and scattered into the other sT
//             buffer.  Hop 0 only gathers: its children are hop 1's nodes, and nothing reads a T of hop 0 in a forward sweep.  Then
//             k_fwd_narrow3's hop with c = L[h] and the children's T from G[h]: no LDS traffic for T in the second walk (round 14; before, T
//             was read back in slot form into T[h], copied into the buffers again hop by hop and gathered a second time);
//   backward: downward first — pushes of f + c with lds_min into alternating frontier buffers, the lane's (fa, fb) into F[h] — then
//             k_bwd_narrow3's hop with F[h] in place of the loaded pair.  The frontier buffers ARE the sT buffers (the phases do not overlap;
//             the sink constants are written after the first walk, whose pushes use the same entries as dummy targets).
// The records are read again in the second walk (shared by a family's packs: L2 hits), two hops ahead of their use as in narrow3.
// Same arithmetic in the same order as fwd_ / bwd_narrow3_body.  Packs with resident headers only (one stage group per pack, one staging
// round per quad), <= HC hops, so one window of hop offsets serves the pack; float (the double form spills).  REBUILD_* = false loads that
// potential from memory as before, STORE_* = false leaves it unwritten: <1, 0> / <1, 0> is the pair iteration() runs on packs of <= 10 hops (HC = 10) and of 11-12 hops (HC = 12).
// G[h] cannot differ from what the second walk used to gather: that walk read buffer (h + 1) & 1 through the record's offsets ra[0], ra[1],
// and the buffer had been refilled with exactly the values the upward walk had computed into buffer (h + 1) & 1 and read there through the
// same offsets; the sink entries and the dummy entries of idle lanes hold the same constants in both walks; additions and minima are untouched.
// The forward form holds L and G of every hop next to the hop's working set: 114 VGPRs at 10 hops (<1, 0> and <1, 1>, 4 and 8 packs; 90 with T
// loaded, <0, 0>), no scratch.  G takes 4 registers per hop where T[] took 2, but the read-back and re-scatter registers are gone: 12 hops
// compile to 126 VGPRs without scratch (T[]: 24 spilled) and are the second capacity of the <1, 0> pair; 14 hops (40 B of scratch) and 16 still
// spill within the 128 of four waves per SIMD.  The backward form fits at 16 (118).  Packs of 13-16 hops therefore keep k_fwd_narrow3 and
// run k_bwd_narrow4 <1, 1>: F on chip, T through memory.  The other pairs exist for the decomposition of NOTES round 10 (variant_flags bits 22, 23).
// The sT buffers are dead in the forward form's second walk; sF is not aliased onto them: the registers hold the kernel at four waves per
// SIMD whatever the LDS says, and the alias would add an ordering hazard around the roots' initialisation.
template <typename REAL, int WPB, int HC, bool REBUILD_T, bool STORE_F>
__device__ __forceinline__ void fwd_narrow4_body(const DevPtrs<REAL>& d, const PackDev& pk, const uint32_t* __restrict__ lrec,
                                                 const uint32_t* __restrict__ lrec_off, uint32_t lrec_words, REAL omega, uint32_t block_id)
{
    static_assert(HC + 1 <= (int)HOP_WIN, "one window of hop offsets has to hold the pack");
    constexpr int W = N3_W;
    constexpr uint32_t S = sizeof(REAL);
    constexpr uint32_t BUF = (W + 128) * S;  // one hop buffer
    using P2 = typename Pair<REAL>::type;
    extern __shared__ __attribute__((aligned(16))) unsigned char dyn_lds[];
    P2* sD = reinterpret_cast<P2*>(dyn_lds);
    __shared__ __attribute__((aligned(16))) unsigned char sF_[WPB][2][BUF];  // frontier of hop h in buffer h & 1
    __shared__ __attribute__((aligned(16))) unsigned char sT_[WPB][2][BUF];  // costs-from-terminal of hop h in buffer h & 1
    __shared__ uint32_t sOffN_[WPB][HOP_WIN], sOffL_[WPB][HOP_WIN], sOffR_[WPB][HOP_WIN];
    const uint32_t tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane((int)(tid >> 6));
    const int lane = tid & 63;
    unsigned char* sFw = &sF_[wave][0][0];
    unsigned char* sTw = &sT_[wave][0][0];
    const uint32_t n_quads = (pk.n_packs + WPB - 1) / WPB;
    const uint32_t quad = block_to_pack(block_id, n_quads, pk.xcd_chunk);
    BDDMMA_EXIT_IF(quad >= n_quads, d)
    const uint32_t p = quad * WPB + wave;
    const bool has_pack = p < pk.n_packs;
    const uint32_t* const hp = pk.hdr_pack + 8 * (size_t)(has_pack ? p : 0);  // resident headers: the rule of SolverT::onchip_hc
    const uint32_t q0 = !has_pack ? 0 : hp[4];
    const uint32_t hops = !has_pack ? 0 : (hp[5] & 0xFFFFu);  // <= HC
    const uint32_t q1 = q0 + hops;
    const uint32_t rbase = has_pack ? lrec_off[p] : 0;
    const uint32_t c0_h = pk.hdr_quad[4 * (size_t)quad], cnt = pk.hdr_quad[4 * (size_t)quad + 1];
    BDDMMA_STAMP(p, 0);
    const REAL INF = inf_v<REAL>();
    const uint32_t slot_first = !has_pack ? 0 : hp[0], l0 = !has_pack ? 0 : hp[2];
    NarrowRs<REAL> rs(d);
    rs.rebase_layers(d, l0);
    uint32_t ent[STAGE_ITERS], esl[STAGE_ITERS];
    stage_load_tables<REAL, WPB, BDDMMA_LD_TAB_AUX>(ent, esl, rs, c0_h, cnt, tid);  // on their way while the potentials are rebuilt
    REAL* const Tp = d.T + slot_first;
    REAL* const Fp = d.F + slot_first;
    const REAL* const lohi_p = d.lohi + 2 * (size_t)l0;
    const rsrc_t rr = make_rsrc(lrec, lrec_words);
    HopWindow hw{sOffN_[wave], sOffL_[wave], sOffR_[wave], q0, q1, slot_first, l0};
    uint32_t o[HC + 4];   // first slot of hops 0 .. HC + 3 of the pack (past the last hop: the pack's end)
    uint32_t lb[HC + 1];  // first layer of hops 0 .. HC
    P2 L[HC];             // {lo, hi} of the lane's layer in every hop
    P2 T[HC + 2];         // !REBUILD_T: costs-from-terminal of every hop, slots (2 lane, 2 lane + 1)
    REAL G[HC][4];        // REBUILD_T: costs-from-terminal at the four children {lo a, hi a, lo b, hi b} of the lane's layer in every hop
#pragma unroll
    for (int i = 0; i < HC + 4; ++i) o[i] = 0;
#pragma unroll
    for (int i = 0; i < HC + 1; ++i) lb[i] = 0;
    if constexpr (REBUILD_T) {
#pragma unroll
        for (int i = 0; i < HC; ++i) G[i][0] = G[i][1] = G[i][2] = G[i][3] = REAL(0);
    } else {
#pragma unroll
        for (int i = 0; i < HC + 2; ++i) T[i] = P2{REAL(0), REAL(0)};
    }
    auto ldrec = [&](uint32_t h) { return __builtin_amdgcn_raw_buffer_load_b128(rr, (uint32_t)lane * 16u, (rbase + h * 64u) * 16u, 0); };
    const uint32_t sink = (W + 2 * (uint32_t)lane) * S;  // this lane's TOP entry; BOT follows it
    u4v rA = u4v{0u, 0u, 0u, 0u}, rB = rA;               // records of the next two hops of the walk under way
    const uint32_t db = (uint32_t)wave * pk.stage_cap * (uint32_t)sizeof(P2);  // this wave's slots of the staging area
    if (has_pack) {
        hw.fill(pk, q0, lane);
#pragma unroll
        for (int i = 0; i < HC + 4; ++i) o[i] = hw.node_off(q0 + i);
#pragma unroll
        for (int i = 0; i < HC + 1; ++i) lb[i] = hw.layer_off(q0 + i);
        // every hop's arc costs at once (hops the pack does not have: past the descriptor, no traffic)
#pragma unroll
        for (int h = 0; h < HC; ++h)
            hop_load(L[h], rs.lohi, (uint32_t)h < hops ? (uint32_t)lane * (uint32_t)sizeof(P2) : OOB, lb[h] * (uint32_t)sizeof(P2));
        if constexpr (!REBUILD_T) {
#pragma unroll
            for (int h = 1; h < HC; ++h) pot_pair_load<REAL, false>(T[h], hop_rsrc(Tp, o[h], o[h + 1] - o[h]), 2u * (uint32_t)lane * S, o[h] * S);
        }
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const uint32_t j = lane + 64 * r;
            lds_st<REAL>(sFw, j * S, (j < o[1] - o[0]) ? REAL(0) : INF);  // every slot of hop 0 is a root (flush_costs_from_root)
        }
#pragma unroll
        for (int b = 0; b < 2; ++b) {  // the sink constants of both costs-from-terminal buffers
            lds_st<REAL>(sTw, b * BUF + sink, REAL(0));
            lds_st<REAL>(sTw, b * BUF + sink + S, INF);
        }
        wave_sync();
        if constexpr (REBUILD_T) {
            // ---- upward walk: the children's T of hops hops - 1 .. 0 into G, T of hops hops - 1 .. 1 into the buffers on the way (hop 0's
            // own T is not read by a forward sweep: its step only gathers)
            rA = ldrec(hops - 1);
            rB = ldrec(hops >= 2 ? hops - 2 : 0);
#pragma unroll
            for (int h = HC - 1; h >= 0; --h) {
                if ((uint32_t)h < hops) {  // uniform
                    const u4v ra = rA;
                    rA = rB;
                    rB = ldrec(h >= 2 ? h - 2 : 0);
                    const uint32_t tc = ((h + 1) & 1) * BUF, tn = (h & 1) * BUF;
                    const REAL tla = lds_ld<REAL>(sTw, tc + (ra[0] & 0xFFFFu)), tha = lds_ld<REAL>(sTw, tc + (ra[0] >> 16));
                    const REAL tlb = lds_ld<REAL>(sTw, tc + (ra[1] & 0xFFFFu)), thb = lds_ld<REAL>(sTw, tc + (ra[1] >> 16));
                    G[h][0] = tla, G[h][1] = tha, G[h][2] = tlb, G[h][3] = thb;
                    if (h >= 1) {
                        const P2 c = L[h];
                        const uint32_t flags = ra[2] >> 16;
                        const REAL ta = rmin(c.y + tha, c.x + tla);
                        const REAL tb = rmin(c.y + thb, c.x + tlb);
                        if (flags & LREC_REAL) lds_st<REAL>(sTw, tn + (ra[2] & 0xFFFFu), ta);
                        if (flags & LREC_TWO) lds_st<REAL>(sTw, tn + (ra[2] & 0xFFFFu) + S, tb);
                        wave_sync();
                    }
                }
            }
            BDDMMA_STAMP(p, 5);
        } else {
            if (2u * (uint32_t)lane < o[2] - o[1]) lds_st<P2>(sTw, BUF + 2u * (uint32_t)lane * S, T[1]);
        }
        rA = ldrec(0);
        rB = ldrec(1);  // (past the last hop: some other record, never used)
    }
    stage_load_pairs<REAL, WPB>(sD, ent, esl, rs, cnt, tid);
    if (WPB > 1) __syncthreads(); else wave_sync();
    BDDMMA_STAMP(p, 1);
    // ---- downward walk: k_fwd_narrow3's hop
#pragma unroll
    for (int h = 0; h < HC; ++h) {
        if ((uint32_t)h < hops) {  // uniform
            const u4v ra = rA;
            rA = rB;
            rB = ldrec(h + 2);
            const uint32_t fc = (h & 1) * BUF, fn = ((h + 1) & 1) * BUF;  // frontier of this / the next hop; !REBUILD_T: T of the next hop lies in fn, of hop h + 2 in fc
            const uint32_t stg = db + (lb[h] + (uint32_t)lane) * (uint32_t)sizeof(P2);  // the lane's layer inside the wave's staging slots
            const P2 c = L[h];
            // ---- the hop's LDS reads, one batch
            const uint32_t flags = ra[2] >> 16;
            REAL fa, fb;
            lds_ld2(fa, fb, sFw, fc + (ra[2] & 0xFFFFu));
            REAL tla, tha, tlb, thb;
            if constexpr (REBUILD_T) {
                tla = G[h][0], tha = G[h][1], tlb = G[h][2], thb = G[h][3];  // what the upward walk read through these very offsets
            } else {
                tla = lds_ld<REAL>(sTw, fn + (ra[0] & 0xFFFFu)), tha = lds_ld<REAL>(sTw, fn + (ra[0] >> 16));
                tlb = lds_ld<REAL>(sTw, fn + (ra[1] & 0xFFFFu)), thb = lds_ld<REAL>(sTw, fn + (ra[1] >> 16));
            }
            const P2 dd = lds_ld<P2>(dyn_lds, stg);
            // ---- set-up of the next hop's buffers (nothing above depends on it)
            if constexpr (!REBUILD_T)
                if (2u * (uint32_t)lane < o[h + 3] - o[h + 2]) lds_st<P2>(sTw, fc + 2u * (uint32_t)lane * S, T[h + 2]);
            lds_st<P2>(sFw, fn + 2u * (uint32_t)lane * S, P2{INF, INF});
            wave_sync();
            // ---- arithmetic: the layer's two candidates per side, their minimum, the deferred difference, the new arc costs
            fa = (flags & LREC_REAL) ? fa : INF;
            fb = (flags & LREC_TWO) ? fb : INF;
            const REAL m0 = rmin((fa + c.x) + tla, (fb + c.x) + tlb);
            const REAL m1 = rmin((fa + c.y) + tha, (fb + c.y) + thb);
            const REAL mm = mm_diff1(m0, m1, omega);
            P2 nc;
            nc.x = (c.x + min0(mm)) + dd.x;
            nc.y = (c.y + min0_neg(mm)) + dd.y;
            // ---- writes: new arc costs, staged difference, pushes into the next frontier, costs-from-root
            const rsrc_t rl = hop_rsrc(reinterpret_cast<const P2*>(lohi_p), lb[h], lb[h + 1] - lb[h]);  // ends with the hop's layers: idle lanes are dropped
            hop_store(nc, rl, (uint32_t)lane * (uint32_t)sizeof(P2), lb[h] * (uint32_t)sizeof(P2));
            if (flags & LREC_REAL) lds_st<REAL>(dyn_lds, stg, mm);
            lds_min(reinterpret_cast<REAL*>(sFw + fn + (ra[0] & 0xFFFFu)), fa + nc.x);  // sinks / idle lanes: the lane's own dummy entries
            lds_min(reinterpret_cast<REAL*>(sFw + fn + (ra[0] >> 16)), fa + nc.y);
            lds_min(reinterpret_cast<REAL*>(sFw + fn + (ra[1] & 0xFFFFu)), fb + nc.x);
            lds_min(reinterpret_cast<REAL*>(sFw + fn + (ra[1] >> 16)), fb + nc.y);
            if constexpr (STORE_F) {
                const rsrc_t rf = hop_rsrc(Fp, o[h], o[h + 1] - o[h]);  // LREC_NO_STORE lies past the slice
                pot_store_layer<REAL>(fa, fb, (flags & LREC_TWO) != 0, rf, ra[3] & 0xFFFFu, o[h] * S, pk.nt_potentials);
            }
            wave_sync();
        }
    }
    BDDMMA_STAMP(p, 3);
    if (WPB > 1) __syncthreads(); else wave_sync();
    BDDMMA_STAMP(p, 2);
    stage_flush<REAL, WPB>(sD, ent, esl, rs, cnt, tid);  // min-marginal differences of the round -> entry array
    BDDMMA_STAMP(p, 4);
}

template <typename REAL, int WPB, int HC, bool REBUILD_T, bool STORE_F>
__global__ void __launch_bounds__(64 * WPB) __attribute__((amdgpu_waves_per_eu(4))) k_fwd_narrow4(DevPtrs<REAL> d, PackDev pk, const uint32_t* __restrict__ lrec, const uint32_t* __restrict__ lrec_off,
                                                          uint32_t lrec_words, REAL omega)
{
    fwd_narrow4_body<REAL, WPB, HC, REBUILD_T, STORE_F>(d, pk, lrec, lrec_off, lrec_words, omega, blockIdx.x);
}

template <typename REAL, int WPB, int HC, bool REBUILD_F, bool STORE_T>
__device__ __forceinline__ void bwd_narrow4_body(const DevPtrs<REAL>& d, const PackDev& pk, const uint32_t* __restrict__ lrec,
                                                 const uint32_t* __restrict__ lrec_off, uint32_t lrec_words, REAL omega, uint32_t block_id)
{
    static_assert(HC + 1 <= (int)HOP_WIN, "one window of hop offsets has to hold the pack");
    constexpr int W = N3_W;
    constexpr uint32_t S = sizeof(REAL);
    constexpr uint32_t BUF = (W + 128) * S;
    using P2 = typename Pair<REAL>::type;
    extern __shared__ __attribute__((aligned(16))) unsigned char dyn_lds[];
    P2* sD = reinterpret_cast<P2*>(dyn_lds);
    __shared__ __attribute__((aligned(16))) unsigned char sT_[WPB][2][BUF];  // first walk: frontier of hop h in buffer h & 1; second: costs-from-terminal of hop h
    __shared__ uint32_t sOffN_[WPB][HOP_WIN], sOffL_[WPB][HOP_WIN], sOffR_[WPB][HOP_WIN];
    const uint32_t tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane((int)(tid >> 6));
    const int lane = tid & 63;
    unsigned char* sTw = &sT_[wave][0][0];
    const uint32_t n_quads = (pk.n_packs + WPB - 1) / WPB;
    const uint32_t quad = block_to_pack(block_id, n_quads, pk.xcd_chunk);
    BDDMMA_EXIT_IF(quad >= n_quads, d)
    const uint32_t p = quad * WPB + wave;
    const bool has_pack = p < pk.n_packs;
    const uint32_t* const hp = pk.hdr_pack + 8 * (size_t)(has_pack ? p : 0);  // resident headers, see fwd_narrow4_body
    const uint32_t q0 = !has_pack ? 0 : hp[4];
    const uint32_t hops = !has_pack ? 0 : (hp[5] & 0xFFFFu);  // <= HC
    const uint32_t q1 = q0 + hops;
    const uint32_t rbase = has_pack ? lrec_off[p] : 0;
    const uint32_t c0_h = pk.hdr_quad[4 * (size_t)quad], cnt = pk.hdr_quad[4 * (size_t)quad + 1];
    BDDMMA_STAMP(p, 0);
    const REAL INF = inf_v<REAL>();
    const uint32_t slot_first = !has_pack ? 0 : hp[0], l0 = !has_pack ? 0 : hp[2];
    NarrowRs<REAL> rs(d);
    rs.rebase_layers(d, l0);
    uint32_t ent[STAGE_ITERS], esl[STAGE_ITERS];
    stage_load_tables<REAL, WPB, BDDMMA_LD_TAB_AUX>(ent, esl, rs, c0_h, cnt, tid);
    REAL* const Tp = d.T + slot_first;
    REAL* const Fp = d.F + slot_first;
    const REAL* const lohi_p = d.lohi + 2 * (size_t)l0;
    const rsrc_t rr = make_rsrc(lrec, lrec_words);
    HopWindow hw{sOffN_[wave], sOffL_[wave], sOffR_[wave], q0, q1, slot_first, l0};
    uint32_t o[HC + 1];   // first slot of hops 0 .. HC of the pack (past the last hop: the pack's end)
    uint32_t lb[HC + 1];  // first layer of hops 0 .. HC
    P2 L[HC];             // {lo, hi} of the lane's layer in every hop
    P2 F[HC];             // costs-from-root of the lane's layer (nodes a, b = a + 1) in every hop
#pragma unroll
    for (int i = 0; i < HC + 1; ++i) o[i] = lb[i] = 0;
#pragma unroll
    for (int i = 0; i < HC; ++i) F[i] = P2{REAL(0), REAL(0)};
    auto ldrec = [&](uint32_t h) { return __builtin_amdgcn_raw_buffer_load_b128(rr, (uint32_t)lane * 16u, (rbase + h * 64u) * 16u, 0); };
    const uint32_t sink = (W + 2 * (uint32_t)lane) * S;
    u4v rA = u4v{0u, 0u, 0u, 0u}, rB = rA;
    const uint32_t db = (uint32_t)wave * pk.stage_cap * (uint32_t)sizeof(P2);
    if (has_pack) {
        hw.fill(pk, q0, lane);
#pragma unroll
        for (int i = 0; i < HC + 1; ++i) {
            o[i] = hw.node_off(q0 + i);
            lb[i] = hw.layer_off(q0 + i);
        }
#pragma unroll
        for (int h = 0; h < HC; ++h)
            hop_load(L[h], rs.lohi, (uint32_t)h < hops ? (uint32_t)lane * (uint32_t)sizeof(P2) : OOB, lb[h] * (uint32_t)sizeof(P2));
        if constexpr (REBUILD_F) {
            // ---- downward walk: the frontier of every hop, from 0 at the roots (every slot of hop 0 is one)
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                const uint32_t j = lane + 64 * r;
                lds_st<REAL>(sTw, j * S, (j < o[1] - o[0]) ? REAL(0) : INF);
            }
            rA = ldrec(0);
            rB = ldrec(1);  // (past the last hop: some other record, never used)
            wave_sync();
#pragma unroll
            for (int h = 0; h < HC; ++h) {
                if ((uint32_t)h < hops) {  // uniform
                    const u4v ra = rA;
                    rA = rB;
                    rB = ldrec(h + 2);
                    const uint32_t fc = (h & 1) * BUF, fn = ((h + 1) & 1) * BUF;
                    const uint32_t flags = ra[2] >> 16;
                    REAL fa, fb;
                    lds_ld2(fa, fb, sTw, fc + (ra[2] & 0xFFFFu));
                    F[h] = P2{fa, fb};
                    if ((uint32_t)h + 1 < hops) {  // uniform
                        lds_st<P2>(sTw, fn + 2u * (uint32_t)lane * S, P2{INF, INF});
                        wave_sync();
                        const P2 c = L[h];
                        fa = (flags & LREC_REAL) ? fa : INF;
                        fb = (flags & LREC_TWO) ? fb : INF;
                        lds_min(reinterpret_cast<REAL*>(sTw + fn + (ra[0] & 0xFFFFu)), fa + c.x);  // sinks / idle lanes: the lane's own entries behind the slots
                        lds_min(reinterpret_cast<REAL*>(sTw + fn + (ra[0] >> 16)), fa + c.y);
                        lds_min(reinterpret_cast<REAL*>(sTw + fn + (ra[1] & 0xFFFFu)), fb + c.x);
                        lds_min(reinterpret_cast<REAL*>(sTw + fn + (ra[1] >> 16)), fb + c.y);
                        wave_sync();
                    }
                }
            }
            wave_sync();
        } else {
            // costs-from-root of the two nodes of the lane's layer: slice of the hop, the record's store offset (idle lanes: past the slice -> 0)
#pragma unroll
            for (int h = 0; h < HC; ++h) {
                const uint32_t so = __builtin_amdgcn_raw_buffer_load_b32(rr, (uint32_t)lane * 16u + 12u, (rbase + ((uint32_t)h < hops ? h : 0u) * 64u) * 16u, 0);
                pot_pair_load<REAL, false>(F[h], hop_rsrc(Fp, o[h], o[h + 1] - o[h]), so & 0xFFFFu, o[h] * S);
            }
        }
#pragma unroll
        for (int b = 0; b < 2; ++b) {  // the sink constants (the first walk's pushes went through these entries)
            lds_st<REAL>(sTw, b * BUF + sink, REAL(0));
            lds_st<REAL>(sTw, b * BUF + sink + S, INF);
        }
        rA = ldrec(hops - 1);
        rB = ldrec(hops >= 2 ? hops - 2 : 0);
        wave_sync();
    }
    stage_load_pairs<REAL, WPB>(sD, ent, esl, rs, cnt, tid);
    if (WPB > 1) __syncthreads(); else wave_sync();
    BDDMMA_STAMP(p, 1);
    // ---- upward walk: k_bwd_narrow3's hop
#pragma unroll
    for (int h = HC - 1; h >= 0; --h) {
        if ((uint32_t)h < hops) {  // uniform
            const u4v ra = rA;
            rA = rB;
            rB = ldrec(h >= 2 ? h - 2 : 0);
            const uint32_t tc = ((h + 1) & 1) * BUF, tn = (h & 1) * BUF;
            const uint32_t stg = db + (lb[h] + (uint32_t)lane) * (uint32_t)sizeof(P2);
            const P2 c = L[h];
            const uint32_t flags = ra[2] >> 16;
            // ---- LDS reads
            const REAL tla = lds_ld<REAL>(sTw, tc + (ra[0] & 0xFFFFu)), tha = lds_ld<REAL>(sTw, tc + (ra[0] >> 16));
            const REAL tlb = lds_ld<REAL>(sTw, tc + (ra[1] & 0xFFFFu)), thb = lds_ld<REAL>(sTw, tc + (ra[1] >> 16));
            const P2 dd = lds_ld<P2>(dyn_lds, stg);
            // ---- arithmetic
            const REAL fa = (flags & LREC_REAL) ? F[h].x : INF;
            const REAL fb = (flags & LREC_TWO) ? F[h].y : INF;
            const REAL m0 = rmin((fa + c.x) + tla, (fb + c.x) + tlb);
            const REAL m1 = rmin((fa + c.y) + tha, (fb + c.y) + thb);
            const REAL mm = mm_diff1(m0, m1, omega);
            P2 nc;
            nc.x = (c.x + min0(mm)) + dd.x;
            nc.y = (c.y + min0_neg(mm)) + dd.y;
            const REAL ta = rmin(nc.y + tha, nc.x + tla);
            const REAL tb = rmin(nc.y + thb, nc.x + tlb);
            // ---- writes
            const rsrc_t rl = hop_rsrc(reinterpret_cast<const P2*>(lohi_p), lb[h], lb[h + 1] - lb[h]);
            hop_store(nc, rl, (uint32_t)lane * (uint32_t)sizeof(P2), lb[h] * (uint32_t)sizeof(P2));
            if (flags & LREC_REAL) {
                lds_st<REAL>(dyn_lds, stg, mm);
                lds_st<REAL>(sTw, tn + (ra[2] & 0xFFFFu), ta);
            }
            if (flags & LREC_TWO) lds_st<REAL>(sTw, tn + (ra[2] & 0xFFFFu) + S, tb);
            if constexpr (STORE_T) {
                const rsrc_t rt = hop_rsrc(Tp, o[h], o[h + 1] - o[h]);
                pot_store_layer<REAL>(ta, tb, (flags & LREC_TWO) != 0, rt, ra[3] & 0xFFFFu, o[h] * S, pk.nt_potentials);
            }
            wave_sync();
        }
    }
    BDDMMA_STAMP(p, 3);
    if (WPB > 1) __syncthreads(); else wave_sync();
    BDDMMA_STAMP(p, 2);
    stage_flush<REAL, WPB>(sD, ent, esl, rs, cnt, tid);
    BDDMMA_STAMP(p, 4);
    if (!has_pack) return;
    // lower bound contribution of this pack: sum of root costs-from-terminal (bdd_cuda_base.cu:1243-1251); every slot of the first hop is a root
    const uint32_t n0 = o[1] - o[0];
    double s = 0.0;
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const uint32_t j = lane + 64 * r;
        if (j < n0) s += (double)lds_ld<REAL>(sTw, j * S);  // hop 0: buffer 0
    }
    for (int off2 = 32; off2 > 0; off2 >>= 1) s += __shfl_down(s, off2);
    if (lane == 0) d.lb_partial[pk.lb_base + p] = s;
}

template <typename REAL, int WPB, int HC, bool REBUILD_F, bool STORE_T>
__global__ void __launch_bounds__(64 * WPB) __attribute__((amdgpu_waves_per_eu(4))) k_bwd_narrow4(DevPtrs<REAL> d, PackDev pk, const uint32_t* __restrict__ lrec, const uint32_t* __restrict__ lrec_off,
                                                          uint32_t lrec_words, REAL omega)
{
    bwd_narrow4_body<REAL, WPB, HC, REBUILD_F, STORE_T>(d, pk, lrec, lrec_off, lrec_words, omega, blockIdx.x);
}

}  // namespace bddmma
