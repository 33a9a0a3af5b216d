// kernels/small.hpp — instances that fit ONE workgroup: whole MMA iterations inside one launch (k_iterate_small, k_iterate_small_batch),
// and whole learned iterations (k_learned_small, k_learned_small_batch; with their history step: k_learned_small_hist_batch, kernels/smallhist.hpp;
// with the stopping rule on the bound's slope: k_learned_small_stop_batch, k_learned_small_hist_stop_batch, kernels/smallstop.hpp).
// Part of kernels.hpp (include that, not this file: the parts build on each other in its order).
#pragma once

namespace bddmma {

// =============================================================================================
// tiny instances: n iterations per launch, the whole solver state resident in one workgroup's LDS
// =============================================================================================
// An instance of a handful of packs (the 8 x 8 assignment problem of BASELINE.json configs[0] is ONE pack of 16 BDDs) is four dependent
// launches per iteration of which each is a few hundred nanoseconds of work behind ~4 us of launch, header, table and pair round trips:
// 18.5 us per iteration (profiles/r03_1m_latency.txt).  Between the workgroups of a grid a pass boundary costs what a launch costs
// (tools/gridsync.hip, round 5) — but when ALL packs fit one workgroup the boundary is a __syncthreads.  So here one workgroup copies the
// packs' costs-from-terminal, arc costs and staged delta pairs into LDS once, runs
//     forward solve sweep | exchange | backward solve sweep | exchange + bound + run_solver's tests
// n times out of LDS with barriers in between, and writes the state back once.  The sweeps are the hop loops of k_fwd_res2 / k_bwd_res2
// on the same per-lane records (same operations in the same order: bit-equal potentials, costs and deferred differences); the exchange is
// one thread per variable over the variable's entries in (variable, bdd) order, accumulated in the exchange tile's type (double) and
// rounded once, as k_exchange_reduce does — bit-equal to its LDS atomics whenever the double sum is exact (float instances) or has at
// most two terms (any variable in <= 2 BDDs), and within rounding of a different summation order otherwise.  run_solver's tests run in
// the kernel after every iteration (run_ctl_finish: the reference's order, the published bound, the latched stop): the launch ends with
// the iteration that met a criterion, so state and iteration count are the sequential loop's (run_solver_util.h:40-73).
// Preconditions (SolverT::small_ok): the second-generation resident records exist (packs of 64 slots, layers of <= 2 nodes, one stage
// group per pack, one staging round per quad), nothing but narrow packs, at most SMALL_MAX_PACKS of them, no L-BFGS wrapper attached
// (x_layer), not the deterministic / by-variable exchanges, everything within the CU's LDS.
constexpr uint32_t SMALL_MAX_PACKS = 16;
struct SmallDev {
    const uint32_t* pack_hdr;   // layout.hpp: struct Resident — 8 words per pack
    const uint32_t* quad_hdr;   // 4 words per quad of the staging tables: first item, items
    const uint32_t* rec;        // Res2Records
    const uint32_t* rec_off;
    uint32_t rec_words;
    uint32_t ns, nl;            // slot / layer capacity of a pack's LDS region (res2_wave_bytes)
    uint32_t n_packs, n_quads, wpb;  // wpb: packs per quad (the staging tables' LDS slots are quad-relative)
    const uint32_t* var_ptr;    // [n_vars + 1]: the variable's entries in var_lds / var_ent, (variable, bdd) order
    const uint32_t* var_lds;    // byte offset of the entry's staging pair inside the staging area
    const uint32_t* var_ent;    // the entry's index in mm_binned / delta_lay
    uint32_t n_vars, n_entries;
    uint32_t rec_cap;           // bytes of a pack's records kept in LDS (RL instantiation): 1 KiB per hop of the longest pack + one spare
    uint32_t off_regions, off_vp, off_vl, off_mm, off_misc, off_rec;  // byte offsets inside the dynamic LDS: pack regions | var_ptr copy | var_lds copy |
                                                                      // the last backward sweep's differences by (variable, bdd) | bounds + flag | records
};
// (rec_cap = 0: the records stay in global memory)
// A pack's staging area and its {lo, hi} array carry ONE pair more than the nl the records address: the dummy pair at offset nl * 2 S that the
// records rewritten in LDS (RL instantiation) point padding lanes and non-head lanes at, so that the hop's stores need no exec masks.
__host__ __device__ inline uint32_t small_stage_stride(uint32_t nl) { return nl + 1u; }   // pairs per pack in the staging area
__host__ __device__ inline uint32_t small_region_bytes(uint32_t real_size, uint32_t ns, uint32_t nl) { return res2_wave_bytes(real_size, ns, nl) + 2u * real_size; }
inline uint32_t small_lds_bytes(uint32_t real_size, uint32_t n_packs, uint32_t n_vars, uint32_t n_entries, SmallDev& sm)
{
    const uint32_t ns = sm.ns, nl = sm.nl;
    uint32_t *off_regions = &sm.off_regions, *off_vp = &sm.off_vp, *off_vl = &sm.off_vl, *off_misc = &sm.off_misc;
    uint32_t o = n_packs * small_stage_stride(nl) * 2u * real_size;   // staging area: a {lo, hi} pair per layer slot, nl (+ the dummy) per pack (the sweeps' own staging reserves stage_cap)
    o = (o + 15u) & ~15u;
    *off_regions = o;
    o += n_packs * small_region_bytes(real_size, ns, nl);
    o = (o + 15u) & ~15u;
    *off_vp = o;
    o += (n_vars + 1u) * 4u;
    o = (o + 15u) & ~15u;
    *off_vl = o;
    o += n_entries * 4u;
    o = (o + 15u) & ~15u;
    sm.off_mm = o;
    o += n_entries * real_size;
    o = (o + 15u) & ~15u;
    *off_misc = o;
    o += (SMALL_MAX_PACKS + 2u) * 8u;
    o = (o + 15u) & ~15u;
    sm.off_rec = o;
    o += n_packs * sm.rec_cap;
    return o;
}

// What the LEARNED form (learned iterations: SolverT::learned_iterations, bdd_cuda_learned_mma.cu:9-262) takes beyond SmallDev — a struct of
// its own, so that SmallDev and the plain kernels' argument layout stay as they are.  In LDS:
//   the distribution weights by (variable, bdd) entry — alpha_ent (binned entry order) gathered through var_ent — live in the off_mm area:
//           that area receives the last backward sweep's differences in the exit exchange, which runs behind the last weighted one, so the
//           weights are dead when it is written (every launch loads them again);
//   off_om  (behind the plain areas) omega per layer of each pack, om_stride = the longest pack's layers per pack: omega_lay (layer order,
//           the order of lohi) or, where that is null, the scalar omega in every slot — ONE instantiation serves bddmma_learned_iterations
//           and _omega_vec, so an omega_vec that holds omega everywhere gives the scalar call's bits.  Padding lanes read the slot their
//           {lo, hi} offset names: slot 0, or (records rewritten in LDS) slot nl — of the next packs' values or, behind the last pack, the
//           nl + 1 - om_stride spare slots the area ends with; whatever they read is not used (their minima are +inf: the difference is 0).
// The two shapes that decided this layout: the 10-pack float and the 7-pack double set covers of tests/test_gpu_small_learned.py fit the
// CU's LDS with it and not with a weight area of their own and nl + 1 omega slots per pack.
template <typename REAL>
struct SmallLearn {
    const REAL* alpha_ent;
    const REAL* omega_lay;
    uint32_t off_om, om_stride;
};
inline uint32_t small_learn_lds_bytes(uint32_t real_size, uint32_t n_packs, uint32_t nl, uint32_t max_layers, uint32_t plain_bytes, uint32_t& off_om)
{
    const uint32_t o = (plain_bytes + 15u) & ~15u;
    off_om = o;
    return o + ((n_packs - 1u) * max_layers + small_stage_stride(nl)) * real_size;
}

// RECORD (k_grad_small_batch, kernels/gradsmall.hpp: the backward of the learned iterations): what the reverse of iteration k reads, written to
// global memory at the pass boundaries — in front of iteration k (and behind the last one, k = n_iters) the arc costs, the deferred
// differences in layer order and the costs-to-terminal; behind its forward sweep the arc costs, the differences and the costs-from-root.
// One block of 6 ls + 2 ss values per iteration, ls / ss the solver's layer / slot counts rounded up to 4: c (2 ls) | dm (ls) | T (ss) | c1 (2 ls) |
// mm1 (ls) | F (ss); the block behind the last iteration holds the first three.  Layers and slots are the solver's.
template <typename REAL>
struct SmallRecord {
    REAL* base;
    uint32_t ls, ss;
    __host__ __device__ size_t stride() const { return 6 * (size_t)ls + 2 * (size_t)ss; }
    __host__ __device__ REAL* c(uint32_t k) const { return base + k * stride(); }          // in front of iteration k
    __host__ __device__ REAL* dm(uint32_t k) const { return c(k) + 2 * (size_t)ls; }
    __host__ __device__ REAL* T(uint32_t k) const { return dm(k) + ls; }
    __host__ __device__ REAL* c1(uint32_t k) const { return T(k) + ss; }                    // behind its forward sweep
    __host__ __device__ REAL* mm1(uint32_t k) const { return c1(k) + 2 * (size_t)ls; }
    __host__ __device__ REAL* F(uint32_t k) const { return mm1(k) + ls; }
};

// HISTORY (k_learned_small_hist_batch, kernels/smallhist.hpp: bddmma_learned_iterations_history_batch): the history step of
// SolverT::learned_iterations (solver_impl.hpp, bdd_cuda_learned_mma.cu:211-254) behind the backward sweep of every iteration with index
// >= hist_from, out of LDS:
//   the arg-min path of every BDD (FWD_SOLUTION, kernels/narrow.hpp): each wave runs a plain forward pass over its pack's hops — costs-from-
//           root from the current arc costs into the pack's F array, which the next forward solve sweep initialises again (after the launch's
//           last iteration the epilogue stores them; the host state marks the costs-from-root invalid after every launch of whole
//           iterations, so nothing reads them).  No LDS of its own: the on-path marks of a hop's nodes are the 64 dummy entries behind the
//           pack's costs-from-root, indexed by the node's slot modulo 64 (a hop's slots are consecutive and at most 64; this pass pushes into
//           no dummy entry), and a layer's decision waits in the .y half of its staging pair — dead between a backward sweep and the next
//           exchange, which writes every pair before a sweep reads it — until the wave applies the sol_avg rule to its layers, coalesced.
//           As other waves' exchange threads write this pack's pairs, a workgroup barrier separates the history step from the next exchange.
//   the per-BDD bounds: thread b owns BDD b (a member has at most 64 BDDs per pack: every root is a node of hop 0) and reads T[root] from
//           the LDS region of the root's pack; the bounds of the two steps before wait in lb_state, between steps and across launches.
// `tracked` is the number of history steps of the call before this launch; the outputs are this member's part of the caller's arrays.
// What the step reads lives in global memory (SmallHistMem, part of the member's item) and is fetched by scalar loads inside the step: held
// in SGPRs through the solve sweeps it spilled the 16-wave instantiations, whose budget is 128 VGPRs, into scratch.
template <typename REAL>
struct SmallHistMem {
    const uint32_t* root_slot;   // [n_bdds]: the solver's slot of BDD b's root (the order of bddmma_lower_bound_per_bdd)
    REAL* lb_state;              // [2 n_bdds]: the bound of the last history step | of the one before it
    REAL *sol_avg, *lb_first, *lb_second;   // this member's part of the caller's arrays
    uint32_t n_bdds;
    REAL beta;
};
template <typename REAL>
struct SmallHist {
    const SmallHistMem<REAL>* mem;
    uint32_t hist_from, tracked;
};
// What the history form asks beyond the learned form (SolverT::small_hist_ok): a thread per BDD.  It holds by construction — every root is a
// node of hop 0, so a pack has at most 64 BDDs and a member at most 64 per wave — and is checked because the kernel relies on it.
inline bool small_hist_fits(uint64_t n_bdds, uint32_t nw) { return n_bdds <= 64ull * nw; }
// compute_exp_moving_avg with the bits of k_ema (kernels/elementwise.hpp), whose sum the compiler contracts into one fused multiply-add —
// in float around (1 - beta) * cur, the product beta * avg being rounded to float first; in double around beta * avg, with (1 - beta) * cur
// rounded (k_ema's ISA: v_mul_f32, v_fmac_f64 / v_mul_f64, v_fmac_f64).  Written out, so that the same operations run wherever this is inlined.
template <typename REAL>
__device__ __forceinline__ REAL small_ema(REAL avg, REAL cur, REAL beta)
{
#pragma clang fp contract(off)
    if constexpr (sizeof(REAL) == 4) {
        const float ba = beta * avg;
        return (float)__builtin_fma(1.0 - (double)beta, (double)cur, (double)ba);
    } else {
        const double oc = (1.0 - beta) * cur;
        return __builtin_fma(beta, avg, oc);
    }
}

// STOP (k_learned_small_stop_batch, k_learned_small_hist_stop_batch, kernels/smallstop.hpp: bddmma_learned_iterations_stop_batch): the stopping
// rule of SolverT::learned_iterations (solver_impl.hpp; bdd_cuda_learned_mma.cu:185-270) inside the launch.  A member's stop block lives in
// global memory and is reached through its item: the slope, the call's two counts, the bound on entry and the set-once initial change (not
// finite: unset) are the call's; the rest is in-out across the launches of one call.  A launch whose block says `done` returns before it touches anything, so the
// member's state stays what its own last launch left.
struct SmallStopBlock {
    double slope, lb_initial, initial_change;
    double lb_prev, lb_post;
    uint64_t num_itr, cfi;     // the call's num_itr and compute_history_for_itr
    uint64_t tracked, iters;   // history steps made / iterations run by the call so far
    uint32_t converged, done;
};
// (A member that is not done has run every iteration of the call's earlier launches: `iters` is also the call's index of the launch's
// first iteration, so a launch takes nothing but the block.)
// The rule's working values between the iterations of a launch: static LDS, written and read by lane 0 of wave 0 only — but for `stop`
// (read by everyone behind the barrier that follows the test) and for trk / step, which the test of iteration i writes for iteration i + 1
// into the slot of that iteration's parity: everyone reads the slot of iteration i behind its backward sweep's barrier, possibly while
// wave 0 is already writing the other one.
struct SmallStopWork {
    double lb_post, initial, slope;
    uint64_t num_itr, cfi, tracked, iters;
    uint32_t converged, stop;
    uint32_t trk[2], step[2];   // is the iteration tracked (bdd_cuda_learned_mma.cu:211) / the history steps of the call before it, saturated at 3
};
constexpr uint32_t SMALL_STOP_LDS = 96;
static_assert(sizeof(SmallStopWork) <= SMALL_STOP_LDS, "the admission rule (SolverT::small_stop_ok) reserves SMALL_STOP_LDS bytes");
// The instantiations that exist: every one but the history form of 16 waves in double with the records in L2, which sits at 128 VGPRs without
// the rule and would spill one register into scratch with it.  A member that would need it is not admitted
// (bddmma_fused_small_stop is 0), with or without a history in the call.
template <typename REAL>
constexpr bool small_stop_built(int nw, bool rl) { return !(sizeof(REAL) == 8 && nw == 16 && !rl); }
template <bool STOP>
__device__ __forceinline__ SmallStopWork* small_stop_work()
{
    if constexpr (STOP) {
        __shared__ SmallStopWork w;
        return &w;
    } else {
        return nullptr;
    }
}

// The workgroup's work, shared by k_iterate_small (one instance per launch) and k_iterate_small_batch (one instance per workgroup).
// NW waves, pack p on wave p (n_packs <= NW); RL: the packs' records live in LDS too (1 KiB per hop), else they stream from L2 eight hops ahead
// LEARNED (k_learned_small, k_learned_small_batch): n learned iterations,
//     weighted exchange | forward solve sweep | weighted exchange | backward solve sweep
// n times and then the plain exchange once.  On entry the layer slots' .x hold the solver's deferred differences (a pending isotropic delta is
// ignored: the state contract of bddmma_learned_iterations); the weighted exchange gives entry k {alpha[k] * Slo, alpha[k] * Shi} of its
// variable's sums — no division by the BDD count, one product each in REAL: exchange_reduce_body<.., WEIGHTED>'s arithmetic; the hop takes
// omega from its layer's slot.  The plain exchange behind the last backward sweep and the plain epilogue leave what the four-launch path
// leaves: the last backward pass's differences deferred, delta their isotropic exchange, the bound's partial sums.  No run_solver (run.ctl
// is null there), so no early return at all.
// STOP: the stopping rule behind every iteration (SmallStopBlock above): the bound's partial sums are taken every iteration, wave 0 reduces
// them in k_lb_reduce's shape and its lane 0 applies the rule in double; the iteration that stops leaves through the exit exchange and the
// epilogue, as the per-member loop does.  With HISTORY the tracked window is the rule's: hs->hist_from / tracked are not read.
template <typename REAL, int NW, bool RL, bool LEARNED = false, bool RECORD = false, bool HISTORY = false, bool STOP = false>
__device__ __forceinline__ void small_iterate(const SmallDev& sm, const DevPtrs<REAL>& d, const PackDev& pk, REAL omega, uint32_t n_iters, const RunStep& run,
                                              const SmallLearn<REAL>* ln = nullptr, const SmallRecord<REAL>* rec = nullptr, const SmallHist<REAL>* hs = nullptr,
                                              SmallStopBlock* const* stp = nullptr)
{
    static_assert(!RECORD || LEARNED, "only the learned iterations are recorded");
    static_assert(!HISTORY || LEARNED, "only the learned iterations have a history");
    static_assert(!(HISTORY && RECORD), "the history form is not recorded");
    static_assert(!STOP || (LEARNED && !RECORD), "the stopping rule is the learned iterations', and its form is not recorded");
    constexpr uint32_t S = sizeof(REAL);
    constexpr uint32_t NT = 64 * NW;
    using P2 = typename Pair<REAL>::type;
    extern __shared__ __attribute__((aligned(16))) unsigned char dyn_lds[];
    const uint32_t tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane((int)(tid >> 6));
    const int lane = tid & 63;
    // run_solver: launches queued behind the iteration that met a criterion do nothing (DevPtrs::stop / run_iter = this launch's first iteration)
    if constexpr (!LEARNED)
        if (d.stop != nullptr && *d.stop <= d.run_iter) return;
    // (STOP: stp is the address of the block's address in the member's item — the block is reached by scalar loads where it is used, so that
    // nothing of it lives in registers through the solve sweeps)
    if constexpr (STOP)
        if ((*stp)->done != 0u) return;   // (uniform) stopped by an earlier launch of the call
    SmallStopWork* const ws = small_stop_work<STOP>();
    const REAL INF = inf_v<REAL>();
    const uint32_t region = small_region_bytes(S, sm.ns, sm.nl), dstride = small_stage_stride(sm.nl);
    const uint32_t ll_dummy = sm.nl * 2u * S;   // the dummy pair of a pack's {lo, hi} array and of its staging area
    uint32_t* const vp = reinterpret_cast<uint32_t*>(dyn_lds + sm.off_vp);
    uint32_t* const vl = reinterpret_cast<uint32_t*>(dyn_lds + sm.off_vl);
    double* const lbp = reinterpret_cast<double*>(dyn_lds + sm.off_misc);          // per-pack bounds of the iteration
    uint32_t* const flag = reinterpret_cast<uint32_t*>(dyn_lds + sm.off_misc + SMALL_MAX_PACKS * 8u);  // [0]: stop reason of the iteration
    const rsrc_t rr = make_rsrc(sm.rec, sm.rec_words);

    REAL* const mmE = reinterpret_cast<REAL*>(dyn_lds + sm.off_mm);
    REAL* const alE = mmE;   // LEARNED: the weights by (variable, bdd) entry, until the exit exchange writes the differences there
    // ---- this wave's pack: everything the sweeps need from the headers, once
    const uint32_t p = (uint32_t)wave;
    const bool has_pack = p < sm.n_packs;
    const uint32_t* hp = sm.pack_hdr + 8 * (size_t)(has_pack ? p : 0);
    const uint32_t slot0 = hp[0], layer0 = hp[2];
    const uint32_t nslots = has_pack ? hp[1] : 0, nlayers = has_pack ? hp[3] : 0, nh = has_pack ? (hp[5] & 0xFFFFu) : 0;
    const uint32_t rbase = sm.rec_off[has_pack ? p : 0];
    const uint32_t db = p * dstride * (uint32_t)sizeof(P2);
    const uint32_t wb = sm.off_regions + p * region, wbF = wb + res2_f_off(S, sm.ns), wbC = wb + res2_c_off(S, sm.ns);
    const uint32_t rl = sm.off_rec + p * sm.rec_cap, rlane = rl + (uint32_t)lane * 16u;
    const uint32_t nhm1 = nh ? nh - 1u : 0u;
    const uint32_t ob = LEARNED ? ln->off_om + p * ln->om_stride * S : 0u;   // LEARNED: this pack's omega slots (layer j at ob + j S = ob + ll / 2)
    // ---- prologue: the state -> LDS
    if (has_pack) {
        wave_copy_to_lds(d.T + slot0, dyn_lds + wb, nslots * S, lane);
        wave_copy_to_lds(d.lohi + 2 * (size_t)layer0, dyn_lds + wbC, nlayers * (uint32_t)sizeof(P2), lane);
        if (RL) {
            // hop h's 64 records: 1 KiB at rl + 1024 h — REWRITTEN on the way so that the hop loop needs no exec masks: padding lanes read and
            // write the dummy pair and the spare entry ns + 2 of the costs-from-terminal (nothing reads either); both lanes of a two-node
            // layer store the layer's new arc costs (the same pair to the same address — in LDS a duplicate costs nothing, the head-only
            // rule of the streaming sweeps saves global bandwidth).  A padding lane is then the lane whose pair offset is the dummy's;
            // .w keeps only the two-node flag, as the sign.
            for (uint32_t h = 0; h < nh; ++h) {
                u4v r = __builtin_amdgcn_raw_buffer_load_b128(rr, (uint32_t)lane * 16u, (rbase + h * 64u) * 16u, 0);
                if (r[3] == RES2_PAD) {
                    r[2] = ll_dummy | (((sm.ns + 2u) * S) << 16);
                    r[3] = 0u;
                } else {
                    r[3] = (r[3] & 0x10000u) ? 0x80000000u : 0u;   // the two-node flag as the sign: one compare in the hop
                }
                lds_st<u4v>(dyn_lds, rl + h * 1024u + (uint32_t)lane * 16u, r);
            }
        }
    }
    for (uint32_t i = tid; i <= sm.n_vars; i += NT) vp[i] = sm.var_ptr[i];
    for (uint32_t i = tid; i < sm.n_entries; i += NT) vl[i] = sm.var_lds[i];
    if constexpr (LEARNED) {
        // the deferred differences -> the .x of the entries' layer slots; the weights -> (variable, bdd) order; omega -> this pack's slots
        for (uint32_t k = tid; k < sm.n_entries; k += NT) {
            const uint32_t e = sm.var_ent[k];
            lds_st<REAL>(dyn_lds, sm.var_lds[k], d.mm_binned[e]);
            alE[k] = ln->alpha_ent[e];
        }
        if (has_pack)
            for (uint32_t j = (uint32_t)lane; j < nlayers; j += 64u)
                lds_st<REAL>(dyn_lds, ob + j * S, ln->omega_lay != nullptr ? ln->omega_lay[layer0 + j] : omega);
    } else {   // the staged delta pairs of every quad: entry -> its layer's slot of the staging area (quad-relative slots, as the sweeps' own staging)
        P2* const sD = reinterpret_cast<P2*>(dyn_lds);
        for (uint32_t q = 0; q < sm.n_quads; ++q) {
            const uint32_t c0 = sm.quad_hdr[4 * (size_t)q], cnt = sm.quad_hdr[4 * (size_t)q + 1];
            for (uint32_t i = tid; i < cnt; i += NT) {
                const uint32_t e = d.cs_entry[c0 + i], sl = d.cs_slot[c0 + i];
                sD[(size_t)(q * sm.wpb + sl / pk.stage_cap) * dstride + sl % pk.stage_cap] = reinterpret_cast<const P2*>(d.delta_lay)[e];   // quad-relative slot -> (pack, layer)
            }
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the direct-to-LDS copies have landed
    if (has_pack && lane < 2) lds_st<REAL>(dyn_lds, wb + (sm.ns + (uint32_t)lane) * S, lane == 0 ? REAL(0) : INF);  // sinks: cost to terminal 0 (top) / +inf (bot)
    RunCtl c{};
    if constexpr (!LEARNED)
        if (run.ctl != nullptr && tid == 0) c = *run.ctl;
    if constexpr (STOP) {
        if (wave == 0) {
            // the call's first launch: the bound on entry from the partial sums the member's last backward sweep left (the caller has made them
            // valid), in k_lb_reduce's shape — SolverT::learned_iterations' lower_bound() in front of its loop
            SmallStopBlock* const b = *stp;
            const bool first = b->iters == 0;   // (uniform)
            double t = 0.0;
            if (first) {
                t = (uint32_t)lane < sm.n_packs ? d.lb_partial[pk.lb_base + (uint32_t)lane] : 0.0;
                for (int off2 = 32; off2 > 0; off2 >>= 1) t += __shfl_down(t, off2);
            }
            if (lane == 0) {
                if (first) b->lb_initial = t;
                ws->lb_post = first ? t : b->lb_post;
                ws->initial = b->initial_change;
                ws->slope = b->slope;
                ws->num_itr = b->num_itr;
                ws->cfi = b->cfi;
                ws->tracked = b->tracked;
                ws->iters = b->iters;
                ws->converged = b->converged;
                ws->stop = 0u;
                ws->trk[0] = (b->cfi > 0 && (b->cfi >= b->num_itr - b->iters || b->converged != 0u)) ? 1u : 0u;
                ws->step[0] = (uint32_t)(b->tracked < 3 ? b->tracked : 3);
            }
        }
    }
    __syncthreads();

    // The exchange (compute_delta + normalize_delta + the broadcast to the variable's layers, bdd_cuda_parallel_mma.cu:358-430,191-197): a
    // thread per variable; the layer slots hold the sweeps' min-marginal differences in .x and receive the variable's normalised pair.
    // `save_mm` (the exchange behind a backward sweep): the differences are kept by (variable, bdd) for the epilogue — they are the
    // solver's deferred differences (get_solver_costs / net_solver_costs) if this turns out to be the launch's last iteration.
    // A thread's first variable (v = tid) with at most four entries is served from registers: its entries' addresses are read once, before the
    // iterations, so an exchange is one LDS round trip (the differences), the sums, the pair, the stores.  Other variables: the generic loop,
    // eight entries per batch of independent loads.  Same order of the additions in both: (variable, bdd).
    // sum / (number of BDDs), rounded once like k_exchange_reduce's division: a count that is a power of two (every variable of an assignment
    // problem sits in two BDDs) divides exactly by an exponent shift — one instruction instead of the ~10 of a correctly rounded division
    auto mean_pair = [&](double lo, double hi, uint32_t n) -> P2 {
        P2 pr;
        if ((n & (n - 1u)) == 0u) {
            const int sh = -(int)__builtin_ctz(n);
            if constexpr (sizeof(REAL) == 4) { pr.x = __builtin_ldexpf(REAL(lo), sh); pr.y = __builtin_ldexpf(REAL(hi), sh); }
            else { pr.x = __builtin_ldexp(REAL(lo), sh); pr.y = __builtin_ldexp(REAL(hi), sh); }
        } else {
            const REAL nb = REAL(n);
            pr.x = REAL(lo) / nb;
            pr.y = REAL(hi) / nb;
        }
        return pr;
    };
    const uint32_t v_own = tid;
    uint32_t own_k0 = 0, own_n = 0, own_a[4] = {0u, 0u, 0u, 0u};
    REAL own_w[4] = {REAL(0), REAL(0), REAL(0), REAL(0)};   // LEARNED: the weights of those entries (they do not change within a launch)
    if (v_own < sm.n_vars) {
        own_k0 = vp[v_own];
        own_n = vp[v_own + 1] - own_k0;
#pragma unroll
        for (int j = 0; j < 4; ++j) own_a[j] = vl[own_k0 + ((uint32_t)j < own_n ? j : 0)];   // past the last entry: the first again (see the exchange)
        if constexpr (LEARNED)
            if (own_n != 0) {
#pragma unroll
                for (int j = 0; j < 4; ++j) own_w[j] = alE[own_k0 + ((uint32_t)j < own_n ? j : 0)];
            }
    }
    // `weighted` (a compile-time tag; LEARNED only): the learned iterations' exchange — the same sums, entry k receives alpha[k] * them
    auto exchange = [&](bool save_mm, auto weighted) {
        constexpr bool W = decltype(weighted)::value;
        auto generic = [&](uint32_t v) {
            const uint32_t k0 = vp[v], k1 = vp[v + 1];
            if (k1 == k0) return;
            double lo = 0.0, hi = 0.0;
            for (uint32_t kb = k0; kb < k1; kb += 8) {
                uint32_t a[8];
                REAL m[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) a[u] = kb + u < k1 ? vl[kb + u] : 0u;
#pragma unroll
                for (int u = 0; u < 8; ++u) m[u] = lds_ld<REAL>(dyn_lds, a[u]);
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    if (kb + u < k1) {
                        if (m[u] > 0) hi += (double)m[u];
                        else if (m[u] < 0) lo += (double)(-m[u]);
                        if (save_mm) mmE[kb + u] = m[u];
                    }
                }
            }
            if constexpr (W) {
                const REAL slo = REAL(lo), shi = REAL(hi);
                for (uint32_t kb = k0; kb < k1; kb += 8) {
                    uint32_t a[8];
                    REAL w[8];
#pragma unroll
                    for (int u = 0; u < 8; ++u) {
                        a[u] = kb + u < k1 ? vl[kb + u] : 0u;
                        w[u] = kb + u < k1 ? alE[kb + u] : REAL(0);
                    }
#pragma unroll
                    for (int u = 0; u < 8; ++u)
                        if (kb + u < k1) {
                            P2 pr;
                            pr.x = w[u] * slo;
                            pr.y = w[u] * shi;
                            lds_st<P2>(dyn_lds, a[u], pr);
                        }
                }
                return;
            }
            const P2 pr = mean_pair(lo, hi, k1 - k0);
            for (uint32_t kb = k0; kb < k1; kb += 8) {
                uint32_t a[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) a[u] = kb + u < k1 ? vl[kb + u] : 0u;
#pragma unroll
                for (int u = 0; u < 8; ++u)
                    if (kb + u < k1) lds_st<P2>(dyn_lds, a[u], pr);
            }
        };
        if (own_n != 0 && own_n <= 4) {
            REAL m[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) m[j] = lds_ld<REAL>(dyn_lds, own_a[j]);
            // without branches: an entry past the variable's last reads its first entry's slot again and counts as 0 — adding +0.0 changes no
            // sum, a NaN difference adds nothing either way (max(NaN, 0) = 0 as `NaN > 0` is false) — and stores the pair there once more
            double lo = 0.0, hi = 0.0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const REAL x = (uint32_t)j < own_n ? m[j] : REAL(0);
                if constexpr (sizeof(REAL) == 4) { hi += (double)__builtin_fmaxf(x, 0.0f); lo += (double)__builtin_fmaxf(-x, 0.0f); }
                else { hi += __builtin_fmax(x, 0.0); lo += __builtin_fmax(-x, 0.0); }
                if (save_mm && (uint32_t)j < own_n) mmE[own_k0 + j] = m[j];
            }
            if constexpr (W) {   // (an entry past the last: the first entry's slot and weight again — the same pair once more)
                const REAL slo = REAL(lo), shi = REAL(hi);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    P2 pr;
                    pr.x = own_w[j] * slo;
                    pr.y = own_w[j] * shi;
                    lds_st<P2>(dyn_lds, own_a[j], pr);
                }
            } else {
            const P2 pr = mean_pair(lo, hi, own_n);
#pragma unroll
            for (int j = 0; j < 4; ++j) lds_st<P2>(dyn_lds, own_a[j], pr);
            }
        } else if (own_n > 4) {
            generic(v_own);
        }
        for (uint32_t v = tid + NT; v < sm.n_vars; v += NT) generic(v);
    };

    // RECORD: this wave's pack -> the record of iteration k; `mid`: behind the forward sweep.  The caller's barrier follows (the exchange
    // behind it overwrites the differences).
    auto record = [&](uint32_t k, bool mid) {
        if constexpr (RECORD) {
            if (!has_pack) return;
            P2* const cg = reinterpret_cast<P2*>(mid ? rec->c1(k) : rec->c(k)) + layer0;
            REAL* const dg = (mid ? rec->mm1(k) : rec->dm(k)) + layer0;
            REAL* const pg = (mid ? rec->F(k) : rec->T(k)) + slot0;
            for (uint32_t j = (uint32_t)lane; j < nlayers; j += 64u) {
                cg[j] = lds_ld<P2>(dyn_lds, wbC + j * (uint32_t)sizeof(P2));
                dg[j] = lds_ld<REAL>(dyn_lds, db + j * (uint32_t)sizeof(P2));
            }
            for (uint32_t j = (uint32_t)lane; j < nslots; j += 64u) pg[j] = lds_ld<REAL>(dyn_lds, (mid ? wbF : wb) + j * S);
        }
    };
    // The history step behind a backward sweep and its barrier; `tracked`: the steps of the call before this one.  The caller's barrier follows.
    auto history = [&](uint32_t tracked) {
        if constexpr (HISTORY) {
            // (the thread's indices through opaque registers: whatever this step derives from them — addresses into the caller's arrays, the
            // root's LDS address — is computed here, not hoisted in front of the iterations, where it would stay live through the solve
            // sweeps and cost the records-in-L2 instantiation of 16 waves its last registers)
            uint32_t ht = tid, hl = (uint32_t)lane;
            asm volatile("" : "+v"(ht), "+v"(hl));
            const SmallHistMem<REAL>* hm = hs->mem;   // likewise: its fields by scalar loads, here
            asm volatile("" : "+s"(hm));
            // thread b's BDD: where its root's cost-to-terminal lies in LDS, and the bounds of the two history steps before — kept in
            // global memory between the steps (and so across launches), not in registers that would live through the solve sweeps;
            // requested here, used behind the pack's pass
            const bool hb_own = ht < hm->n_bdds;
            uint32_t hb_addr = 0;
            REAL hb_second = REAL(0), hb_third = REAL(0);
            if (hb_own) {
                const uint32_t slot = hm->root_slot[ht];
                uint32_t q = 0;
                for (uint32_t k = 1; k < sm.n_packs; ++k)
                    if (slot - sm.pack_hdr[8 * (size_t)k] < sm.pack_hdr[8 * (size_t)k + 1]) q = k;   // the pack whose slot range holds the root
                hb_addr = sm.off_regions + q * region + (slot - sm.pack_hdr[8 * (size_t)q]) * S;
                if (tracked >= 1) hb_second = hm->lb_state[ht];
                if (tracked >= 2) hb_third = hm->lb_state[hm->n_bdds + ht];
            }
            if (has_pack) {
                // the decisions per layer in the .y of the layer's staging pair (0 where no node of the layer is on the path, as the memset
                // of the solution buffer leaves it); the on-path marks of a hop's nodes in the 64 dummy entries behind the costs-from-root,
                // indexed by the slot modulo 64: this pass pushes into no dummy entry
                constexpr uint32_t P2S = (uint32_t)sizeof(P2);
                const uint32_t mk = wbF + sm.ns * S, f_end = res2_f_off(S, sm.ns) + sm.ns * S;
                for (uint32_t o = hl; o < sm.ns; o += 64u) lds_st<REAL>(dyn_lds, wbF + o * S, INF);
                lds_st<REAL>(dyn_lds, mk + hl * S, REAL(0));
                for (uint32_t j = hl; j < nlayers; j += 64u) lds_st<REAL>(dyn_lds, db + j * P2S + S, REAL(0));
                wave_sync();
                for (uint32_t h = 0; h < nh; ++h) {
                    const u4v r = RL ? lds_ld<u4v>(dyn_lds, rlane + h * 1024u) : __builtin_amdgcn_raw_buffer_load_b128(rr, hl * 16u, (rbase + h * 64u) * 16u, 0);
                    const bool real = RL ? (r[2] & 0xFFFFu) != ll_dummy : r[3] != RES2_PAD;
                    const uint32_t ll = r[2] & 0xFFFFu, fs = r[2] >> 16;
                    const uint32_t own_mark = mk + ((fs / S) & 63u) * S;
                    // every node of hop 0 is a root: cost-from-root 0 and on the path (flush_costs_from_root; FWD_SOLUTION's `j == rt`)
                    const REAL f = h == 0 ? (real ? REAL(0) : INF) : lds_ld<REAL>(dyn_lds, wbF + fs);
                    const bool on = real && (h == 0 || lds_ld<REAL>(dyn_lds, own_mark) != REAL(0));
                    const REAL tl = lds_ld<REAL>(dyn_lds, wb + (r[0] & 0xFFFFu)), th = lds_ld<REAL>(dyn_lds, wb + (r[0] >> 16));
                    const P2 cc = lds_ld<P2>(dyn_lds, wbC + ll);
                    if (on) lds_st<REAL>(dyn_lds, own_mark, REAL(0));   // (before the marks of the next hop: its slots may have the same index)
                    wave_sync();
                    // compute_bdd_sol_func as FWD_SOLUTION evaluates it (kernels/narrow.hpp): this parenthesisation, not the solve sweeps'
                    const REAL hi_path = f + (th + cc.y);
                    const REAL lo_path = f + (tl + cc.x);
                    const bool take_lo = (hi_path - lo_path) > 0;
                    if (on) {
                        lds_st<REAL>(dyn_lds, db + ll + S, take_lo ? REAL(0) : REAL(1));
                        const uint32_t ct = take_lo ? (r[0] & 0xFFFFu) : (r[0] >> 16);   // the child taken: its slot, or a sink's entry
                        if (ct < sm.ns * S) lds_st<REAL>(dyn_lds, mk + ((ct / S) & 63u) * S, REAL(1));
                    }
                    // the pushes; into a sink or from a padding lane: +inf into the lane's own slot (a padding lane's is a mark: min(mark, +inf))
                    const uint32_t plo = r[1] & 0xFFFFu, phi = r[1] >> 16;
                    const bool blo = plo < f_end, bhi = phi < f_end;
                    lds_min(reinterpret_cast<REAL*>(dyn_lds + (blo ? wb + plo : wbF + fs)), blo ? f + cc.x : INF);
                    lds_min(reinterpret_cast<REAL*>(dyn_lds + (bhi ? wb + phi : wbF + fs)), bhi ? f + cc.y : INF);
                    wave_sync();
                }
                // sol_avg: copied at the first step of a call, the moving average afterwards (bdd_cuda_learned_mma.cu:217-222)
                REAL* const so = hm->sol_avg + layer0;
                for (uint32_t j = hl; j < nlayers; j += 64u) {
                    const REAL x = lds_ld<REAL>(dyn_lds, db + j * P2S + S);
                    so[j] = tracked == 0 ? x : small_ema(so[j], x, hm->beta);
                }
            }
            // the per-BDD bounds (:224-252): the change against the step before, the change of the change, then the bounds rotate
            if (hb_own) {
                const REAL lb_last = lds_ld<REAL>(dyn_lds, hb_addr);
                if (tracked >= 1) {
                    REAL chg = lb_last - hb_second;
                    REAL* const o1 = hm->lb_first + ht;
                    if (tracked == 1) {
                        *o1 = chg;
                    } else {
                        *o1 = small_ema(*o1, chg, hm->beta);
                        const REAL prev_chg = hb_second - hb_third;
                        chg = chg - prev_chg;
                        REAL* const o2 = hm->lb_second + ht;
                        *o2 = tracked == 2 ? chg : small_ema(*o2, chg, hm->beta);
                    }
                }
                hm->lb_state[hm->n_bdds + ht] = hb_second;
                hm->lb_state[ht] = lb_last;
            }
        }
    };
    constexpr std::integral_constant<bool, false> PLAIN_EX{};
    constexpr std::integral_constant<bool, LEARNED> ITER_EX{};
    uint32_t it = 0;
    for (; it < n_iters; ++it) {
        if constexpr (RECORD) {
            record(it, false);
            __syncthreads();
        }
        if constexpr (LEARNED) {   // forward_iteration_learned_mm_dist: the weighted exchange of the deferred differences in front of the sweep
            exchange(false, ITER_EX);
            __syncthreads();
        }
        // ---------------------------------------------------------------- forward solve sweep (k_fwd_res2's hop, state in LDS)
#ifdef BDDMMA_EXP_SMALL_SKIP   // timing experiments only (wrong results): bit 0 forward sweep, 1 first exchange, 2 backward sweep, 3 second exchange, 4 bound
        if (has_pack && !(BDDMMA_EXP_SMALL_SKIP & 1)) {
#else
        if (has_pack) {
#endif
            for (uint32_t o = (uint32_t)lane; o < sm.ns + 64u; o += 64u) lds_st<REAL>(dyn_lds, wbF + o * S, INF);  // costs-from-root and the dummy entries
            wave_sync();
            auto hop = [&](const u4v& r) {
                const uint32_t ll = r[2] & 0xFFFFu, fs = r[2] >> 16;
                const REAL f = lds_ld<REAL>(dyn_lds, wbF + fs);
                const REAL tl = lds_ld<REAL>(dyn_lds, wb + (r[0] & 0xFFFFu)), th = lds_ld<REAL>(dyn_lds, wb + (r[0] >> 16));
                const P2 cc = lds_ld<P2>(dyn_lds, wbC + ll);
                const P2 dd = lds_ld<P2>(dyn_lds, db + ll);
                REAL m0 = (f + cc.x) + tl, m1 = (f + cc.y) + th;  // padding lanes: +inf
                pair_min_aligned(m0, m1, RL ? (int32_t)r[3] < 0 : (r[3] & 0x10000u) != 0);
                const REAL mm = mm_diff1(m0, m1, LEARNED ? lds_ld<REAL>(dyn_lds, ob + (ll >> 1)) : omega);
                P2 nc;
                nc.x = (cc.x + min0(mm)) + dd.x;
                nc.y = (cc.y + min0_neg(mm)) + dd.y;
                if constexpr (RL) {   // rewritten records: every lane stores (both lanes of a layer the same pair; padding lanes the dummy pair)
                    lds_st<P2>(dyn_lds, wbC + ll, nc);
                    lds_st<REAL>(dyn_lds, db + ll, mm);
                } else {
                    const bool real = r[3] != RES2_PAD;
                    if ((r[3] & 0xFFFFu) != RES2_NO_STORE && real) lds_st<P2>(dyn_lds, wbC + ll, nc);  // the layer's head: new arc costs (every lane of the layer has read the old ones)
                    if (real) lds_st<REAL>(dyn_lds, db + ll, mm);                                       // every lane of a layer holds the same value
                }
                lds_min(reinterpret_cast<REAL*>(dyn_lds + wb + (r[1] & 0xFFFFu)), f + nc.x);        // sinks / padding: the lane's own dummy entry
                lds_min(reinterpret_cast<REAL*>(dyn_lds + wb + (r[1] >> 16)), f + nc.y);
                wave_sync();
            };
            if constexpr (RL) {
                // records in LDS: one hop ahead is all the distance an LDS read needs; the record behind the pack's last hop is the spare KiB of
                // its record area (never used)
                uint32_t ra = rlane;
                u4v ra_rec = lds_ld<u4v>(dyn_lds, ra), rb_rec;
                if ((ra_rec[2] & 0xFFFFu) != ll_dummy) lds_st<REAL>(dyn_lds, wbF + (ra_rec[2] >> 16), REAL(0));  // every node of hop 0 is a root (flush_costs_from_root)
                wave_sync();
                for (uint32_t h = 0; h < nh; h += 2) {
                    rb_rec = lds_ld<u4v>(dyn_lds, ra + 1024u);
                    hop(ra_rec);
                    if (h + 1 >= nh) break;
                    ra_rec = lds_ld<u4v>(dyn_lds, ra + 2048u);
                    hop(rb_rec);
                    ra += 2048u;
                }
            } else {
                auto ldrec = [&](uint32_t h) -> u4v { return __builtin_amdgcn_raw_buffer_load_b128(rr, (uint32_t)lane * 16u, (rbase + h * 64u) * 16u, 0); };
                u4v r0 = ldrec(0), r1 = ldrec(1), r2 = ldrec(2), r3 = ldrec(3), r4 = ldrec(4), r5 = ldrec(5), r6 = ldrec(6), r7 = ldrec(7);
                if (r0[3] != RES2_PAD) lds_st<REAL>(dyn_lds, wbF + (r0[2] >> 16), REAL(0));  // every node of hop 0 is a root (flush_costs_from_root)
                wave_sync();
#define SMALL_HOP(RK, HK)           \
    hop(RK);                        \
    RK = ldrec(h + (HK) + 8);       \
    if (h + (HK) + 1 >= nh) break;
                for (uint32_t h = 0; h < nh; h += 16) {
                    SMALL_HOP(r0, 0) SMALL_HOP(r1, 1) SMALL_HOP(r2, 2) SMALL_HOP(r3, 3) SMALL_HOP(r4, 4) SMALL_HOP(r5, 5) SMALL_HOP(r6, 6) SMALL_HOP(r7, 7)
                    SMALL_HOP(r0, 8) SMALL_HOP(r1, 9) SMALL_HOP(r2, 10) SMALL_HOP(r3, 11) SMALL_HOP(r4, 12) SMALL_HOP(r5, 13) SMALL_HOP(r6, 14) SMALL_HOP(r7, 15)
                }
            }
        }
        __syncthreads();
        if constexpr (RECORD) {
            record(it, true);
            __syncthreads();
        }
#ifdef BDDMMA_EXP_SMALL_SKIP
        if (!(BDDMMA_EXP_SMALL_SKIP & 2))
#endif
        exchange(false, ITER_EX);
        __syncthreads();
        // ---------------------------------------------------------------- backward solve sweep (k_bwd_res2's hop)
#ifdef BDDMMA_EXP_SMALL_SKIP
        if (has_pack && !(BDDMMA_EXP_SMALL_SKIP & 4)) {
#else
        if (has_pack) {
#endif
            auto hop = [&](const u4v& r) {
                const uint32_t ll = r[2] & 0xFFFFu, fs = r[2] >> 16;
                const REAL f = lds_ld<REAL>(dyn_lds, wbF + fs);  // padding lanes: whatever the dummy entry holds; their results go nowhere
                const REAL tl = lds_ld<REAL>(dyn_lds, wb + (r[0] & 0xFFFFu)), th = lds_ld<REAL>(dyn_lds, wb + (r[0] >> 16));
                const P2 cc = lds_ld<P2>(dyn_lds, wbC + ll);
                const P2 dd = lds_ld<P2>(dyn_lds, db + ll);
                REAL m0 = (f + cc.x) + tl, m1 = (f + cc.y) + th;
                pair_min_aligned(m0, m1, RL ? (int32_t)r[3] < 0 : (r[3] & 0x10000u) != 0);
                const REAL mm = mm_diff1(m0, m1, LEARNED ? lds_ld<REAL>(dyn_lds, ob + (ll >> 1)) : omega);
                P2 nc;
                nc.x = (cc.x + min0(mm)) + dd.x;
                nc.y = (cc.y + min0_neg(mm)) + dd.y;
                const REAL t = rmin(nc.y + th, nc.x + tl);
                if constexpr (RL) {   // rewritten records: no exec masks (padding lanes: the dummy pair, the spare entry ns + 2)
                    lds_st<P2>(dyn_lds, wbC + ll, nc);
                    lds_st<REAL>(dyn_lds, db + ll, mm);
                    lds_st<REAL>(dyn_lds, wb + fs, t);
                } else {
                    const bool real = r[3] != RES2_PAD;
                    if ((r[3] & 0xFFFFu) != RES2_NO_STORE && real) lds_st<P2>(dyn_lds, wbC + ll, nc);
                    if (real) {
                        lds_st<REAL>(dyn_lds, db + ll, mm);
                        lds_st<REAL>(dyn_lds, wb + fs, t);
                    }
                }
                wave_sync();
            };
            if constexpr (RL) {
                // from the pack's last hop upwards; the record read "before" hop 0 lies in front of the record area (any LDS contents, never used)
                uint32_t ra = rlane + nhm1 * 1024u;
                u4v ra_rec = lds_ld<u4v>(dyn_lds, ra), rb_rec;
                for (uint32_t k = 0; k < nh; k += 2) {
                    rb_rec = lds_ld<u4v>(dyn_lds, ra - 1024u);
                    hop(ra_rec);
                    if (k + 1 >= nh) break;
                    ra_rec = lds_ld<u4v>(dyn_lds, ra - 2048u);
                    hop(rb_rec);
                    ra -= 2048u;
                }
            } else {
                // k-th hop processed = hop nh - 1 - k of the pack; past the first hop: any record (never used)
                auto ldrec = [&](uint32_t k) -> u4v {
                    const uint32_t h = k < nhm1 ? nhm1 - k : 0u;
                    return __builtin_amdgcn_raw_buffer_load_b128(rr, (uint32_t)lane * 16u, (rbase + h * 64u) * 16u, 0);
                };
                u4v r0 = ldrec(0), r1 = ldrec(1), r2 = ldrec(2), r3 = ldrec(3), r4 = ldrec(4), r5 = ldrec(5), r6 = ldrec(6), r7 = ldrec(7);
                for (uint32_t h = 0; h < nh; h += 16) {  // h counts the hops processed, from the pack's last hop upwards
                    SMALL_HOP(r0, 0) SMALL_HOP(r1, 1) SMALL_HOP(r2, 2) SMALL_HOP(r3, 3) SMALL_HOP(r4, 4) SMALL_HOP(r5, 5) SMALL_HOP(r6, 6) SMALL_HOP(r7, 7)
                    SMALL_HOP(r0, 8) SMALL_HOP(r1, 9) SMALL_HOP(r2, 10) SMALL_HOP(r3, 11) SMALL_HOP(r4, 12) SMALL_HOP(r5, 13) SMALL_HOP(r6, 14) SMALL_HOP(r7, 15)
                }
            }
#undef SMALL_HOP
            // lower bound contribution of this pack: sum of root costs-from-terminal (bdd_cuda_base.cu:1243-1251); every node of the first hop is a root
            if ((!LEARNED && run.ctl != nullptr) || STOP || it + 1 == n_iters) {   // (uniform) the bound: run_solver's tests, the stopping rule, or the state the launch leaves
            const u4v rroot = RL ? lds_ld<u4v>(dyn_lds, rl + (uint32_t)lane * 16u) : __builtin_amdgcn_raw_buffer_load_b128(rr, (uint32_t)lane * 16u, rbase * 16u, 0);
            double lb = (RL ? (rroot[2] & 0xFFFFu) != ll_dummy : rroot[3] != RES2_PAD) ? (double)lds_ld<REAL>(dyn_lds, wb + (rroot[2] >> 16)) : 0.0;
            for (int off2 = 32; off2 > 0; off2 >>= 1) lb += __shfl_down(lb, off2);
            if (lane == 0) lbp[p] = lb;
            }
        }
        __syncthreads();
        if constexpr (HISTORY && STOP) {
            if (__builtin_amdgcn_readfirstlane(ws->trk[it & 1u]) != 0u) {   // (uniform) tracked: the tail window, or converged by an earlier iteration's test
                history(__builtin_amdgcn_readfirstlane(ws->step[it & 1u]));
                __syncthreads();   // the next exchange writes the staging pairs of every pack
            }
        } else if constexpr (HISTORY) {
            if (it >= hs->hist_from) {   // (uniform)
                history(hs->tracked + (it - hs->hist_from));
                __syncthreads();   // the next exchange writes the staging pairs of every pack
            }
        }
        if constexpr (STOP) {
            if (wave == 0) {
                // the bound of the iteration in the shape of k_lb_reduce, then SolverT::learned_iterations' lines behind its history step
                double t = (uint32_t)lane < sm.n_packs ? lbp[lane] : 0.0;
                for (int off2 = 32; off2 > 0; off2 >>= 1) t += __shfl_down(t, off2);
                if (lane == 0) {
                    const uint64_t g = ws->iters, num_itr = ws->num_itr, cfi = ws->cfi;
                    const uint64_t tracked = ws->tracked + ws->trk[it & 1u];
                    const double lb_prev = ws->lb_post;
                    double initial = ws->initial;
                    if (g == 0 && !(__builtin_fabs(initial) < __builtin_huge_val())) initial = __builtin_fabs(lb_prev - t);   // set_initial_lb_change: once per solver (lb_prev is the bound on entry)
                    uint32_t conv = ws->converged;
                    if (conv == 0u && __builtin_fabs(lb_prev - t) < ws->slope * initial) conv = 1u;
                    const bool stop = conv != 0u && tracked == cfi;
                    ws->lb_post = t;
                    ws->initial = initial;
                    ws->tracked = tracked;
                    ws->iters = g + 1;
                    ws->converged = conv;
                    ws->stop = stop ? 1u : 0u;
                    ws->trk[(it + 1u) & 1u] = (cfi > 0 && (cfi >= num_itr - (g + 1) || conv != 0u)) ? 1u : 0u;
                    ws->step[(it + 1u) & 1u] = (uint32_t)(tracked < 3 ? tracked : 3);
                    if (stop || it + 1 == n_iters) {   // the block for the call's next launch, or for the host
                        SmallStopBlock* const b = *stp;
                        b->lb_prev = lb_prev;
                        b->lb_post = t;
                        b->initial_change = initial;
                        b->tracked = tracked;
                        b->iters = g + 1;
                        b->converged = conv;
                        b->done = (stop || g + 1 == num_itr) ? 1u : 0u;
                    }
                }
            }
            // A barrier of its own: the next use of the decision is the choice between the next iteration's weighted exchange and the exit
            // exchange, and the former overwrites the differences the latter reads — it cannot wait for that iteration's first barrier.
            __syncthreads();
            if (__builtin_amdgcn_readfirstlane(ws->stop) != 0u) { ++it; break; }   // (uniform) the iteration that stopped is complete
        }
        if constexpr (!LEARNED) {
#ifdef BDDMMA_EXP_SMALL_SKIP
        if (!(BDDMMA_EXP_SMALL_SKIP & 8))
#endif
        exchange(true, PLAIN_EX);
        if (run.ctl != nullptr && wave == 0) {
            // the bound of the iteration in the shape of k_lb_reduce / run_ctl_step (<= 64 partial sums: lane i holds pack i's, an in-wave tree,
            // the other fifteen partial results are 0) and run_solver's tests
            double t = (uint32_t)lane < sm.n_packs ? lbp[lane] : 0.0;
            for (int off2 = 32; off2 > 0; off2 >>= 1) t += __shfl_down(t, off2);
            if (lane == 0) {
                // (the bounds are published to the host — a system-scope fence, ~2 us of PCIe round trip — with the launch's last iteration or
                // the one that stops the run; in between they are only written to the ring)
                const uint32_t reason = run_ctl_finish(run, c, t, it + 1 == n_iters);
                if (c.iter == 0) c.lb_first = t;
                c.lb_post = t;
                c.iter += 1;
                flag[0] = reason;
            }
        }
        __syncthreads();
        if (run.ctl != nullptr && flag[0] != 0) { ++it; break; }  // uniform: the iteration that met a criterion is complete
        }
    }
    (void)it;
    if constexpr (RECORD) {
        record(n_iters, false);
        __syncthreads();
    }
    if constexpr (LEARNED) {   // the exit state: the last backward pass's differences deferred, delta their isotropic exchange
        exchange(true, PLAIN_EX);
        __syncthreads();
    }
    // ---- epilogue: the state -> global memory, as the last iteration's four launches would have left it
    if (has_pack) {
        for (uint32_t j = (uint32_t)lane; j < nslots; j += 64) {
            d.T[slot0 + j] = lds_ld<REAL>(dyn_lds, wb + j * S);
            d.F[slot0 + j] = lds_ld<REAL>(dyn_lds, wbF + j * S);
        }
        for (uint32_t j = (uint32_t)lane; j < nlayers; j += 64)
            reinterpret_cast<P2*>(d.lohi)[layer0 + j] = lds_ld<P2>(dyn_lds, wbC + j * (uint32_t)sizeof(P2));
        if (lane == 0) d.lb_partial[pk.lb_base + p] = lbp[p];
    }
    for (uint32_t k = tid; k < sm.n_entries; k += NT) d.mm_binned[sm.var_ent[k]] = mmE[k];   // the deferred differences of the last backward sweep
    {
        const P2* const sD = reinterpret_cast<const P2*>(dyn_lds);
        for (uint32_t q = 0; q < sm.n_quads; ++q) {
            const uint32_t c0 = sm.quad_hdr[4 * (size_t)q], cnt = sm.quad_hdr[4 * (size_t)q + 1];
            for (uint32_t i = tid; i < cnt; i += NT) {
                const uint32_t e = d.cs_entry[c0 + i], sl = d.cs_slot[c0 + i];
                const_cast<P2*>(reinterpret_cast<const P2*>(d.delta_lay))[e] = sD[(size_t)(q * sm.wpb + sl / pk.stage_cap) * small_stage_stride(sm.nl) + sl % pk.stage_cap];
            }
        }
    }
}

template <typename REAL, int NW, bool RL>
__global__ void __launch_bounds__(64 * NW) k_iterate_small(SmallDev sm, DevPtrs<REAL> d, PackDev pk, REAL omega, uint32_t n_iters, RunStep run)
{
    small_iterate<REAL, NW, RL>(sm, d, pk, omega, n_iters, run);
}

// A batch of such instances in one launch (solver_bt.hpp): workgroup b runs instance items[b], which holds what k_iterate_small takes by
// value.  No workgroup talks to another.  The item's address is uniform and the array is read-only for the launch, so its fields arrive
// by scalar loads as kernel arguments do.  Every member of a launch has the same NW and RL; the dynamic LDS is the largest member's.
template <typename REAL>
struct SmallItem {
    SmallDev sm;
    DevPtrs<REAL> d;
    PackDev pk;
    RunStep run;
};
template <typename REAL, int NW, bool RL>
__global__ void __launch_bounds__(64 * NW) k_iterate_small_batch(const SmallItem<REAL>* __restrict__ items, REAL omega, uint32_t n_iters)
{
    const SmallItem<REAL>& item = items[blockIdx.x];
    small_iterate<REAL, NW, RL>(item.sm, item.d, item.pk, omega, n_iters, item.run);
}
// The learned form of both (SolverT::launch_small_learned, BatchT::learned_iterations); instantiated in solver_sl_f32.hip / _f64.hip only.
template <typename REAL, int NW, bool RL>
__global__ void __launch_bounds__(64 * NW) k_learned_small(SmallDev sm, DevPtrs<REAL> d, PackDev pk, SmallLearn<REAL> ln, REAL omega, uint32_t n_iters)
{
    small_iterate<REAL, NW, RL, true>(sm, d, pk, omega, n_iters, RunStep{}, &ln);
}
template <typename REAL>
struct SmallLearnItem {
    SmallDev sm;
    DevPtrs<REAL> d;
    PackDev pk;
    SmallLearn<REAL> ln;
};
// use_ov = 0: the scalar omega for every member (the items keep the address of each member's omega_lay)
template <typename REAL, int NW, bool RL>
__global__ void __launch_bounds__(64 * NW) k_learned_small_batch(const SmallLearnItem<REAL>* __restrict__ items, REAL omega, uint32_t n_iters, uint32_t use_ov)
{
    const SmallLearnItem<REAL>& item = items[blockIdx.x];
    SmallLearn<REAL> ln = item.ln;
    if (!use_ov) ln.omega_lay = nullptr;
    small_iterate<REAL, NW, RL, true>(item.sm, item.d, item.pk, omega, n_iters, RunStep{}, &ln);
}
// The arguments of one batch call in one launch: workgroup b checks member b's dist_weights (and omega_vec) and moves them where its
// workgroup of k_learned_small_batch reads them — the weights layer -> binned entry order through lpos (k_layers_to_entries), omega_vec as
// it is (layer order).  bad[0] / bad[1]: the smallest member index with a weight / an omega that is negative or not finite (the caller
// presets both to 0xFFFFFFFF).
template <typename REAL>
struct LearnLoad {
    const uint32_t* lpos;
    REAL* alpha_ent;
    REAL* omega_lay;
    uint32_t src, n;   // first value of the member in the concatenated inputs, values
};
template <typename REAL>
__global__ void k_batch_learn_load(const LearnLoad<REAL>* __restrict__ tab, const REAL* __restrict__ w, const REAL* __restrict__ ov, uint32_t* __restrict__ bad)
{
    const LearnLoad<REAL> t = tab[blockIdx.x];
    bool bw = false, bo = false;
    for (uint32_t l = threadIdx.x; l < t.n; l += blockDim.x) {
        const REAL a = w[t.src + l];
        bw |= !(a >= REAL(0) && a < REAL(__builtin_huge_val()));   // NaN fails both tests
        t.alpha_ent[t.lpos[l]] = a;
        if (ov != nullptr) {
            const REAL o = ov[t.src + l];
            bo |= !(o >= REAL(0) && o < REAL(__builtin_huge_val()));
            t.omega_lay[l] = o;
        }
    }
    if (bw) atomicMin(bad, blockIdx.x);
    if (bo) atomicMin(bad + 1, blockIdx.x);
}
// What changes between the launches of a batch, written into the items on the device (in stream order, so no launch sees half an update):
// the run_solver gate and control block of each item — `ctl` null: outside run_solver — and the index of the launch's first iteration.
template <typename REAL>
__global__ void k_small_items_refresh(SmallItem<REAL>* items, uint32_t n, RunCtl* ctl, RunHost* host, uint32_t run_iter)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    items[i].d.stop = ctl != nullptr ? &ctl[i].stop : nullptr;
    items[i].d.run_iter = run_iter;
    items[i].run.ctl = ctl != nullptr ? ctl + i : nullptr;
    items[i].run.host = ctl != nullptr ? host + i : nullptr;
}
// k_run_begin for every control block of a batch: one clock for all of them
static __global__ void k_run_begin_batch(RunCtl* ctl, uint32_t n, uint64_t host_ticks_so_far)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) ctl[i].t0 = __builtin_amdgcn_s_memrealtime() - host_ticks_so_far;
}

}  // namespace bddmma
