// kernels/summarg.hpp — the sweeps in the (log-sum-exp, +) semiring: sum-marginals (bdd_cuda_base.cu:788-1025, sum_marginals_cuda).
// The two kernels are instantiated by solver_sm.hpp only (translation units solver_sm_f32.hip / solver_sm_f64.hip); their bodies also run
// inside k_small_summarg_batch (kernels/batchsm.hpp).  Behind kernels.hpp.
//
// Two pull sweeps (kernels/pull.hpp: one launch per pack family, one workgroup per pack; the skeleton of a hop and the fixed orders of
// its folds are written there):
//   forward   F~[n] = logsumexp over the parents p of n (F~[p] - cost of the arc p -> n), roots 0.  A sum cannot be pushed the way the
//             minimum is (lds_min), so a node PULLS: every node of a hop leaves F~ - lo and F~ - hi in two LDS arrays, and a node of the
//             next hop walks its parents, maximum first, then the sum of exp(x - max).
//   backward  T~[n] = logaddexp(T~[lo] - lo, T~[hi] - hi) by pull (top sink 0, bottom sink -inf), and in the same hop the two path values
//             F~[n] + (T~[child] - cost) go to LDS and are reduced per layer by two layer folds, first the maximum, then the sum of
//             exp(x - max) with every node computing its own exp.
#pragma once
#include "pull.hpp"

namespace bddmma {

__device__ __forceinline__ float sm_exp(float x) { return expf(x); }   // OCML, full accuracy (not __expf)
__device__ __forceinline__ double sm_exp(double x) { return exp(x); }
__device__ __forceinline__ float sm_log(float x) { return logf(x); }
__device__ __forceinline__ double sm_log(double x) { return log(x); }
__device__ __forceinline__ float sm_log1p(float x) { return log1pf(x); }
__device__ __forceinline__ double sm_log1p(double x) { return log1p(x); }
__device__ __forceinline__ float rmax(float a, float b) { return __builtin_fmaxf(a, b); }
__device__ __forceinline__ double rmax(double a, double b) { return __builtin_fmax(a, b); }

// log(exp(a) + exp(b)); -inf where both are
template <typename REAL>
__device__ __forceinline__ REAL sm_logaddexp(REAL a, REAL b)
{
    const REAL m = rmax(a, b), n = rmin(a, b);
    if (!(m > -inf_v<REAL>())) return -inf_v<REAL>();
    return m + sm_log1p(sm_exp(n - m));
}
// m + log(s) of a maximum and the sum of exp(x - m); -inf for the empty sum
template <typename REAL>
__device__ __forceinline__ REAL sm_finish(REAL m, REAL s)
{
    return m > -inf_v<REAL>() ? m + sm_log(s) : -inf_v<REAL>();
}

// LDS of a pack of width ww: forward 4 arrays of ww values; backward 7 arrays of values + 1 of layer indices (huge packs: the same in a
// global scratch of their own, SolverT::d_sm_scratch)
__host__ __device__ inline size_t sm_lds_bytes(size_t real_size, uint32_t ww) { return (7 * real_size + 4) * (size_t)ww; }


// The sweeps' bodies for the pack `pc`: k_sm_fwd / k_sm_bwd run them with the workgroup's pack and PullBlockBar (__syncthreads()) as BAR,
// k_small_summarg_batch (kernels/batchsm.hpp) with a wave's pack and a wave-level ordering point.
// (par_ptr / par: kernels/pull.hpp, pull_parents)
template <typename REAL, bool NARROW, typename BAR>
__device__ __forceinline__ void sm_fwd_body(const DevPtrs<REAL>& d, const PackDev& pk, const PullPack<REAL>& pc, const uint32_t* par_ptr, const uint32_t* par,
                                            uint32_t ww)
{
    REAL* const A = pc.base;  // [hop parity][arc][slot]
    const REAL NINF = -inf_v<REAL>();
    uint32_t cur = 0;
    for (uint32_t q = pc.q0; q < pc.q1; ++q, cur ^= 1u) {
        const uint32_t nb = pk.hop_node_off[q], n = pk.hop_node_off[q + 1] - nb, lbase = pk.hop_layer_off[q];
        const uint32_t rt = (pk.hop_root != nullptr && q > pc.q0) ? (uint32_t)pk.hop_root[q] : (uint32_t)NO_ROOT;  // a BDD that starts at this hop
        REAL* const Ac = A + (size_t)cur * 2 * ww;
        const REAL* const Ap = A + (size_t)(cur ^ 1u) * 2 * ww;
        pull_slots<REAL, NARROW, false>(d, pc, nb, n, lbase, nullptr, [&](uint32_t j, uint32_t wi, const PullNode& nd) {
            REAL f = REAL(0);  // roots (flush_costs_from_root)
            if (!(q == pc.q0 || j == rt)) {
                REAL m = NINF;
                pull_parents(par_ptr, par, wi, [&](uint32_t slot, uint32_t arc) { m = rmax(m, Ap[(size_t)arc * ww + slot]); });
                REAL s = REAL(0);
                if (m > NINF) pull_parents(par_ptr, par, wi, [&](uint32_t slot, uint32_t arc) { s += sm_exp(Ap[(size_t)arc * ww + slot] - m); });
                f = sm_finish(m, s);
            }
            Ac[j] = f - d.lohi[2 * (size_t)nd.layer];
            Ac[ww + j] = f - d.lohi[2 * (size_t)nd.layer + 1];
            d.F[nb + j] = f;
        });
        BAR::sync();  // this hop's values before the next hop's pulls; the next hop writes the other parity
    }
}

template <typename REAL, bool NARROW, bool GLOBAL>
__global__ void __launch_bounds__(NARROW ? 64 : WIDE_THREADS) k_sm_fwd(DevPtrs<REAL> d, PackDev pk, const uint32_t* par_ptr, const uint32_t* par, uint32_t ww,
                                                                       unsigned char* scratch)
{
    if (blockIdx.x >= pk.n_packs) return;
    const PullPack<REAL> pc = pull_pack<REAL, NARROW, GLOBAL>(d, pk, ww, scratch, sm_lds_bytes(sizeof(REAL), ww));
    sm_fwd_body<REAL, NARROW, PullBlockBar>(d, pk, pc, par_ptr, par, ww);
}

// (the parent tables are not read: the leading arguments are those of every pull sweep)
template <typename REAL, bool NARROW, typename BAR>
__device__ __forceinline__ void sm_bwd_body(const DevPtrs<REAL>& d, const PackDev& pk, const PullPack<REAL>& pc, const uint32_t*, const uint32_t*, uint32_t ww)
{
    REAL* const Tb = pc.base;                   // [hop parity][slot]: T~
    REAL* const P0 = pc.base + 2 * (size_t)ww;  // path values through the lo arc per slot, then exp(value - the layer's maximum)
    REAL* const P1 = pc.base + 3 * (size_t)ww;  // ... the hi arc
    REAL* const Q0 = pc.base + 4 * (size_t)ww;  // per run (at its first slot): the run's maximum, then its sum
    REAL* const Q1 = pc.base + 5 * (size_t)ww;
    REAL* const M1 = pc.base + 6 * (size_t)ww;  // per layer of the hop: the maximum of the hi values (lo: in the children's T~, dead by then)
    uint32_t* const Lid = reinterpret_cast<uint32_t*>(pc.base + 7 * (size_t)ww);  // hop-local layer of the slot, PULL_NO_LAYER for padding
    const REAL NINF = -inf_v<REAL>();
    const auto path = [&](uint32_t j) { return Pull2<REAL>{P0[j], P1[j]}; };
    const auto run = [&](uint32_t j) { return Pull2<REAL>{Q0[j], Q1[j]}; };
    const auto keep = [&](uint32_t j, Pull2<REAL> v) { Q0[j] = v.lo; Q1[j] = v.hi; };
    uint32_t cur = 0;
    for (uint32_t q = pc.q1; q-- > pc.q0; cur ^= 1u) {
        const uint32_t nb = pk.hop_node_off[q], n = pk.hop_node_off[q + 1] - nb, lbase = pk.hop_layer_off[q];
        REAL* const Tc = Tb + (size_t)cur * ww;           // this hop
        REAL* const Tn = Tb + (size_t)(cur ^ 1u) * ww;    // the hop below (children); after the pull: M0, the layers' maxima of the lo values
        REAL* const M0 = Tn;
        // ---- pull, path values
        pull_slots<REAL, NARROW, true>(d, pc, nb, n, lbase, Lid, [&](uint32_t j, uint32_t, const PullNode& nd) {
            const REAL tl = nd.lo == PULL_BOT ? NINF : (nd.lo == PULL_TOP ? REAL(0) : Tn[nd.lo]);
            const REAL th = nd.hi == PULL_BOT ? NINF : (nd.hi == PULL_TOP ? REAL(0) : Tn[nd.hi]);
            const REAL a = tl - d.lohi[2 * (size_t)nd.layer], b = th - d.lohi[2 * (size_t)nd.layer + 1];
            const REAL t = sm_logaddexp(a, b);
            const REAL f = d.F[nb + j];
            Tc[j] = t;
            d.T[nb + j] = t;
            P0[j] = f + a;
            P1[j] = f + b;
        });
        BAR::sync();
        // ---- maxima
        pull_layer_fold_bar<BAR>(pc, Lid, n, path, [](Pull2<REAL> v, Pull2<REAL> w) { return Pull2<REAL>{rmax(v.lo, w.lo), rmax(v.hi, w.hi)}; }, keep, run,
                                 [&](uint32_t l, Pull2<REAL> m) { M0[l] = m.lo; M1[l] = m.hi; });
        BAR::sync();
        // ---- exp(value - maximum), every node its own; then the sums
        for (uint32_t j = pc.tid; j < n; j += pc.T) {
            const uint32_t l = Lid[j];
            if (l != PULL_NO_LAYER) {
                const REAL m0 = M0[l], m1 = M1[l];
                P0[j] = m0 > NINF ? sm_exp(P0[j] - m0) : REAL(0);
                P1[j] = m1 > NINF ? sm_exp(P1[j] - m1) : REAL(0);
            }
        }
        BAR::sync();
        pull_layer_fold_bar<BAR>(pc, Lid, n, path, pull_add<REAL>, keep, run,
                                 [&](uint32_t l, Pull2<REAL> s) {
                                     d.mm0_out[lbase + l] = sm_finish(M0[l], s.lo);
                                     d.mm1_out[lbase + l] = sm_finish(M1[l], s.hi);
                                 });
        BAR::sync();  // the next hop overwrites every array (M0 is its T~ buffer)
    }
}

// (the leading arguments are those of every pull kernel, SolverT::launch_pull)
template <typename REAL, bool NARROW, bool GLOBAL>
__global__ void __launch_bounds__(NARROW ? 64 : WIDE_THREADS) k_sm_bwd(DevPtrs<REAL> d, PackDev pk, const uint32_t* par_ptr, const uint32_t* par, uint32_t ww,
                                                                       unsigned char* scratch)
{
    if (blockIdx.x >= pk.n_packs) return;
    const PullPack<REAL> pc = pull_pack<REAL, NARROW, GLOBAL>(d, pk, ww, scratch, sm_lds_bytes(sizeof(REAL), ww));
    sm_bwd_body<REAL, NARROW, PullBlockBar>(d, pk, pc, par_ptr, par, ww);
}

}  // namespace bddmma
