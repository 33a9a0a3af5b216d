// kernels/gradmm.hpp — the backward operator of the min-marginal differences (bdd_cuda_learned_mma.cu:623-1023, grad_mm_diff_all_hops):
// the transpose-Jacobian product of mm_diff[l] = m_hi[l] - m_lo[l], m_a[l] = min over the nodes u of l of F[u] + c_a[l] + T[child_a(u)],
// with respect to the lo / hi arc costs.  The two kernels are instantiated by solver_gr.hpp only (translation units solver_gr_f32.hip /
// solver_gr_f64.hip); their bodies also run inside k_small_grad_mm_batch (kernels/batchmm.hpp).  Behind kernels.hpp.
//
// F and T are the stored potentials of the plain sweeps.  With g the incoming gradient:
//   seeds      per layer l and arc a, at the arg-min node u*_a(l) (sign s = +1 for hi, -1 for lo):  dc_a[l] += s g[l],  dF[u*_a] += s g[l],
//              dT[child_a(u*_a)] += s g[l]; a sink takes nothing, an arc with no finite path seeds nothing.
//   through T  root -> terminal (k_gr_down): every node hands its whole dT along its arg-min arc to that child and adds it to that arc's
//              dc of its layer.
//   through F  terminal -> root (k_gr_up): every node hands its whole dF to its arg-min (parent, arc) and adds it to that arc's dc of
//              the parent's layer.
// Ties: lowest slot first among a layer's nodes, first in parent table order among parents, lo before hi (include/bdd_mma.h).
//
// Both directions are pull sweeps (kernels/pull.hpp: one launch per pack family, one workgroup per pack; the skeleton of a hop and the
// fixed orders of its folds are written there):
//   down  a node leaves in LDS what it sends along each arc, S_a[u] = (a is u's arg-min arc ? dT[u] : 0) + (u == u*_a ? s g : 0); a node
//         of the next hop sums S over its parents in parent table order.  The layer's dc is the sum of S_a over its slots.
//   up    the nodes of hop q leave F + c_a in LDS, the nodes of hop q + 1 publish their arg-min (parent, arc) from it, and every node
//         of hop q takes dF of each child that names it.  The layer's dc grows by the sum of what its nodes took per arc.
// The per-layer arg-min and the per-layer sums are layer folds (pull_layer_fold), so two calls agree bit for bit whatever the number of waves.
// k_gr_down writes grad_lo / grad_hi of every layer and the arg-min slots (arg); k_gr_up, launched behind it, adds its part.
#pragma once
#include "pull.hpp"

namespace bddmma {

constexpr uint32_t GR_NONE = 0xFFFFFFFFu;

// LDS of a pack of width ww: down 6 arrays of values + 3 of indices, up 6 + 2.  In float that is 36 bytes per slot against the 32 of
// sm_lds_bytes (double: 60 against 60), so a wide pack width that the sum-marginals just fit (above lds_cu / 36 slots, 4 551 at 160 KiB)
// is refused here with BDDMMA_ERR_UNSUPPORTED (SolverT::gr_prepare); the default wide pack width is 2 048 slots.
__host__ __device__ inline size_t gr_lds_bytes(size_t real_size, uint32_t ww) { return (6 * real_size + 12) * (size_t)ww; }

// ---- the steps of a hop that every sweep carrying dT or dF shares (the two kernels here and those of kernels/graditer.hpp): the tie rules
// of the routing are written here and nowhere else.
// T of a child: 0 at the top sink, inf at the bottom sink
template <typename REAL>
__device__ __forceinline__ REAL gr_child_T(const REAL* __restrict__ T, uint32_t nbn, uint32_t c)
{
    return c == PULL_BOT ? inf_v<REAL>() : (c == PULL_TOP ? REAL(0) : T[nbn + c]);
}
// Down: slot j's dT = dt0 + what its parents sent (parent table order; `pull` false: a root, nobody sends), and it leaves along the arc of
// the smaller of a (lo) and b (hi), lo before hi: Sc[arc][j] = dT, the other arc 0.
template <typename REAL>
__device__ __forceinline__ void gr_send_down(const uint32_t* par_ptr, const uint32_t* par, uint32_t wi, bool pull, const REAL* Sp, REAL* Sc, uint32_t ww,
                                             uint32_t j, REAL dt0, REAL a, REAL b)
{
    REAL dt = dt0;
    if (pull) pull_parents(par_ptr, par, wi, [&](uint32_t slot, uint32_t arc) { dt += Sp[(size_t)arc * ww + slot]; });
    const bool lo_arc = a <= b;  // lo before hi
    Sc[j] = lo_arc ? dt : REAL(0);
    Sc[ww + j] = lo_arc ? REAL(0) : dt;
}
// Up: the nn children (word index w0 + c) publish their arg-min (parent, arc) over V0 / V1 = F + cost of the lo / hi arc per slot of this
// hop: AP[c] = slot << 1 | arc; first in parent table order wins a tie; a root or an unreachable node names nobody (GR_NONE).
template <typename REAL>
__device__ __forceinline__ void gr_name_parents(const PullPack<REAL>& pc, const uint32_t* par_ptr, const uint32_t* par, uint32_t w0, uint32_t nn, const REAL* V0,
                                                const REAL* V1, uint32_t* AP)
{
    for (uint32_t c = pc.tid; c < nn; c += pc.T) {
        REAL m = inf_v<REAL>();
        uint32_t best = GR_NONE;
        pull_parents(par_ptr, par, w0 + c, [&](uint32_t slot, uint32_t arc) {
            const REAL v = arc ? V1[slot] : V0[slot];
            if (v < m) { m = v; best = (slot << 1) | arc; }
        });
        AP[c] = best;
    }
}
// ... and slot j takes dF (Dn) of each child that names it: {over its lo arc, over its hi arc}
template <typename REAL>
__device__ __forceinline__ Pull2<REAL> gr_take_up(const PullNode& nd, uint32_t j, uint32_t nn, const uint32_t* AP, const REAL* Dn)
{
    return {(nd.lo < nn && AP[nd.lo] == (j << 1)) ? Dn[nd.lo] : REAL(0), (nd.hi < nn && AP[nd.hi] == ((j << 1) | 1u)) ? Dn[nd.hi] : REAL(0)};
}

// The sweeps' bodies for the pack `pc`: k_gr_down / k_gr_up run them with the workgroup's pack and PullBlockBar (__syncthreads()) as BAR,
// k_small_grad_mm_batch (kernels/batchmm.hpp) with a wave's pack and a wave-level ordering point.
template <typename REAL, bool NARROW, typename BAR>
__device__ __forceinline__ void gr_down_body(const DevPtrs<REAL>& d, const PackDev& pk, const PullPack<REAL>& pc, const uint32_t* par_ptr, const uint32_t* par,
                                             uint32_t ww, const REAL* __restrict__ g, REAL* __restrict__ out_lo, REAL* __restrict__ out_hi,
                                             uint32_t* __restrict__ arg)
{
    REAL* const S = pc.base;                    // [hop parity][arc][slot]: what the node sends along the arc
    REAL* const P0 = pc.base + 4 * (size_t)ww;  // path value through the lo arc per slot; after the arg-min: the runs' sums of S
    REAL* const P1 = pc.base + 5 * (size_t)ww;  // ... the hi arc
    uint32_t* const I0 = reinterpret_cast<uint32_t*>(pc.base + 6 * (size_t)ww);  // per run (at its first slot): the slot of the run's minimum, lo
    uint32_t* const I1 = I0 + ww;                                                // ... hi
    uint32_t* const Lid = I1 + ww;              // hop-local layer of the slot, PULL_NO_LAYER for padding
    const REAL INF = inf_v<REAL>();
    uint32_t cur = 0;
    for (uint32_t q = pc.q0; q < pc.q1; ++q, cur ^= 1u) {
        const uint32_t nb = pk.hop_node_off[q], n = pk.hop_node_off[q + 1] - nb, lbase = pk.hop_layer_off[q];
        const uint32_t nbn = nb + n;  // first slot of the next hop (the children)
        const uint32_t rt = (pk.hop_root != nullptr && q > pc.q0) ? (uint32_t)pk.hop_root[q] : (uint32_t)NO_ROOT;
        REAL* const Sc = S + (size_t)cur * 2 * ww;
        const REAL* const Sp = S + (size_t)(cur ^ 1u) * 2 * ww;
        // ---- pull dT, path values, what goes down each arc
        pull_slots<REAL, NARROW, true>(d, pc, nb, n, lbase, Lid, [&](uint32_t j, uint32_t wi, const PullNode& nd) {
            const REAL a = d.lohi[2 * (size_t)nd.layer] + gr_child_T(d.T, nbn, nd.lo), b = d.lohi[2 * (size_t)nd.layer + 1] + gr_child_T(d.T, nbn, nd.hi);
            const REAL f = d.F[nb + j];
            P0[j] = f + a;
            P1[j] = f + b;
            gr_send_down(par_ptr, par, wi, !(q == pc.q0 || j == rt), Sp, Sc, ww, j, REAL(0), a, b);
        });
        BAR::sync();
        // ---- arg-min per layer and arc (strictly smaller replaces, in the runs and among them: the lowest slot wins a tie)
        pull_layer_fold_bar<BAR>(
            pc, Lid, n, [](uint32_t j) { return Pull2<uint32_t>{j, j}; },
            [&](Pull2<uint32_t> v, Pull2<uint32_t> w) { return Pull2<uint32_t>{P0[w.lo] < P0[v.lo] ? w.lo : v.lo, P1[w.hi] < P1[v.hi] ? w.hi : v.hi}; },
            [&](uint32_t j, Pull2<uint32_t> v) { I0[j] = v.lo; I1[j] = v.hi; }, [&](uint32_t j) { return Pull2<uint32_t>{I0[j], I1[j]}; },
            [&](uint32_t l, Pull2<uint32_t> i) {
                // the seeds: only the head touches its layer's slots of S here
                const REAL gl = g[lbase + l];
                const bool f0 = P0[i.lo] < INF, f1 = P1[i.hi] < INF;
                if (f0) Sc[i.lo] -= gl;
                if (f1) Sc[ww + i.hi] += gl;
                arg[2 * (size_t)(lbase + l)] = f0 ? i.lo : GR_NONE;
                arg[2 * (size_t)(lbase + l) + 1] = f1 ? i.hi : GR_NONE;
            });
        BAR::sync();
        // ---- dc of the layer = the sum of S over its slots (the runs' sums into P0 / P1, dead by now)
        pull_layer_fold_bar<BAR>(
            pc, Lid, n, [&](uint32_t j) { return Pull2<REAL>{Sc[j], Sc[ww + j]}; },
            pull_add<REAL>, [&](uint32_t j, Pull2<REAL> v) { P0[j] = v.lo; P1[j] = v.hi; },
            [&](uint32_t j) { return Pull2<REAL>{P0[j], P1[j]}; }, [&](uint32_t l, Pull2<REAL> s) { out_lo[lbase + l] = s.lo; out_hi[lbase + l] = s.hi; });
        BAR::sync();  // the next hop overwrites P, I and Lid and pulls from this hop's S
    }
}

template <typename REAL, bool NARROW, bool GLOBAL>
__global__ void __launch_bounds__(NARROW ? 64 : WIDE_THREADS) k_gr_down(DevPtrs<REAL> d, PackDev pk, const uint32_t* par_ptr, const uint32_t* par, uint32_t ww,
                                                                        unsigned char* scratch, const REAL* __restrict__ g, REAL* __restrict__ out_lo,
                                                                        REAL* __restrict__ out_hi, uint32_t* __restrict__ arg)
{
    if (blockIdx.x >= pk.n_packs) return;
    const PullPack<REAL> pc = pull_pack<REAL, NARROW, GLOBAL>(d, pk, ww, scratch, gr_lds_bytes(sizeof(REAL), ww));
    gr_down_body<REAL, NARROW, PullBlockBar>(d, pk, pc, par_ptr, par, ww, g, out_lo, out_hi, arg);
}

template <typename REAL, bool NARROW, typename BAR>
__device__ __forceinline__ void gr_up_body(const DevPtrs<REAL>& d, const PackDev& pk, const PullPack<REAL>& pc, const uint32_t* par_ptr, const uint32_t* par,
                                           uint32_t ww, const REAL* __restrict__ g, REAL* __restrict__ out_lo, REAL* __restrict__ out_hi,
                                           const uint32_t* __restrict__ arg)
{
    REAL* const D = pc.base;                    // [hop parity][slot]: dF
    REAL* const V0 = pc.base + 2 * (size_t)ww;  // F + lo cost per slot of this hop; after the children's arg-min: what the node took over its lo arc
    REAL* const V1 = pc.base + 3 * (size_t)ww;  // ... hi
    REAL* const Q0 = pc.base + 4 * (size_t)ww;  // per run (at its first slot): the run's sum
    REAL* const Q1 = pc.base + 5 * (size_t)ww;
    uint32_t* const AP = reinterpret_cast<uint32_t*>(pc.base + 6 * (size_t)ww);  // per slot of the hop below: its arg-min parent << 1 | arc, GR_NONE
    uint32_t* const Lid = AP + ww;
    uint32_t cur = 0;
    for (uint32_t q = pc.q1; q-- > pc.q0; cur ^= 1u) {
        const uint32_t nb = pk.hop_node_off[q], n = pk.hop_node_off[q + 1] - nb, lbase = pk.hop_layer_off[q];
        const uint32_t nn = q + 1 < pc.q1 ? pk.hop_node_off[q + 2] - (nb + n) : 0u;  // slots of the hop below (the children)
        REAL* const Dc = D + (size_t)cur * ww;
        const REAL* const Dn = D + (size_t)(cur ^ 1u) * ww;
        // ---- F + cost of each arc
        pull_slots<REAL, NARROW, true>(d, pc, nb, n, lbase, Lid, [&](uint32_t j, uint32_t, const PullNode& nd) {
            const REAL f = d.F[nb + j];
            V0[j] = f + d.lohi[2 * (size_t)nd.layer];
            V1[j] = f + d.lohi[2 * (size_t)nd.layer + 1];
        });
        BAR::sync();
        // ---- the children's arg-min (parent, arc): first in parent table order wins a tie; a root or an unreachable node names nobody
        gr_name_parents(pc, par_ptr, par, nb + n + pc.wdelta, nn, V0, V1, AP);
        BAR::sync();
        // ---- dF = seeds + dF of the children that name this node
        pull_slots<REAL, NARROW, false>(d, pc, nb, n, lbase, nullptr, [&](uint32_t j, uint32_t, const PullNode& nd) {
            const Pull2<REAL> t = gr_take_up(nd, j, nn, AP, Dn);
            const REAL t0 = t.lo, t1 = t.hi;
            REAL df = t0 + t1;
            const uint32_t a0 = arg[2 * (size_t)nd.layer], a1 = arg[2 * (size_t)nd.layer + 1];
            if (a0 == j || a1 == j) {
                const REAL gl = g[nd.layer];
                if (a1 == j) df += gl;
                if (a0 == j) df -= gl;
            }
            Dc[j] = df;
            V0[j] = t0;
            V1[j] = t1;
        });
        BAR::sync();
        // ---- dc of the layer grows by the sum of what its nodes took
        pull_layer_fold_bar<BAR>(
            pc, Lid, n, [&](uint32_t j) { return Pull2<REAL>{V0[j], V1[j]}; },
            pull_add<REAL>, [&](uint32_t j, Pull2<REAL> v) { Q0[j] = v.lo; Q1[j] = v.hi; },
            [&](uint32_t j) { return Pull2<REAL>{Q0[j], Q1[j]}; },
            [&](uint32_t l, Pull2<REAL> s) {
                out_lo[lbase + l] += s.lo;  // behind k_gr_down's value; one writer per layer
                out_hi[lbase + l] += s.hi;
            });
        BAR::sync();  // the next hop overwrites every array but this hop's dF
    }
}

template <typename REAL, bool NARROW, bool GLOBAL>
__global__ void __launch_bounds__(NARROW ? 64 : WIDE_THREADS) k_gr_up(DevPtrs<REAL> d, PackDev pk, const uint32_t* par_ptr, const uint32_t* par, uint32_t ww,
                                                                      unsigned char* scratch, const REAL* __restrict__ g, REAL* __restrict__ out_lo,
                                                                      REAL* __restrict__ out_hi, const uint32_t* __restrict__ arg)
{
    if (blockIdx.x >= pk.n_packs) return;
    const PullPack<REAL> pc = pull_pack<REAL, NARROW, GLOBAL>(d, pk, ww, scratch, gr_lds_bytes(sizeof(REAL), ww));
    gr_up_body<REAL, NARROW, PullBlockBar>(d, pk, pc, par_ptr, par, ww, g, out_lo, out_hi, arg);
}

}  // namespace bddmma
