// kernels/graditer.hpp — the reverse of the two passes of a learned MMA iteration (bdd_cuda_learned_mma.cu:308-385 with :418-621,
// grad_iterations): k_gi_down reverses a backward pass, k_gi_up a forward pass.  Included by solver_gi.hpp (translation units
// solver_gi_f32.hip / solver_gi_f64.hip) and, for the sweeps' bodies, by kernels/gradsmall.hpp; behind kernels.hpp.
//
// A pass is described by what it read and wrote (GiArgs): the arc costs before (pre) and after it (post), the potentials F and T its
// min-marginals m_a[l] = min over the nodes u of l of F[u] + pre_a[l] + T[child_a(u)] were taken with, its mm[l] = omega_l (m_hi - m_lo), and
// the per-variable sums S of the deferred differences it consumed: post_a[l] = pre_a[l] + min(-+mm, 0) + alpha[l] S_a[v(l)].
//   backward pass  F is the forward pass's, T that of the post costs (rebuilt as the pass rose).  Its reverse goes root -> terminal and
//                  carries dT: per layer (1) dT[u] = what the parents sent + the incoming gT[u]; (2) every node sends its dT along its
//                  arg-min arc of post_a + T[child_a] (lo wins a tie), dpost_a[l] = the sum of what went along arc a; (3) the dual update,
//                  g_a = dpost_a[l] + the incoming g_a[l]: dmm = g_mm[l] + (mm[l] >= 0 ? -g_hi : g_lo), gS_a[l] = alpha[l] g_a,
//                  g_alpha[l] += S_lo g_lo + S_hi g_hi; (4) where both m_a are finite: g_omega[l] += dmm (m_hi - m_lo) and, with
//                  t = omega_l dmm and s = -1 (lo) / +1 (hi), at the arg-min node u*_a (lowest slot first): g_a += s t, gF[u*_a] += s t, and
//                  s t joins what u*_a sends down arc a.  g_a is the gradient of the pre costs.
//   forward pass   F is that of the post costs, T the one the pass read.  Its reverse goes terminal -> root and carries dF through the
//                  arg-min (parent, arc) of F[u] + post_a (parent table order), as k_gr_up does; steps (3) and (4) are the same with the
//                  seeds s t going to dF[u*_a] and to gT[child_a(u*_a)].
// FULL = false: only steps (1) and (2), g_a[l] += dpost_a[l] — the gradient of T(lo, hi) itself, which ends the reverse of the first
// tracked iteration.
// The routing steps — dT along the arg-min arc, the children's arg-min (parent, arc), what a node takes from the children that name it — are
// those of kernels/gradmm.hpp (gr_send_down, gr_name_parents, gr_take_up), with this pass's costs and potentials.
// Both are pull sweeps (kernels/pull.hpp): one launch per pack family, one workgroup per pack, the arg-mins and the layer sums in ONE layer
// fold per hop whose value is {sum lo, sum hi, arg-min lo, arg-min hi}; the layer's head then does steps (3) and (4) alone.  Nothing is
// accumulated atomically: two calls agree bit for bit.
#pragma once
#include "gradmm.hpp"

namespace bddmma {

template <typename REAL>
struct GiArgs {
    const REAL *F, *T;        // per slot
    const REAL *pre, *post;   // {lo, hi} per layer, interleaved
    const REAL* mm;           // per layer: what the pass wrote
    const REAL* S;            // {S_lo, S_hi} per variable: sums of the differences the pass consumed
    const int32_t* var;       // variable of a layer
    const REAL* alpha;        // per layer
    const REAL* omega_lay;    // per layer, or null: omega
    REAL omega;
    REAL *g_lo, *g_hi;        // per layer, in: of the post costs, out: of the pre costs
    const REAL* g_mm;         // per layer: of the pass's mm
    REAL* gS;                 // {alpha g_lo, alpha g_hi} per layer, out
    REAL *g_alpha, *g_omega;  // per layer, accumulated
    const REAL* g_in;         // per slot: gT (down) / gF (up)
    REAL* g_out;              // per slot, zero on entry: gF (down) / gT (up)
};

// 8 arrays of values + 3 of indices per slot (gr_lds_bytes: 6 + 3): float 44 bytes, double 76; a wide pack width beyond lds_cu / that is
// refused with BDDMMA_ERR_UNSUPPORTED (SolverT::gi_prepare).  The default wide pack width of 2 048 slots fits both.
__host__ __device__ inline size_t gi_lds_bytes(size_t real_size, uint32_t ww) { return (8 * real_size + 12) * (size_t)ww; }

template <typename REAL>
struct GiFold {
    REAL s0, s1;       // sums over the slots so far, per arc
    uint32_t i0, i1;   // slot of the smallest path value so far, per arc
};

// Steps (3) and (4) for layer l at its head: dc = what reached the post costs through the potentials, (m0, m1) the layer's min-marginals.
// Returns t (0: no seeds) and writes the layer's outputs.
// PIN (k_grad_small_batch): the products and sums below spelled out operation by operation, with contraction off.  Written as expressions
// they are contracted by the compiler as it sees fit in each kernel, and the narrow kernels k_gi_down / k_gi_up — whose bits the batch form
// promises — came out as: g_alpha's S_lo g_lo + S_hi g_hi two rounded products and a sum in float, fma(g_lo, S_lo, S_hi g_hi) in double;
// g_omega by one fma; g_hi + t by one fma; g_lo - t a subtraction of the rounded t in float, one fma in double.  The pinned form states
// exactly that, so that the fused kernel's bits do not depend on what surrounds this function there
// (tests/test_gpu_grad_small.py::test_batch_equals_each_member_on_the_four_launch_path holds the two together).
__device__ __forceinline__ float gi_fma(float x, float y, float z) { return __builtin_fmaf(x, y, z); }
__device__ __forceinline__ double gi_fma(double x, double y, double z) { return __builtin_fma(x, y, z); }
template <typename REAL>
__device__ __forceinline__ REAL gi_dual_pinned(const GiArgs<REAL>& a, uint32_t l, REAL dc0, REAL dc1, REAL m0, REAL m1)
{
#pragma clang fp contract(off)
    REAL g0 = dc0 + a.g_lo[l], g1 = dc1 + a.g_hi[l];
    const REAL dmm = a.g_mm[l] + (a.mm[l] >= REAL(0) ? -g1 : g0);
    const REAL al = a.alpha[l];
    const uint32_t v = (uint32_t)a.var[l];
    a.gS[2 * (size_t)l] = al * g0;
    a.gS[2 * (size_t)l + 1] = al * g1;
    const REAL p1 = a.S[2 * (size_t)v + 1] * g1;
    const REAL sg = sizeof(REAL) == 4 ? a.S[2 * (size_t)v] * g0 + p1 : gi_fma(g0, a.S[2 * (size_t)v], p1);
    a.g_alpha[l] = a.g_alpha[l] + sg;
    REAL t = REAL(0);
    if (m0 < inf_v<REAL>() && m1 < inf_v<REAL>()) {
        a.g_omega[l] = gi_fma(m1 - m0, dmm, a.g_omega[l]);
        const REAL om = a.omega_lay ? a.omega_lay[l] : a.omega;
        t = om * dmm;
        g0 = sizeof(REAL) == 4 ? g0 - t : gi_fma(-dmm, om, g0);
        g1 = gi_fma(dmm, om, g1);
    }
    a.g_lo[l] = g0;
    a.g_hi[l] = g1;
    return t;
}
template <typename REAL, bool PIN = false>
__device__ __forceinline__ REAL gi_dual(const GiArgs<REAL>& a, uint32_t l, REAL dc0, REAL dc1, REAL m0, REAL m1)
{
    if constexpr (PIN) return gi_dual_pinned(a, l, dc0, dc1, m0, m1);
    REAL g0 = dc0 + a.g_lo[l], g1 = dc1 + a.g_hi[l];
    const REAL dmm = a.g_mm[l] + (a.mm[l] >= REAL(0) ? -g1 : g0);
    const REAL al = a.alpha[l];
    const uint32_t v = (uint32_t)a.var[l];
    a.gS[2 * (size_t)l] = al * g0;
    a.gS[2 * (size_t)l + 1] = al * g1;
    a.g_alpha[l] += a.S[2 * (size_t)v] * g0 + a.S[2 * (size_t)v + 1] * g1;
    REAL t = REAL(0);
    if (m0 < inf_v<REAL>() && m1 < inf_v<REAL>()) {
        a.g_omega[l] += dmm * (m1 - m0);
        t = (a.omega_lay ? a.omega_lay[l] : a.omega) * dmm;
        g0 -= t;
        g1 += t;
    }
    a.g_lo[l] = g0;
    a.g_hi[l] = g1;
    return t;
}

// the layer fold of both sweeps: A0 / A1 what each slot adds to the layer's sums, P0 / P1 its path values (FULL), runs kept in Q0 / Q1 / I0 / I1
template <typename REAL, bool FULL, typename BAR, typename DONE>
__device__ __forceinline__ void gi_fold(const PullPack<REAL>& pc, const uint32_t* Lid, uint32_t n, const REAL* A0, const REAL* A1, const REAL* P0,
                                        const REAL* P1, REAL* Q0, REAL* Q1, uint32_t* I0, uint32_t* I1, DONE done)
{
    pull_layer_fold_bar<BAR>(
        pc, Lid, n, [&](uint32_t j) { return GiFold<REAL>{A0[j], A1[j], j, j}; },
        [&](GiFold<REAL> v, GiFold<REAL> w) {
            GiFold<REAL> r{v.s0 + w.s0, v.s1 + w.s1, v.i0, v.i1};
            if constexpr (FULL) {  // strictly smaller replaces: the lowest slot wins a tie
                if (P0[w.i0] < P0[v.i0]) r.i0 = w.i0;
                if (P1[w.i1] < P1[v.i1]) r.i1 = w.i1;
            }
            return r;
        },
        [&](uint32_t j, GiFold<REAL> v) { Q0[j] = v.s0; Q1[j] = v.s1; I0[j] = v.i0; I1[j] = v.i1; },
        [&](uint32_t j) { return GiFold<REAL>{Q0[j], Q1[j], I0[j], I1[j]}; }, done);
}

// The sweeps' bodies for the pack `pc`: k_gi_down / k_gi_up run them with the workgroup's pack and PullBlockBar (__syncthreads()) as BAR,
// k_grad_small_batch (kernels/gradsmall.hpp) with a wave's pack and a wave-level ordering point.
template <typename REAL, bool NARROW, bool FULL, typename BAR, bool PIN = false>
__device__ __forceinline__ void gi_down_body(const DevPtrs<REAL>& d, const PackDev& pk, const PullPack<REAL>& pc, const uint32_t* par_ptr, const uint32_t* par,
                                             uint32_t ww, const GiArgs<REAL>& a)
{
    REAL* const S = pc.base;                    // [hop parity][arc][slot]: what the node sends along the arc
    REAL* const P0 = pc.base + 4 * (size_t)ww;  // F + pre + T[child] through the lo arc per slot
    REAL* const P1 = pc.base + 5 * (size_t)ww;
    REAL* const Q0 = pc.base + 6 * (size_t)ww;  // per run (at its first slot): the run's sums
    REAL* const Q1 = pc.base + 7 * (size_t)ww;
    uint32_t* const I0 = reinterpret_cast<uint32_t*>(pc.base + 8 * (size_t)ww);  // ... and the slots of its minima
    uint32_t* const I1 = I0 + ww;
    uint32_t* const Lid = I1 + ww;
    uint32_t cur = 0;
    for (uint32_t q = pc.q0; q < pc.q1; ++q, cur ^= 1u) {
        const uint32_t nb = pk.hop_node_off[q], n = pk.hop_node_off[q + 1] - nb, lbase = pk.hop_layer_off[q];
        const uint32_t nbn = nb + n;
        const uint32_t rt = (pk.hop_root != nullptr && q > pc.q0) ? (uint32_t)pk.hop_root[q] : (uint32_t)NO_ROOT;
        REAL* const Sc = S + (size_t)cur * 2 * ww;
        const REAL* const Sp = S + (size_t)(cur ^ 1u) * 2 * ww;
        // ---- (1), (2): dT, the arc it leaves along, the path values of the min-marginals
        pull_slots<REAL, NARROW, true>(d, pc, nb, n, lbase, Lid, [&](uint32_t j, uint32_t wi, const PullNode& nd) {
            const REAL tl = gr_child_T(a.T, nbn, nd.lo), th = gr_child_T(a.T, nbn, nd.hi);
            gr_send_down(par_ptr, par, wi, !(q == pc.q0 || j == rt), Sp, Sc, ww, j, a.g_in[nb + j], a.post[2 * (size_t)nd.layer] + tl,
                         a.post[2 * (size_t)nd.layer + 1] + th);
            if constexpr (FULL) {
                const REAL f = a.F[nb + j];
                P0[j] = (f + a.pre[2 * (size_t)nd.layer]) + tl;
                P1[j] = (f + a.pre[2 * (size_t)nd.layer + 1]) + th;
            }
        });
        BAR::sync();
        // ---- the layer's sums and arg-mins; (3), (4) at its head: only the head touches its layer's slots of S here
        gi_fold<REAL, FULL, BAR>(pc, Lid, n, Sc, Sc + ww, P0, P1, Q0, Q1, I0, I1, [&](uint32_t l, GiFold<REAL> v) {
            const uint32_t L = lbase + l;
            if constexpr (FULL) {
                const REAL t = gi_dual<REAL, PIN>(a, L, v.s0, v.s1, P0[v.i0], P1[v.i1]);
                if (t != REAL(0)) {
                    Sc[v.i0] -= t;
                    Sc[ww + v.i1] += t;
                    a.g_out[nb + v.i0] -= t;
                    a.g_out[nb + v.i1] += t;
                }
            } else {
                a.g_lo[L] += v.s0;
                a.g_hi[L] += v.s1;
            }
        });
        BAR::sync();  // the next hop overwrites P, Q, I and Lid and pulls from this hop's S
    }
}

template <typename REAL, bool NARROW, bool GLOBAL, bool FULL>
__global__ void __launch_bounds__(NARROW ? 64 : WIDE_THREADS) k_gi_down(DevPtrs<REAL> d, PackDev pk, const uint32_t* par_ptr, const uint32_t* par, uint32_t ww,
                                                                        unsigned char* scratch, GiArgs<REAL> a)
{
    if (blockIdx.x >= pk.n_packs) return;
    const PullPack<REAL> pc = pull_pack<REAL, NARROW, GLOBAL>(d, pk, ww, scratch, gi_lds_bytes(sizeof(REAL), ww));
    gi_down_body<REAL, NARROW, FULL, PullBlockBar>(d, pk, pc, par_ptr, par, ww, a);
}

template <typename REAL, bool NARROW, typename BAR, bool PIN = false>
__device__ __forceinline__ void gi_up_body(const DevPtrs<REAL>& d, const PackDev& pk, const PullPack<REAL>& pc, const uint32_t* par_ptr, const uint32_t* par,
                                           uint32_t ww, const GiArgs<REAL>& a)
{
    REAL* const D = pc.base;                    // [hop parity][slot]: dF
    REAL* const V0 = pc.base + 2 * (size_t)ww;  // F + post lo cost per slot; after the children's arg-min: what the node took over its lo arc
    REAL* const V1 = pc.base + 3 * (size_t)ww;
    REAL* const P0 = pc.base + 4 * (size_t)ww;  // F + pre + T[child] through the lo arc per slot
    REAL* const P1 = pc.base + 5 * (size_t)ww;
    REAL* const Q0 = pc.base + 6 * (size_t)ww;
    REAL* const Q1 = pc.base + 7 * (size_t)ww;
    uint32_t* const AP = reinterpret_cast<uint32_t*>(pc.base + 8 * (size_t)ww);  // per slot of the hop below: gr_name_parents
    uint32_t* const I0 = AP;                    // (dead by the fold)
    uint32_t* const I1 = AP + ww;
    uint32_t* const Lid = I1 + ww;
    uint32_t cur = 0;
    for (uint32_t q = pc.q1; q-- > pc.q0; cur ^= 1u) {
        const uint32_t nb = pk.hop_node_off[q], n = pk.hop_node_off[q + 1] - nb, lbase = pk.hop_layer_off[q];
        const uint32_t nbn = nb + n;
        const uint32_t nn = q + 1 < pc.q1 ? pk.hop_node_off[q + 2] - nbn : 0u;  // slots of the hop below (the children)
        REAL* const Dc = D + (size_t)cur * ww;
        const REAL* const Dn = D + (size_t)(cur ^ 1u) * ww;
        pull_slots<REAL, NARROW, true>(d, pc, nb, n, lbase, Lid, [&](uint32_t j, uint32_t, const PullNode& nd) {
            const REAL f = a.F[nb + j];
            V0[j] = f + a.post[2 * (size_t)nd.layer];
            V1[j] = f + a.post[2 * (size_t)nd.layer + 1];
        });
        BAR::sync();
        // ---- the children's arg-min (parent, arc): first in parent table order wins a tie; a root or an unreachable node names nobody
        gr_name_parents(pc, par_ptr, par, nbn + pc.wdelta, nn, V0, V1, AP);
        BAR::sync();
        // ---- dF = the incoming gF + dF of the children that name this node; the path values of the min-marginals
        pull_slots<REAL, NARROW, false>(d, pc, nb, n, lbase, nullptr, [&](uint32_t j, uint32_t, const PullNode& nd) {
            const Pull2<REAL> t = gr_take_up(nd, j, nn, AP, Dn);
            Dc[j] = (t.lo + t.hi) + a.g_in[nb + j];
            V0[j] = t.lo;
            V1[j] = t.hi;
            const REAL f = a.F[nb + j];
            P0[j] = (f + a.pre[2 * (size_t)nd.layer]) + gr_child_T(a.T, nbn, nd.lo);
            P1[j] = (f + a.pre[2 * (size_t)nd.layer + 1]) + gr_child_T(a.T, nbn, nd.hi);
        });
        BAR::sync();  // AP is dead: the fold keeps its runs' minima there
        gi_fold<REAL, true, BAR>(pc, Lid, n, V0, V1, P0, P1, Q0, Q1, I0, I1, [&](uint32_t l, GiFold<REAL> v) {
            const REAL t = gi_dual<REAL, PIN>(a, lbase + l, v.s0, v.s1, P0[v.i0], P1[v.i1]);
            if (t != REAL(0)) {
                Dc[v.i0] -= t;
                Dc[v.i1] += t;
                const uint32_t c0 = pull_children<REAL, NARROW>(d, nb + v.i0 + pc.wdelta, ww).lo, c1 = pull_children<REAL, NARROW>(d, nb + v.i1 + pc.wdelta, ww).hi;
                if (c0 < nn) a.g_out[nbn + c0] -= t;  // the two may be one slot: one thread, in this order
                if (c1 < nn) a.g_out[nbn + c1] += t;
            }
        });
        BAR::sync();  // the next hop overwrites every array but this hop's dF
    }
}

template <typename REAL, bool NARROW, bool GLOBAL>
__global__ void __launch_bounds__(NARROW ? 64 : WIDE_THREADS) k_gi_up(DevPtrs<REAL> d, PackDev pk, const uint32_t* par_ptr, const uint32_t* par, uint32_t ww,
                                                                      unsigned char* scratch, GiArgs<REAL> a)
{
    if (blockIdx.x >= pk.n_packs) return;
    const PullPack<REAL> pc = pull_pack<REAL, NARROW, GLOBAL>(d, pk, ww, scratch, gi_lds_bytes(sizeof(REAL), ww));
    gi_up_body<REAL, NARROW, PullBlockBar>(d, pk, pc, par_ptr, par, ww, a);
}

// ---- elementwise
// S[v] = {sum of -d over d < 0, sum of d over d > 0} over the layers of v, in the order of the variable -> layer table (d in layer order)
// (the `_at` functions: one variable / layer of each, shared with k_grad_small_batch, kernels/gradsmall.hpp)
template <typename REAL>
__device__ __forceinline__ void gi_sums_at(const REAL* dl, const uint32_t* var_ptr, const uint32_t* var_layers, REAL* S, uint32_t v)
{
    REAL s0 = 0, s1 = 0;
    for (uint32_t k = var_ptr[v], e = var_ptr[v + 1]; k < e; ++k) {
        const REAL x = dl[var_layers[k]];
        if (x > REAL(0)) s1 += x;
        else if (x < REAL(0)) s0 -= x;
    }
    S[2 * (size_t)v] = s0;
    S[2 * (size_t)v + 1] = s1;
}
template <typename REAL>
__global__ void k_gi_sums(const REAL* __restrict__ dl, const uint32_t* __restrict__ var_ptr, const uint32_t* __restrict__ var_layers, REAL* __restrict__ S,
                          uint32_t n_vars)
{
    const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= n_vars) return;
    gi_sums_at(dl, var_ptr, var_layers, S, v);
}
// gS[v] = the sum of gS[l] over the layers of v, same order
template <typename REAL>
__device__ __forceinline__ void gi_var_sums_at(const REAL* gS, const uint32_t* var_ptr, const uint32_t* var_layers, REAL* gSv, uint32_t v)
{
    REAL s0 = 0, s1 = 0;
    for (uint32_t k = var_ptr[v], e = var_ptr[v + 1]; k < e; ++k) {
        s0 += gS[2 * (size_t)var_layers[k]];
        s1 += gS[2 * (size_t)var_layers[k] + 1];
    }
    gSv[2 * (size_t)v] = s0;
    gSv[2 * (size_t)v + 1] = s1;
}
template <typename REAL>
__global__ void k_gi_var_sums(const REAL* __restrict__ gS, const uint32_t* __restrict__ var_ptr, const uint32_t* __restrict__ var_layers, REAL* __restrict__ gSv,
                              uint32_t n_vars)
{
    const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= n_vars) return;
    gi_var_sums_at(gS, var_ptr, var_layers, gSv, v);
}
// the gradient of the differences a pass consumed (:503-518): gd[l] = d[l] >= 0 ? gS_hi[v] : -gS_lo[v]
template <typename REAL>
__device__ __forceinline__ void gi_gd_at(const REAL* dl, const REAL* gSv, const int32_t* var, REAL* gd, uint32_t l)
{
    const uint32_t v = (uint32_t)var[l];
    gd[l] = dl[l] >= REAL(0) ? gSv[2 * (size_t)v + 1] : -gSv[2 * (size_t)v];
}
template <typename REAL>
__global__ void k_gi_gd(const REAL* __restrict__ dl, const REAL* __restrict__ gSv, const int32_t* __restrict__ var, REAL* __restrict__ gd, uint32_t n)
{
    const uint32_t l = blockIdx.x * blockDim.x + threadIdx.x;
    if (l >= n) return;
    gi_gd_at(dl, gSv, var, gd, l);
}
// the gradient of a scalar omega: the per-layer values summed in double by one workgroup, every thread its strided share in layer order, then a
// tree over the threads — a fixed order
template <typename REAL>
__global__ void __launch_bounds__(256) k_gi_omega_sum(const REAL* __restrict__ g, REAL* __restrict__ out, uint32_t n)
{
    __shared__ double sh[256];
    double s = 0.0;
    for (uint32_t i = threadIdx.x; i < n; i += 256) s += (double)g[i];
    sh[threadIdx.x] = s;
    __syncthreads();
    for (uint32_t k = 128; k > 0; k >>= 1) {
        if (threadIdx.x < k) sh[threadIdx.x] += sh[threadIdx.x + k];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = (REAL)sh[0];
}

}  // namespace bddmma
