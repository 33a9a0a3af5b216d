// kernels/gradmm.hpp — the backward operator of the min-marginal differences (bdd_cuda_learned_mma.cu:623-1023, grad_mm_diff_all_hops):
// the transpose-Jacobian product of mm_diff[l] = m_hi[l] - m_lo[l], m_a[l] = min over the nodes u of l of F[u] + c_a[l] + T[child_a(u)],
// with respect to the lo / hi arc costs.  Included by solver_gr.hpp only (translation units solver_gr_f32.hip / solver_gr_f64.hip), behind
// kernels.hpp and kernels/summarg.hpp (node decoding, parent tables, SM_CHUNK runs).
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
// One launch per direction and pack family (narrow / wide / huge), one workgroup per pack, frontier in LDS (huge packs: a global scratch
// of the same shape), no atomics of any kind — both directions PULL:
//   down  a node leaves in LDS what it sends along each arc, S_a[u] = (a is u's arg-min arc ? dT[u] : 0) + (u == u*_a ? s g : 0); a node
//         of the next hop sums S over its parents in parent table order.  The layer's dc is the sum of S_a over its slots.
//   up    the nodes of hop q leave F + c_a in LDS, the nodes of hop q + 1 publish their arg-min (parent, arc) from it, and every node
//         of hop q takes dF of each child that names it.  The layer's dc grows by the sum of what its nodes took per arc.
// The per-layer arg-min and the per-layer sums run over the layer's consecutive slots in two levels with a fixed order (runs of SM_CHUNK
// slots, then the layer's runs, as k_sm_bwd), so two calls agree bit for bit whatever the number of waves.
// k_gr_down writes grad_lo / grad_hi of every layer and the arg-min slots (arg); k_gr_up, launched behind it, adds its part.
#pragma once

namespace bddmma {

constexpr uint32_t GR_NONE = 0xFFFFFFFFu;
// LDS of a pack of width ww: down 6 arrays of values + 3 of indices, up 6 + 2.  In float that is 36 bytes per slot against the 32 of
// sm_lds_bytes (double: 60 against 60), so a wide pack width that the sum-marginals just fit (above lds_cu / 36 slots, 4 551 at 160 KiB)
// is refused here with BDDMMA_ERR_UNSUPPORTED (SolverT::gr_prepare); the default wide pack width is 2 048 slots.
__host__ __device__ inline size_t gr_lds_bytes(size_t real_size, uint32_t ww) { return (6 * real_size + 12) * (size_t)ww; }

template <typename REAL, bool NARROW, bool GLOBAL>
__global__ void __launch_bounds__(NARROW ? 64 : WIDE_THREADS) k_gr_down(DevPtrs<REAL> d, PackDev pk, const uint32_t* par_ptr, const uint32_t* par, uint32_t ww,
                                                                        unsigned char* scratch, const REAL* __restrict__ g, REAL* __restrict__ out_lo,
                                                                        REAL* __restrict__ out_hi, uint32_t* __restrict__ arg)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const uint32_t tid = threadIdx.x, T = blockDim.x, p = blockIdx.x;
    if (p >= pk.n_packs) return;
    REAL* const base = reinterpret_cast<REAL*>(GLOBAL ? scratch + (size_t)p * gr_lds_bytes(sizeof(REAL), ww) : smem);
    REAL* const S = base;                    // [hop parity][arc][slot]: what the node sends along the arc
    REAL* const P0 = base + 4 * (size_t)ww;  // path value through the lo arc per slot; after the arg-min: the runs' sums of S
    REAL* const P1 = base + 5 * (size_t)ww;  // ... the hi arc
    uint32_t* const I0 = reinterpret_cast<uint32_t*>(base + 6 * (size_t)ww);  // per run (at its first slot): the slot of the run's minimum, lo
    uint32_t* const I1 = I0 + ww;                                             // ... hi
    uint32_t* const Lid = I1 + ww;           // hop-local layer of the slot, SM_NO_LAYER for padding
    const uint32_t q0 = pk.pack_hop_ptr[p], q1 = pk.pack_hop_ptr[p + 1];
    const uint32_t wdelta = sm_wdelta<REAL, NARROW>(d, pk, p, q0);
    const REAL INF = inf_v<REAL>();
    auto run_start = [&](uint32_t j, uint32_t l) { return l != SM_NO_LAYER && (j % SM_CHUNK == 0 || j == 0 || Lid[j - 1] != l); };
    auto is_head = [&](uint32_t j, uint32_t l) { return l != SM_NO_LAYER && (j == 0 || Lid[j - 1] != l); };
    uint32_t cur = 0;
    for (uint32_t q = q0; q < q1; ++q, cur ^= 1u) {
        const uint32_t nb = pk.hop_node_off[q], n = pk.hop_node_off[q + 1] - nb, lbase = pk.hop_layer_off[q];
        const uint32_t nbn = nb + n;  // first slot of the next hop (the children)
        const uint32_t rt = (pk.hop_root != nullptr && q > q0) ? (uint32_t)pk.hop_root[q] : (uint32_t)NO_ROOT;
        REAL* const Sc = S + (size_t)cur * 2 * ww;
        const REAL* const Sp = S + (size_t)(cur ^ 1u) * 2 * ww;
        uint32_t lgrp = lbase;
        // ---- pull dT, path values, what goes down each arc.  Every lane runs every trip to its end (sm_decode ballots over the wave).
        for (uint32_t r0 = 0; r0 < n; r0 += T) {
            const uint32_t j = r0 + tid;
            const uint32_t wi = nb + j + wdelta;
            const SmNode nd = sm_decode<REAL, NARROW>(d, wi, j < n, ww, lbase, lgrp);
            if (j < n) Lid[j] = nd.act ? nd.layer - lbase : SM_NO_LAYER;
            if (nd.act) {
                REAL dt = REAL(0);
                if (!(q == q0 || j == rt)) {
                    const uint32_t b = par_ptr[wi], e = par_ptr[wi + 1];
                    for (uint32_t k = b; k < e; ++k) {
                        const uint32_t x = par[k];
                        dt += Sp[(size_t)(x & 1u) * ww + (x >> 1)];
                    }
                }
                const REAL tl = nd.lo == SM_BOT ? INF : (nd.lo == SM_TOP ? REAL(0) : d.T[nbn + nd.lo]);
                const REAL th = nd.hi == SM_BOT ? INF : (nd.hi == SM_TOP ? REAL(0) : d.T[nbn + nd.hi]);
                const REAL a = d.lohi[2 * (size_t)nd.layer] + tl, b = d.lohi[2 * (size_t)nd.layer + 1] + th;
                const REAL f = d.F[nb + j];
                P0[j] = f + a;
                P1[j] = f + b;
                const bool lo_arc = a <= b;  // lo before hi
                Sc[j] = lo_arc ? dt : REAL(0);
                Sc[ww + j] = lo_arc ? REAL(0) : dt;
            }
        }
        __syncthreads();
        // ---- arg-min per layer and arc: runs, then layers (strictly smaller replaces: the lowest slot wins a tie)
        for (uint32_t j = tid; j < n; j += T) {
            const uint32_t l = Lid[j];
            if (run_start(j, l)) {
                uint32_t i0 = j, i1 = j;
                for (uint32_t e = j + 1; e < n && e % SM_CHUNK != 0 && Lid[e] == l; ++e) {
                    if (P0[e] < P0[i0]) i0 = e;
                    if (P1[e] < P1[i1]) i1 = e;
                }
                I0[j] = i0;
                I1[j] = i1;
            }
        }
        __syncthreads();
        for (uint32_t j = tid; j < n; j += T) {
            const uint32_t l = Lid[j];
            if (is_head(j, l)) {
                uint32_t i0 = I0[j], i1 = I1[j];
                for (uint32_t e = (j / SM_CHUNK + 1) * SM_CHUNK; e < n && Lid[e] == l; e += SM_CHUNK) {
                    const uint32_t c0 = I0[e], c1 = I1[e];
                    if (P0[c0] < P0[i0]) i0 = c0;
                    if (P1[c1] < P1[i1]) i1 = c1;
                }
                // the seeds: only the head touches its layer's slots of S here
                const REAL gl = g[lbase + l];
                const bool f0 = P0[i0] < INF, f1 = P1[i1] < INF;
                if (f0) Sc[i0] -= gl;
                if (f1) Sc[ww + i1] += gl;
                arg[2 * (size_t)(lbase + l)] = f0 ? i0 : GR_NONE;
                arg[2 * (size_t)(lbase + l) + 1] = f1 ? i1 : GR_NONE;
            }
        }
        __syncthreads();
        // ---- dc of the layer = the sum of S over its slots: runs (into P0 / P1, dead by now), then layers
        for (uint32_t j = tid; j < n; j += T) {
            const uint32_t l = Lid[j];
            if (run_start(j, l)) {
                REAL s0 = Sc[j], s1 = Sc[ww + j];
                for (uint32_t e = j + 1; e < n && e % SM_CHUNK != 0 && Lid[e] == l; ++e) {
                    s0 += Sc[e];
                    s1 += Sc[ww + e];
                }
                P0[j] = s0;
                P1[j] = s1;
            }
        }
        __syncthreads();
        for (uint32_t j = tid; j < n; j += T) {
            const uint32_t l = Lid[j];
            if (is_head(j, l)) {
                REAL s0 = P0[j], s1 = P1[j];
                for (uint32_t e = (j / SM_CHUNK + 1) * SM_CHUNK; e < n && Lid[e] == l; e += SM_CHUNK) {
                    s0 += P0[e];
                    s1 += P1[e];
                }
                out_lo[lbase + l] = s0;
                out_hi[lbase + l] = s1;
            }
        }
        __syncthreads();  // the next hop overwrites P, I and Lid and pulls from this hop's S
    }
}

template <typename REAL, bool NARROW, bool GLOBAL>
__global__ void __launch_bounds__(NARROW ? 64 : WIDE_THREADS) k_gr_up(DevPtrs<REAL> d, PackDev pk, const uint32_t* par_ptr, const uint32_t* par, uint32_t ww,
                                                                      unsigned char* scratch, const REAL* __restrict__ g, REAL* __restrict__ out_lo,
                                                                      REAL* __restrict__ out_hi, const uint32_t* __restrict__ arg)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const uint32_t tid = threadIdx.x, T = blockDim.x, p = blockIdx.x;
    if (p >= pk.n_packs) return;
    REAL* const base = reinterpret_cast<REAL*>(GLOBAL ? scratch + (size_t)p * gr_lds_bytes(sizeof(REAL), ww) : smem);
    REAL* const D = base;                    // [hop parity][slot]: dF
    REAL* const V0 = base + 2 * (size_t)ww;  // F + lo cost per slot of this hop; after the children's arg-min: what the node took over its lo arc
    REAL* const V1 = base + 3 * (size_t)ww;  // ... hi
    REAL* const Q0 = base + 4 * (size_t)ww;  // per run (at its first slot): the run's sum
    REAL* const Q1 = base + 5 * (size_t)ww;
    uint32_t* const AP = reinterpret_cast<uint32_t*>(base + 6 * (size_t)ww);  // per slot of the hop below: its arg-min parent << 1 | arc, GR_NONE
    uint32_t* const Lid = AP + ww;
    const uint32_t q0 = pk.pack_hop_ptr[p], q1 = pk.pack_hop_ptr[p + 1];
    const uint32_t wdelta = sm_wdelta<REAL, NARROW>(d, pk, p, q0);
    const REAL INF = inf_v<REAL>();
    auto run_start = [&](uint32_t j, uint32_t l) { return l != SM_NO_LAYER && (j % SM_CHUNK == 0 || j == 0 || Lid[j - 1] != l); };
    auto is_head = [&](uint32_t j, uint32_t l) { return l != SM_NO_LAYER && (j == 0 || Lid[j - 1] != l); };
    uint32_t cur = 0;
    for (uint32_t q = q1; q-- > q0; cur ^= 1u) {
        const uint32_t nb = pk.hop_node_off[q], n = pk.hop_node_off[q + 1] - nb, lbase = pk.hop_layer_off[q];
        const uint32_t nn = q + 1 < q1 ? pk.hop_node_off[q + 2] - (nb + n) : 0u;  // slots of the hop below (the children)
        REAL* const Dc = D + (size_t)cur * ww;
        const REAL* const Dn = D + (size_t)(cur ^ 1u) * ww;
        uint32_t lgrp = lbase;
        // ---- F + cost of each arc.  Every lane runs every trip to its end (sm_decode ballots over the wave).
        for (uint32_t r0 = 0; r0 < n; r0 += T) {
            const uint32_t j = r0 + tid;
            const SmNode nd = sm_decode<REAL, NARROW>(d, nb + j + wdelta, j < n, ww, lbase, lgrp);
            if (j < n) Lid[j] = nd.act ? nd.layer - lbase : SM_NO_LAYER;
            if (nd.act) {
                const REAL f = d.F[nb + j];
                V0[j] = f + d.lohi[2 * (size_t)nd.layer];
                V1[j] = f + d.lohi[2 * (size_t)nd.layer + 1];
            }
        }
        __syncthreads();
        // ---- the children's arg-min (parent, arc): first in parent table order wins a tie; a root or an unreachable node names nobody
        for (uint32_t c = tid; c < nn; c += T) {
            const uint32_t wi = nb + n + c + wdelta;
            const uint32_t b = par_ptr[wi], e = par_ptr[wi + 1];
            REAL m = INF;
            uint32_t best = GR_NONE;
            for (uint32_t k = b; k < e; ++k) {
                const uint32_t x = par[k];
                const REAL v = (x & 1u) ? V1[x >> 1] : V0[x >> 1];
                if (v < m) { m = v; best = x; }
            }
            AP[c] = best;
        }
        __syncthreads();
        // ---- dF = seeds + dF of the children that name this node
        lgrp = lbase;
        for (uint32_t r0 = 0; r0 < n; r0 += T) {
            const uint32_t j = r0 + tid;
            const SmNode nd = sm_decode<REAL, NARROW>(d, nb + j + wdelta, j < n, ww, lbase, lgrp);
            if (nd.act) {
                const REAL t0 = (nd.lo < nn && AP[nd.lo] == (j << 1)) ? Dn[nd.lo] : REAL(0);
                const REAL t1 = (nd.hi < nn && AP[nd.hi] == ((j << 1) | 1u)) ? Dn[nd.hi] : REAL(0);
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
            }
        }
        __syncthreads();
        // ---- dc of the layer grows by the sum of what its nodes took: runs, then layers
        for (uint32_t j = tid; j < n; j += T) {
            const uint32_t l = Lid[j];
            if (run_start(j, l)) {
                REAL s0 = V0[j], s1 = V1[j];
                for (uint32_t e = j + 1; e < n && e % SM_CHUNK != 0 && Lid[e] == l; ++e) {
                    s0 += V0[e];
                    s1 += V1[e];
                }
                Q0[j] = s0;
                Q1[j] = s1;
            }
        }
        __syncthreads();
        for (uint32_t j = tid; j < n; j += T) {
            const uint32_t l = Lid[j];
            if (is_head(j, l)) {
                REAL s0 = Q0[j], s1 = Q1[j];
                for (uint32_t e = (j / SM_CHUNK + 1) * SM_CHUNK; e < n && Lid[e] == l; e += SM_CHUNK) {
                    s0 += Q0[e];
                    s1 += Q1[e];
                }
                out_lo[lbase + l] += s0;  // behind k_gr_down's value; one writer per layer
                out_hi[lbase + l] += s1;
            }
        }
        __syncthreads();  // the next hop overwrites every array but this hop's dF
    }
}

}  // namespace bddmma
