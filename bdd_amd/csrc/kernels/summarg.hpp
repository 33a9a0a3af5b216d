// kernels/summarg.hpp — the sweeps in the (log-sum-exp, +) semiring: sum-marginals (bdd_cuda_base.cu:788-1025, sum_marginals_cuda).
// Included by solver_sm.hpp only (translation units solver_sm_f32.hip / solver_sm_f64.hip), behind kernels.hpp.
//
// One forward and one backward launch per pack family (narrow / wide / huge), one workgroup per pack, frontier in LDS (huge packs: a
// global scratch of the same shape), no atomics of any kind:
//   forward   F~[n] = logsumexp over the parents p of n (F~[p] - cost of the arc p -> n), roots 0.  A sum cannot be pushed the way the
//             minimum is (lds_min), so a node PULLS: every node of a hop leaves F~ - lo and F~ - hi in two LDS arrays, and a node of the
//             next hop walks its parents through a parent table derived on the host from the node words (SolverT::sm_prepare), maximum
//             first, then the sum of exp(x - max).
//   backward  T~[n] = logaddexp(T~[lo] - lo, T~[hi] - hi) by pull (top sink 0, bottom sink -inf), and in the same hop the two path values
//             F~[n] + (T~[child] - cost) go to LDS and are reduced per layer (consecutive slots) in two levels, first the maximum, then
//             the sum of exp(x - max) with every node computing its own exp: the slots are cut into runs at every SM_CHUNK-th slot and
//             at every layer head; the first node of a run folds its run (<= SM_CHUNK steps), the layer's head folds its layer's runs
//             (width / SM_CHUNK steps).  A layer of one or two nodes is one run of its head.
// Every sum runs in a fixed order (parent table order, slot order, run order), so the results are the same bit for bit from call to call
// whatever the number of waves — which LDS float atomics into a layer slot would not give.
#pragma once

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

constexpr uint32_t SM_TOP = 0xFFFFFFFEu, SM_BOT = 0xFFFFFFFFu, SM_NO_LAYER = 0xFFFFFFFFu;
struct SmNode {
    bool act;           // a node (not a padding slot, not past the hop)
    uint32_t lo, hi;    // children: slot in the next hop, SM_TOP or SM_BOT
    uint32_t layer;     // global layer index
};
// Node j of a hop: NARROW — the 64 lanes of the (one-wave) workgroup decode 64 consecutive slots together; `lgrp` is the first layer of
// that lane group and is advanced by the group's layer count (load_layer, kernels/narrow.hpp).  Wide / huge: the word holds everything.
template <typename REAL, bool NARROW>
__device__ __forceinline__ SmNode sm_decode(const DevPtrs<REAL>& d, uint32_t wi, bool in, uint32_t ww, uint32_t lbase, uint32_t& lgrp)
{
    SmNode nd;
    if constexpr (NARROW) {
        const uint32_t w = in ? d.nwords[wi] : nw_pad_word(0);
        nd.act = !(w & NW_PAD);
        const uint32_t lo = w & NW_CHILD_MASK, hi = (w >> NW_CHILD_BITS) & NW_CHILD_MASK;
        nd.lo = lo < ww ? lo : (lo == nw_top(ww) ? SM_TOP : SM_BOT);
        nd.hi = hi < ww ? hi : (hi == nw_top(ww) ? SM_TOP : SM_BOT);
        nd.layer = lgrp + nw_lidx(w);
        lgrp += (uint32_t)__popcll(__ballot(nw_head(w)));
    } else {
        const uint64_t w = in ? d.wwords[wi] : WW_PAD_WORD;
        nd.act = in;
        const uint64_t lo = w & WW_CHILD_MASK, hi = (w >> WW_CHILD_BITS) & WW_CHILD_MASK;
        nd.lo = lo < WW_TOP ? (uint32_t)lo : (lo == WW_TOP ? SM_TOP : SM_BOT);
        nd.hi = hi < WW_TOP ? (uint32_t)hi : (hi == WW_TOP ? SM_TOP : SM_BOT);
        nd.layer = lbase + ww_layer(w);
    }
    return nd;
}

// LDS of a pack of width ww: forward 4 arrays of ww values; backward 7 arrays of values + 1 of layer indices (huge packs: the same in a
// global scratch of their own, SolverT::d_sm_scratch)
constexpr uint32_t SM_CHUNK = 16;
__host__ __device__ inline size_t sm_lds_bytes(size_t real_size, uint32_t ww) { return (7 * real_size + 4) * (size_t)ww; }

// word index of a slot = slot + wdelta: narrow packs read the (shared) word sequence of their structure, wide packs wwords[slot - base]
template <typename REAL, bool NARROW>
__device__ __forceinline__ uint32_t sm_wdelta(const DevPtrs<REAL>& d, const PackDev& pk, uint32_t p, uint32_t q0)
{
    return NARROW ? pk.pack_word_off[p] - pk.hop_node_off[q0] : 0u - d.wide_slot_base;
}

// par_ptr / par: parents of the node with word index wi are par[par_ptr[wi] .. par_ptr[wi + 1]): (slot in the previous hop) << 1 | arc
template <typename REAL, bool NARROW, bool GLOBAL>
__global__ void __launch_bounds__(NARROW ? 64 : WIDE_THREADS) k_sm_fwd(DevPtrs<REAL> d, PackDev pk, const uint32_t* par_ptr, const uint32_t* par, uint32_t ww,
                                                                       unsigned char* scratch)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const uint32_t tid = threadIdx.x, T = blockDim.x, p = blockIdx.x;
    if (p >= pk.n_packs) return;
    REAL* const A = reinterpret_cast<REAL*>(GLOBAL ? scratch + (size_t)p * sm_lds_bytes(sizeof(REAL), ww) : smem);  // [hop parity][arc][slot]
    const uint32_t q0 = pk.pack_hop_ptr[p], q1 = pk.pack_hop_ptr[p + 1];
    const uint32_t wdelta = sm_wdelta<REAL, NARROW>(d, pk, p, q0);
    const REAL NINF = -inf_v<REAL>();
    uint32_t cur = 0;
    for (uint32_t q = q0; q < q1; ++q, cur ^= 1u) {
        const uint32_t nb = pk.hop_node_off[q], n = pk.hop_node_off[q + 1] - nb, lbase = pk.hop_layer_off[q];
        const uint32_t rt = (pk.hop_root != nullptr && q > q0) ? (uint32_t)pk.hop_root[q] : (uint32_t)NO_ROOT;  // a BDD that starts at this hop
        REAL* const Ac = A + (size_t)cur * 2 * ww;
        const REAL* const Ap = A + (size_t)(cur ^ 1u) * 2 * ww;
        uint32_t lgrp = lbase;
        // Every lane runs every trip to its end (sm_decode ballots over the wave): the body is predicated on nd.act, never left early.
        for (uint32_t r0 = 0; r0 < n; r0 += T) {
            const uint32_t j = r0 + tid;
            const uint32_t wi = nb + j + wdelta;
            const SmNode nd = sm_decode<REAL, NARROW>(d, wi, j < n, ww, lbase, lgrp);
            if (nd.act) {
                REAL f = REAL(0);  // roots (flush_costs_from_root)
                if (!(q == q0 || j == rt)) {
                    const uint32_t b = par_ptr[wi], e = par_ptr[wi + 1];
                    REAL m = NINF;
                    for (uint32_t k = b; k < e; ++k) {
                        const uint32_t x = par[k];
                        m = rmax(m, Ap[(size_t)(x & 1u) * ww + (x >> 1)]);
                    }
                    REAL s = REAL(0);
                    if (m > NINF)
                        for (uint32_t k = b; k < e; ++k) {
                            const uint32_t x = par[k];
                            s += sm_exp(Ap[(size_t)(x & 1u) * ww + (x >> 1)] - m);
                        }
                    f = sm_finish(m, s);
                }
                Ac[j] = f - d.lohi[2 * (size_t)nd.layer];
                Ac[ww + j] = f - d.lohi[2 * (size_t)nd.layer + 1];
                d.F[nb + j] = f;
            }
        }
        __syncthreads();  // this hop's values before the next hop's pulls; the next hop writes the other parity
    }
}

template <typename REAL, bool NARROW, bool GLOBAL>
__global__ void __launch_bounds__(NARROW ? 64 : WIDE_THREADS) k_sm_bwd(DevPtrs<REAL> d, PackDev pk, uint32_t ww, unsigned char* scratch)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const uint32_t tid = threadIdx.x, T = blockDim.x, p = blockIdx.x;
    if (p >= pk.n_packs) return;
    REAL* const base = reinterpret_cast<REAL*>(GLOBAL ? scratch + (size_t)p * sm_lds_bytes(sizeof(REAL), ww) : smem);
    REAL* const Tb = base;                   // [hop parity][slot]: T~
    REAL* const P0 = base + 2 * (size_t)ww;  // path values through the lo arc per slot, then exp(value - the layer's maximum)
    REAL* const P1 = base + 3 * (size_t)ww;  // ... the hi arc
    REAL* const Q0 = base + 4 * (size_t)ww;  // per run (at its first slot): the run's maximum, then its sum
    REAL* const Q1 = base + 5 * (size_t)ww;
    REAL* const M1 = base + 6 * (size_t)ww;  // per layer of the hop: the maximum of the hi values (lo: in the children's T~, dead by then)
    uint32_t* const Lid = reinterpret_cast<uint32_t*>(base + 7 * (size_t)ww);  // hop-local layer of the slot, SM_NO_LAYER for padding
    const uint32_t q0 = pk.pack_hop_ptr[p], q1 = pk.pack_hop_ptr[p + 1];
    const uint32_t wdelta = sm_wdelta<REAL, NARROW>(d, pk, p, q0);
    const REAL NINF = -inf_v<REAL>();
    uint32_t cur = 0;
    // slot j starts a run: the head of its layer, or every SM_CHUNK-th slot inside a layer
    auto run_start = [&](uint32_t j, uint32_t l) { return l != SM_NO_LAYER && (j % SM_CHUNK == 0 || j == 0 || Lid[j - 1] != l); };
    auto is_head = [&](uint32_t j, uint32_t l) { return l != SM_NO_LAYER && (j == 0 || Lid[j - 1] != l); };
    for (uint32_t q = q1; q-- > q0; cur ^= 1u) {
        const uint32_t nb = pk.hop_node_off[q], n = pk.hop_node_off[q + 1] - nb, lbase = pk.hop_layer_off[q];
        REAL* const Tc = Tb + (size_t)cur * ww;           // this hop
        REAL* const Tn = Tb + (size_t)(cur ^ 1u) * ww;    // the hop below (children); after the pull: M0, the layers' maxima of the lo values
        REAL* const M0 = Tn;
        uint32_t lgrp = lbase;
        // ---- pull, path values.  Every lane runs every trip to its end (sm_decode ballots over the wave): predicated, never left early.
        for (uint32_t r0 = 0; r0 < n; r0 += T) {
            const uint32_t j = r0 + tid;
            const SmNode nd = sm_decode<REAL, NARROW>(d, nb + j + wdelta, j < n, ww, lbase, lgrp);
            if (j < n) Lid[j] = nd.act ? nd.layer - lbase : SM_NO_LAYER;
            if (nd.act) {
                const REAL tl = nd.lo == SM_BOT ? NINF : (nd.lo == SM_TOP ? REAL(0) : Tn[nd.lo]);
                const REAL th = nd.hi == SM_BOT ? NINF : (nd.hi == SM_TOP ? REAL(0) : Tn[nd.hi]);
                const REAL a = tl - d.lohi[2 * (size_t)nd.layer], b = th - d.lohi[2 * (size_t)nd.layer + 1];
                const REAL t = sm_logaddexp(a, b);
                const REAL f = d.F[nb + j];
                Tc[j] = t;
                d.T[nb + j] = t;
                P0[j] = f + a;
                P1[j] = f + b;
            }
        }
        __syncthreads();
        // ---- maxima: runs, then layers
        for (uint32_t j = tid; j < n; j += T) {
            const uint32_t l = Lid[j];
            if (run_start(j, l)) {
                REAL m0 = P0[j], m1 = P1[j];
                for (uint32_t e = j + 1; e < n && e % SM_CHUNK != 0 && Lid[e] == l; ++e) {
                    m0 = rmax(m0, P0[e]);
                    m1 = rmax(m1, P1[e]);
                }
                Q0[j] = m0;
                Q1[j] = m1;
            }
        }
        __syncthreads();
        for (uint32_t j = tid; j < n; j += T) {
            const uint32_t l = Lid[j];
            if (is_head(j, l)) {
                REAL m0 = Q0[j], m1 = Q1[j];
                for (uint32_t e = (j / SM_CHUNK + 1) * SM_CHUNK; e < n && Lid[e] == l; e += SM_CHUNK) {
                    m0 = rmax(m0, Q0[e]);
                    m1 = rmax(m1, Q1[e]);
                }
                M0[l] = m0;
                M1[l] = m1;
            }
        }
        __syncthreads();
        // ---- exp(value - maximum), every node its own; then the sums: runs, then layers
        for (uint32_t j = tid; j < n; j += T) {
            const uint32_t l = Lid[j];
            if (l != SM_NO_LAYER) {
                const REAL m0 = M0[l], m1 = M1[l];
                P0[j] = m0 > NINF ? sm_exp(P0[j] - m0) : REAL(0);
                P1[j] = m1 > NINF ? sm_exp(P1[j] - m1) : REAL(0);
            }
        }
        __syncthreads();
        for (uint32_t j = tid; j < n; j += T) {
            const uint32_t l = Lid[j];
            if (run_start(j, l)) {
                REAL s0 = P0[j], s1 = P1[j];
                for (uint32_t e = j + 1; e < n && e % SM_CHUNK != 0 && Lid[e] == l; ++e) {
                    s0 += P0[e];
                    s1 += P1[e];
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
                d.mm0_out[lbase + l] = sm_finish(M0[l], s0);
                d.mm1_out[lbase + l] = sm_finish(M1[l], s1);
            }
        }
        __syncthreads();  // the next hop overwrites every array (M0 is its T~ buffer)
    }
}

}  // namespace bddmma
