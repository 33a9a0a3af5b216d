// kernels/pull.hpp — the skeleton of the pull sweeps: the sum-marginals (kernels/summarg.hpp) and the gradient of the min-marginal
// differences (kernels/gradmm.hpp).  Included by summarg.hpp and gradmm.hpp, behind kernels.hpp.
//
// A pull sweep runs one workgroup per pack (narrow / wide / huge: one launch each), hop by hop, with the frontier in per-pack arrays
// (PullPack::base: LDS, huge packs a global scratch of the same shape) and no atomics of any kind.  A node PULLS what the previous hop
// left there: from its parents through a parent table derived on the host from the node words (SolverT::sm_prepare), or from its children
// through its node word.  A value per layer is folded over the layer's consecutive slots in two levels (pull_layer_fold).
// Every fold runs in a fixed order (parent table order, slot order, run order), so the results are the same bit for bit from call to call
// whatever the number of waves — which LDS float atomics into a layer slot would not give.  That order is written here and nowhere else.
#pragma once

namespace bddmma {

constexpr uint32_t PULL_TOP = 0xFFFFFFFEu, PULL_BOT = 0xFFFFFFFFu, PULL_NO_LAYER = 0xFFFFFFFFu;
constexpr uint32_t PULL_CHUNK = 16;  // slots of a run, the first level of pull_layer_fold

struct PullNode {
    bool act;           // a node (not a padding slot, not past the hop)
    uint32_t lo, hi;    // children: slot in the next hop, PULL_TOP or PULL_BOT
    uint32_t layer;     // global layer index
};
// Node j of a hop: NARROW — the 64 lanes of the (one-wave) workgroup decode 64 consecutive slots together; `lgrp` is the first layer of
// that lane group and is advanced by the group's layer count (load_layer, kernels/narrow.hpp).  Wide / huge: the word holds everything.
// The children of a node word as slots of the next hop, PULL_TOP or PULL_BOT: the part of the decode that needs no ballot, so a single lane
// may ask for the children of any slot (word index wi).  W: uint32_t (narrow) / uint64_t (wide).
struct PullChildren {
    uint32_t lo, hi;
};
template <bool NARROW, typename W>
__device__ __forceinline__ PullChildren pull_children_of(W w, uint32_t ww)
{
    if constexpr (NARROW) {
        const uint32_t lo = w & NW_CHILD_MASK, hi = (w >> NW_CHILD_BITS) & NW_CHILD_MASK;
        return {lo < ww ? lo : (lo == nw_top(ww) ? PULL_TOP : PULL_BOT), hi < ww ? hi : (hi == nw_top(ww) ? PULL_TOP : PULL_BOT)};
    } else {
        const uint64_t lo = w & WW_CHILD_MASK, hi = (w >> WW_CHILD_BITS) & WW_CHILD_MASK;
        return {lo < WW_TOP ? (uint32_t)lo : (lo == WW_TOP ? PULL_TOP : PULL_BOT), hi < WW_TOP ? (uint32_t)hi : (hi == WW_TOP ? PULL_TOP : PULL_BOT)};
    }
}
template <typename REAL, bool NARROW>
__device__ __forceinline__ PullChildren pull_children(const DevPtrs<REAL>& d, uint32_t wi, uint32_t ww)
{
    if constexpr (NARROW) return pull_children_of<true>(d.nwords[wi], ww);
    else return pull_children_of<false>(d.wwords[wi], ww);
}
template <typename REAL, bool NARROW>
__device__ __forceinline__ PullNode pull_decode(const DevPtrs<REAL>& d, uint32_t wi, bool in, uint32_t ww, uint32_t lbase, uint32_t& lgrp)
{
    PullNode nd;
    if constexpr (NARROW) {
        const uint32_t w = in ? d.nwords[wi] : nw_pad_word(0);
        nd.act = !(w & NW_PAD);
        const PullChildren c = pull_children_of<true>(w, ww);
        nd.lo = c.lo;
        nd.hi = c.hi;
        nd.layer = lgrp + nw_lidx(w);
        lgrp += (uint32_t)__popcll(__ballot(nw_head(w)));
    } else {
        const uint64_t w = in ? d.wwords[wi] : WW_PAD_WORD;
        nd.act = in;
        const PullChildren c = pull_children_of<false>(w, ww);
        nd.lo = c.lo;
        nd.hi = c.hi;
        nd.layer = lbase + ww_layer(w);
    }
    return nd;
}

// The pack of this workgroup (blockIdx.x < pk.n_packs).  `bytes` = the size of a pack's arrays (sm_lds_bytes / gr_lds_bytes of ww).
template <typename REAL>
struct PullPack {
    REAL* base;        // the pack's arrays: the dynamic LDS; GLOBAL (huge packs): scratch + pack * bytes
    uint32_t q0, q1;   // its hops
    uint32_t wdelta;   // word index of a slot = slot + wdelta: narrow packs read the (shared) word sequence of their structure, wide
                       // packs wwords[slot - base]
    uint32_t ww, tid, T;
};
template <typename REAL, bool NARROW, bool GLOBAL>
__device__ __forceinline__ PullPack<REAL> pull_pack(const DevPtrs<REAL>& d, const PackDev& pk, uint32_t ww, unsigned char* scratch, size_t bytes)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const uint32_t p = blockIdx.x, q0 = pk.pack_hop_ptr[p];
    return {reinterpret_cast<REAL*>(GLOBAL ? scratch + (size_t)p * bytes : smem), q0, pk.pack_hop_ptr[p + 1],
            NARROW ? pk.pack_word_off[p] - pk.hop_node_off[q0] : 0u - d.wide_slot_base, ww, threadIdx.x, blockDim.x};
}

// body(j, wi, nd) for every node of the hop of n slots from nb on (j: slot in the hop, wi: its word index), T slots a trip.  Every lane
// runs every trip to its end, because pull_decode ballots over the wave: the body is predicated on nd.act, never left early.
// FILL: Lid[j] = the hop-local layer of slot j, PULL_NO_LAYER for padding — what pull_layer_fold reads.
template <typename REAL, bool NARROW, bool FILL, typename BODY>
__device__ __forceinline__ void pull_slots(const DevPtrs<REAL>& d, const PullPack<REAL>& pc, uint32_t nb, uint32_t n, uint32_t lbase, uint32_t* Lid, BODY body)
{
    uint32_t lgrp = lbase;
    for (uint32_t r0 = 0; r0 < n; r0 += pc.T) {
        const uint32_t j = r0 + pc.tid, wi = nb + j + pc.wdelta;
        const PullNode nd = pull_decode<REAL, NARROW>(d, wi, j < n, pc.ww, lbase, lgrp);
        if constexpr (FILL)
            if (j < n) Lid[j] = nd.act ? nd.layer - lbase : PULL_NO_LAYER;
        if (nd.act) body(j, wi, nd);
    }
}

// body(slot, arc) for the parents of the node with word index wi, in parent table order: par[par_ptr[wi] .. par_ptr[wi + 1]) holds
// (slot in the previous hop) << 1 | arc, parents in slot order, lo arc before hi arc (sm_build_parents)
template <typename BODY>
__device__ __forceinline__ void pull_parents(const uint32_t* par_ptr, const uint32_t* par, uint32_t wi, BODY body)
{
    for (uint32_t k = par_ptr[wi], e = par_ptr[wi + 1]; k < e; ++k) {
        const uint32_t x = par[k];
        body(x >> 1, x & 1u);
    }
}

// a value per arc
template <typename X>
struct Pull2 {
    X lo, hi;
};
template <typename X>
__device__ __forceinline__ Pull2<X> pull_add(Pull2<X> v, Pull2<X> w) { return {v.lo + w.lo, v.hi + w.hi}; }

// One value per layer of a hop out of its slots, in two levels with a barrier between them.  The slots are cut into runs at every
// PULL_CHUNK-th slot and at every layer head; the first lane of a run folds its run from its first slot on (<= PULL_CHUNK steps), then
// the layer's head folds its layer's runs from its own on (width / PULL_CHUNK steps).  A layer of one or two nodes is one run of its head.
//   at(j)       the value of slot j                 put(j, v)   keep a run's value, j its first slot
//   comb(v, w)  v combined with the later w         get(j)      ... and read it back
//   done(l, v)  the value of layer l, at its head
//   BAR::sync() the barrier between the two levels: __syncthreads() where the pack is a workgroup's (PullBlockBar), a wave-level ordering
//               point where it is one wave's among several of a workgroup (kernels/gradsmall.hpp)
// The caller's barrier follows.
struct PullBlockBar {   // the pack is a workgroup's
    static __device__ __forceinline__ void sync() { __syncthreads(); }
};
template <typename BAR, typename REAL, typename AT, typename COMB, typename PUT, typename GET, typename DONE>
__device__ __forceinline__ void pull_layer_fold_bar(const PullPack<REAL>& pc, const uint32_t* Lid, uint32_t n, AT at, COMB comb, PUT put, GET get, DONE done)
{
    auto run_start = [&](uint32_t j, uint32_t l) { return l != PULL_NO_LAYER && (j % PULL_CHUNK == 0 || j == 0 || Lid[j - 1] != l); };
    auto is_head = [&](uint32_t j, uint32_t l) { return l != PULL_NO_LAYER && (j == 0 || Lid[j - 1] != l); };
    for (uint32_t j = pc.tid; j < n; j += pc.T) {
        const uint32_t l = Lid[j];
        if (run_start(j, l)) {
            auto v = at(j);
            for (uint32_t e = j + 1; e < n && e % PULL_CHUNK != 0 && Lid[e] == l; ++e) v = comb(v, at(e));
            put(j, v);
        }
    }
    BAR::sync();
    for (uint32_t j = pc.tid; j < n; j += pc.T) {
        const uint32_t l = Lid[j];
        if (is_head(j, l)) {
            auto v = get(j);
            for (uint32_t e = (j / PULL_CHUNK + 1) * PULL_CHUNK; e < n && Lid[e] == l; e += PULL_CHUNK) v = comb(v, get(e));
            done(l, v);
        }
    }
}
template <typename REAL, typename AT, typename COMB, typename PUT, typename GET, typename DONE>
__device__ __forceinline__ void pull_layer_fold(const PullPack<REAL>& pc, const uint32_t* Lid, uint32_t n, AT at, COMB comb, PUT put, GET get, DONE done)
{
    pull_layer_fold_bar<PullBlockBar>(pc, Lid, n, at, comb, put, get, done);
}

}  // namespace bddmma
