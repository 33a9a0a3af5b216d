// solver_sm.hpp — sum-marginals and the smooth solution for SolverT<REAL> (bdd_cuda_base.cu:788-1064: sum_marginals_cuda,
// smooth_solution_cuda): the parent tables of the pull sweeps, the two sweeps of kernels/summarg.hpp and the two entry points.  Included
// by solver_sm_f32.hip / solver_sm_f64.hip only, so that these kernels compile in translation units of their own.
#pragma once
#include "solver_impl.hpp"
#include "kernels/summarg.hpp"

namespace bddmma {

// Parents of every node, by word index (kernels/pull.hpp: pull_parents): the children of a node are slots of the next hop of its pack, so
// the parents of slot c of hop q + 1 are the nodes of hop q that name c, in slot order, lo arc before hi arc.  `word_of(p)` = word index
// of the first slot of pack p of a set; packs that share a word sequence (narrow packs of one structure) share their part of the table.
// One table may cover several pack sets (wide and huge packs share wwords).
struct SmPackSet {
    std::vector<uint32_t> pack_hop_ptr, hop_node_off;
};
template <typename WORD, typename DECODE, typename WORDOF>
static bool sm_build_parents(const std::vector<SmPackSet>& sets, const std::vector<WORD>& words, DECODE decode, WORDOF word_of, std::vector<uint32_t>& ptr,
                             std::vector<uint32_t>& par)
{
    const size_t nw = words.size();
    ptr.assign(nw + 1, 0);
    std::vector<uint8_t> seen(nw, 0);
    for (int pass = 0; pass < 2; ++pass) {
        std::vector<uint32_t> fill;
        if (pass == 1) {
            for (size_t i = 0; i < nw; ++i) ptr[i + 1] += ptr[i];   // counts (at i + 1) -> offsets
            par.assign(ptr[nw], 0);
            fill.assign(ptr.begin(), ptr.end() - 1);
            std::fill(seen.begin(), seen.end(), 0);
        }
        for (const SmPackSet& ps : sets)
        for (size_t p = 0; p + 1 < ps.pack_hop_ptr.size(); ++p) {
            const std::vector<uint32_t>& hop_node_off = ps.hop_node_off;
            const uint32_t q0 = ps.pack_hop_ptr[p], q1 = ps.pack_hop_ptr[p + 1];
            if (q0 == q1) continue;
            const size_t w0 = word_of(ps, p);
            if (w0 + (hop_node_off[q1] - hop_node_off[q0]) > nw) return false;  // the pack's words do not lie inside the word array
            if (seen[w0]) continue;   // a word sequence shared with an earlier pack (word sequences are shared whole: layout.hpp, narrow_word_off)
            seen[w0] = 1;
            for (uint32_t q = q0; q + 1 < q1; ++q) {
                const size_t wq = w0 + (hop_node_off[q] - hop_node_off[q0]), wn = w0 + (hop_node_off[q + 1] - hop_node_off[q0]);
                const uint32_t n = hop_node_off[q + 1] - hop_node_off[q], n_next = hop_node_off[q + 2] - hop_node_off[q + 1];
                for (uint32_t j = 0; j < n; ++j) {
                    uint32_t ch[2];
                    if (!decode(words[wq + j], ch)) continue;
                    for (uint32_t arc = 0; arc < 2; ++arc) {
                        if (ch[arc] >= n_next) continue;  // a sink
                        if (pass == 0) ++ptr[wn + ch[arc] + 1];
                        else par[fill[wn + ch[arc]]++] = (j << 1) | arc;
                    }
                }
            }
        }
    }
    return true;
}

template <typename REAL>
int SolverT<REAL>::sm_prepare()
{
    if (sm_ready) return BDDMMA_OK;
    HIPCHK(hipSetDevice(device));
    auto fetch = [&](int id, auto& vec) -> hipError_t {
        using T = typename std::remove_reference_t<decltype(vec)>::value_type;
        const DevField& f = dev_fields[id];
        vec.resize(f.count);
        return f.count ? hipMemcpyAsync(vec.data(), f.ptr, f.count * sizeof(T), hipMemcpyDeviceToHost, stream) : hipSuccess;
    };
    int rc;
    if (nb_.n_packs) {
        std::vector<uint32_t> words, word_off;
        std::vector<SmPackSet> sets(1);
        // (LAY_NARROW_WORD_OFF is d_pack_word_off, what the kernels index with: SolverT::init uploads it under that id)
        HIPCHK(fetch(LAY_NARROW_WORDS, words)); HIPCHK(fetch(LAY_NARROW_WORD_OFF, word_off));
        HIPCHK(fetch(LAY_NARROW_PACK_HOP_PTR, sets[0].pack_hop_ptr)); HIPCHK(fetch(LAY_NARROW_HOP_NODE_OFF, sets[0].hop_node_off));
        HIPCHK(hipStreamSynchronize(stream));
        std::vector<uint32_t> ptr, par;
        const uint32_t W = pack_width;
        const bool ok = sm_build_parents(sets, words,
                         [W](uint32_t w, uint32_t (&ch)[2]) {
                             if (w & NW_PAD) return false;
                             ch[0] = w & NW_CHILD_MASK;
                             ch[1] = (w >> NW_CHILD_BITS) & NW_CHILD_MASK;
                             if (ch[0] >= W) ch[0] = 0xFFFFFFFFu;
                             if (ch[1] >= W) ch[1] = 0xFFFFFFFFu;
                             return true;
                         },
                         [&](const SmPackSet&, size_t p) { return (size_t)word_off[p]; }, ptr, par);
        if (!ok) { err = "sum-marginals: a narrow pack's node words lie outside the word array"; return BDDMMA_ERR_STATE; }
        if ((rc = upload(&d_sm_nptr, ptr))) return rc;
        if ((rc = upload(&d_sm_npar, par))) return rc;
        HIPCHK(hipStreamSynchronize(stream));  // the uploads read host vectors that end here
    }
    if (wb_.n_packs || hb_.n_packs) {
        std::vector<uint64_t> words;
        HIPCHK(fetch(LAY_WIDE_WORDS, words));
        std::vector<SmPackSet> sets(2);  // wide packs, then huge packs: one table over wwords[slot - wide_slot_base]
        HIPCHK(fetch(LAY_WIDE_PACK_HOP_PTR, sets[0].pack_hop_ptr)); HIPCHK(fetch(LAY_WIDE_HOP_NODE_OFF, sets[0].hop_node_off));
        HIPCHK(fetch(LAY_HUGE_PACK_HOP_PTR, sets[1].pack_hop_ptr)); HIPCHK(fetch(LAY_HUGE_HOP_NODE_OFF, sets[1].hop_node_off));
        HIPCHK(hipStreamSynchronize(stream));
        std::vector<uint32_t> ptr, par;
        const uint32_t wsb = wide_slot_base;
        const bool ok = sm_build_parents(sets, words,
                         [](uint64_t w, uint32_t (&ch)[2]) {
                             const uint64_t lo = w & WW_CHILD_MASK, hi = (w >> WW_CHILD_BITS) & WW_CHILD_MASK;
                             ch[0] = lo < WW_TOP ? (uint32_t)lo : 0xFFFFFFFFu;
                             ch[1] = hi < WW_TOP ? (uint32_t)hi : 0xFFFFFFFFu;
                             return true;
                         },
                         [&](const SmPackSet& ps, size_t p) { return (size_t)(ps.hop_node_off[ps.pack_hop_ptr[p]] - wsb); }, ptr, par);
        if (!ok) { err = "sum-marginals: a wide pack's node words lie outside the word array"; return BDDMMA_ERR_STATE; }
        if ((rc = upload(&d_sm_wptr, ptr))) return rc;
        if ((rc = upload(&d_sm_wpar, par))) return rc;
        HIPCHK(hipStreamSynchronize(stream));
    }
    if (hb_.n_packs && (rc = dalloc(&d_sm_scratch, (uint64_t)hb_.n_packs * sm_lds_bytes(sizeof(REAL), huge_pack_width)))) return rc;
    if ((rc = pull_wide_lds("sum-marginals", sm_fwd_sweep(), sm_bwd_sweep()))) return rc;
    sm_ready = true;
    return BDDMMA_OK;
}

template <typename REAL>
PullSweep<REAL> SolverT<REAL>::sm_fwd_sweep() const
{
    return {&k_sm_fwd<REAL, true, false>, &k_sm_fwd<REAL, false, false>, &k_sm_fwd<REAL, false, true>, &sm_lds_bytes, d_sm_scratch};
}
template <typename REAL>
PullSweep<REAL> SolverT<REAL>::sm_bwd_sweep() const
{
    return {&k_sm_bwd<REAL, true, false>, &k_sm_bwd<REAL, false, false>, &k_sm_bwd<REAL, false, true>, &sm_lds_bytes, d_sm_scratch};
}

template <typename REAL>
int SolverT<REAL>::sm_launch_fwd()
{
    if (int rc = launch_pull(sm_fwd_sweep())) return rc;
    fwd_valid = false;  // the stored costs from root are log-partition values now
    return BDDMMA_OK;
}

template <typename REAL>
int SolverT<REAL>::sm_launch_bwd()
{
    bwd_valid = lb_valid = false;  // ... and the costs from terminal; the cached bound goes with them (flush_backward_states, bdd_cuda_base.cu:1011)
    lb_cached = false;
    ++lb_gen;
    return launch_pull(sm_bwd_sweep());
}

template <typename REAL>
int SolverT<REAL>::sm_sum_marginals(int sorted, int log_probs, int32_t* var, void* sm0, void* sm1, int on_device)
{
    HIPCHK(hipSetDevice(device));
    int rc;
    if ((rc = sm_prepare())) return rc;
    if ((rc = sm_launch_fwd())) return rc;
    if ((rc = sm_launch_bwd())) return rc;
    if (!log_probs) hipLaunchKernelGGL((k_exp_pair<REAL>), dim3(cdiv(n_layers, 256)), dim3(256), 0, stream, d_tmp0, d_tmp1, (uint32_t)n_layers);
    return marginals_out(sorted, var, sm0, sm1, on_device);
}

template <typename REAL>
int SolverT<REAL>::sm_smooth_solution(void* out, int on_device)
{
    HIPCHK(hipSetDevice(device));
    int rc;
    if ((rc = sm_prepare())) return rc;
    if ((rc = sm_launch_fwd())) return rc;
    if ((rc = sm_launch_bwd())) return rc;
    REAL* dst = on_device ? (REAL*)out : d_tmp0;  // in place over the lo values when the result goes to the host
    hipLaunchKernelGGL((k_smooth_solution<REAL>), dim3(cdiv(n_layers, 256)), dim3(256), 0, stream, (const REAL*)d_tmp0, (const REAL*)d_tmp1, dst, (uint32_t)n_layers);
    if (!on_device) return copy_out(out, dst, n_layers * sizeof(REAL), 0);
    HIPCHK(hipStreamSynchronize(stream));
    return BDDMMA_OK;
}

}  // namespace bddmma
