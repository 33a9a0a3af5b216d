// solver_gr.hpp — the single-shot backward operators of the learned solver for SolverT<REAL> (bdd_cuda_learned_mma.h:82-110:
// grad_mm_diff_all_hops, grad_lower_bound_per_bdd, grad_distribute_delta, grad_cost_perturbation): the two sweeps of kernels/gradmm.hpp and
// the four entry points.  Included by solver_gr_f32.hip / solver_gr_f64.hip only, so that these kernels compile in translation units of
// their own.  The parent tables are the sum-marginals' (SolverT::sm_prepare, defined in the solver_sm translation units).
#pragma once
#include "solver_impl.hpp"
#include "kernels/gradmm.hpp"

namespace bddmma {

template <typename REAL>
int SolverT<REAL>::gr_prepare()
{
    if (gr_ready) return BDDMMA_OK;
    HIPCHK(hipSetDevice(device));
    int rc;
    if ((rc = sm_prepare())) return rc;
    if ((rc = gr_inputs(false))) return rc;
    if (!d_gr_arg && (rc = dalloc(&d_gr_arg, 2 * n_layers))) return rc;
    if (hb_.n_packs && !d_gr_scratch && (rc = dalloc(&d_gr_scratch, (uint64_t)hb_.n_packs * gr_lds_bytes(sizeof(REAL), huge_pack_width)))) return rc;
    if ((rc = pull_wide_lds("grad_min_marginal_diff", gr_down_sweep(), gr_up_sweep()))) return rc;
    gr_ready = true;
    return BDDMMA_OK;
}

template <typename REAL>
int SolverT<REAL>::gr_inputs(bool second)
{
    int rc;
    if (!d_gr_in0 && (rc = dalloc(&d_gr_in0, n_layers))) return rc;
    if (second && !d_gr_in1 && (rc = dalloc(&d_gr_in1, n_layers))) return rc;
    return BDDMMA_OK;
}

// Both sweeps read d_gr_in0 (the incoming gradient) and write d_tmp0 / d_tmp1 (grad_lo / grad_hi); d_gr_arg goes from the first to the second.
template <typename REAL>
PullSweep<REAL, const REAL*, REAL*, REAL*, uint32_t*> SolverT<REAL>::gr_down_sweep() const
{
    return {&k_gr_down<REAL, true, false>, &k_gr_down<REAL, false, false>, &k_gr_down<REAL, false, true>, &gr_lds_bytes, d_gr_scratch};
}
template <typename REAL>
PullSweep<REAL, const REAL*, REAL*, REAL*, const uint32_t*> SolverT<REAL>::gr_up_sweep() const
{
    return {&k_gr_up<REAL, true, false>, &k_gr_up<REAL, false, false>, &k_gr_up<REAL, false, true>, &gr_lds_bytes, d_gr_scratch};
}
template <typename REAL>
int SolverT<REAL>::gr_launch_down()
{
    return launch_pull(gr_down_sweep(), d_gr_in0, d_tmp0, d_tmp1, d_gr_arg);
}
template <typename REAL>
int SolverT<REAL>::gr_launch_up()
{
    return launch_pull(gr_up_sweep(), d_gr_in0, d_tmp0, d_tmp1, d_gr_arg);
}

// An incoming gradient (n values) -> dst on the device; BDDMMA_ERR_INVALID_ARGUMENT when a value is not finite (host input: before anything
// is copied).  Nothing the solver's state depends on is written.
template <typename REAL>
int SolverT<REAL>::gr_load(REAL* dst, const void* src, uint64_t n, int on_dev, const char* what)
{
    if (!on_dev) {
        const REAL* h = (const REAL*)src;
        for (uint64_t i = 0; i < n; ++i)
            if (!std::isfinite(h[i])) {
                err = std::string(what) + "[" + std::to_string(i) + "] is not finite";
                return BDDMMA_ERR_INVALID_ARGUMENT;
            }
    }
    if (n) HIPCHK(hipMemcpyAsync(dst, src, n * sizeof(REAL), on_dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, stream));
    if (on_dev && n) {
        HIPCHK(hipMemsetAsync(d_counts, 0, sizeof(uint32_t), stream));
        hipLaunchKernelGGL((k_count_nonfinite<REAL>), dim3(cdiv(n, 256)), dim3(256), 0, stream, (const REAL*)dst, d_counts, (uint32_t)n);
        uint32_t bad = 0;
        HIPCHK(hipMemcpyAsync(&bad, d_counts, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
        HIPCHK(hipStreamSynchronize(stream));
        if (bad) {
            err = std::to_string(bad) + " values of " + what + " are not finite";
            return BDDMMA_ERR_INVALID_ARGUMENT;
        }
    } else {
        HIPCHK(hipStreamSynchronize(stream));  // the copy reads the caller's host array
    }
    return BDDMMA_OK;
}

template <typename REAL>
int SolverT<REAL>::gr_load_device(const LoadSpec* specs, int count, uint64_t n, const char* me)
{
    if (count <= 0 || n == 0) return BDDMMA_OK;
    LoadArrays<REAL> a{};
    a.n = (uint32_t)n;
    a.count = (uint32_t)count;
    for (int k = 0; k < count; ++k) {
        a.src[k] = (const REAL*)specs[k].src;
        a.dst[k] = specs[k].dst;
        if (specs[k].weights) a.nonneg |= 1u << k;
    }
    uint32_t bad[LOAD_MAX_ARRAYS] = {};
    HIPCHK(hipMemsetAsync(d_counts, 0, sizeof(bad), stream));
    // a 16-byte vector per thread and trip, at most 2048 workgroups: the rest by the grid-stride loop
    const uint64_t vecs = cdiv(n, 16 / sizeof(REAL));
    hipLaunchKernelGGL((k_load_checked<REAL>), dim3((uint32_t)std::min<uint64_t>(cdiv(vecs, 256), 2048)), dim3(256), 0, stream, a, d_counts);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(bad, d_counts, sizeof(bad), hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));
    for (int k = 0; k < count; ++k) {
        if (!bad[k]) continue;
        err = specs[k].weights ? std::string(me) + ": " + std::to_string(bad[k]) + " of the " + specs[k].what + " are negative or not finite"
                               : std::to_string(bad[k]) + " values of " + me + ": " + specs[k].what + " are not finite";
        return BDDMMA_ERR_INVALID_ARGUMENT;
    }
    return BDDMMA_OK;
}

template <typename REAL>
int SolverT<REAL>::gr_min_marginal_diff(const void* grad_mm, void* grad_lo, void* grad_hi, int on_device)
{
    HIPCHK(hipSetDevice(device));
    int rc;
    if ((rc = gr_prepare())) return rc;
    if ((rc = gr_load(d_gr_in0, grad_mm, n_layers, on_device, "grad_min_marginal_diff: grad_mm"))) return rc;
    // the stored potentials of the plain sweeps; a sum-marginals call has overwritten both and left both invalid
    if ((rc = forward_run())) return rc;
    if ((rc = backward_run())) return rc;
    if ((rc = gr_launch_down())) return rc;
    if ((rc = gr_launch_up())) return rc;
    const hipMemcpyKind k = on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    HIPCHK(hipMemcpyAsync(grad_lo, d_tmp0, n_layers * sizeof(REAL), k, stream));
    HIPCHK(hipMemcpyAsync(grad_hi, d_tmp1, n_layers * sizeof(REAL), k, stream));
    HIPCHK(hipStreamSynchronize(stream));
    return BDDMMA_OK;
}

template <typename REAL>
int SolverT<REAL>::gr_lower_bound_per_bdd(const void* grad_lb, void* grad_lo, void* grad_hi, int smooth, int on_device)
{
    HIPCHK(hipSetDevice(device));
    int rc;
    if ((rc = gr_inputs(false))) return rc;
    // (the n_bdds values fit the layer-sized buffer: every BDD has at least one layer)
    if ((rc = gr_load(d_gr_in0, grad_lb, n_bdds, on_device, "grad_lower_bound_per_bdd: grad_lb_per_bdd"))) return rc;
    REAL* const lo = on_device ? (REAL*)grad_lo : d_tmp1;
    REAL* const hi = on_device ? (REAL*)grad_hi : d_tmp0;
    const dim3 g(cdiv(n_layers, 256)), b(256);
    if (smooth) {
        if ((rc = sm_prepare())) return rc;
        if ((rc = sm_launch_fwd())) return rc;
        if ((rc = sm_launch_bwd())) return rc;
        hipLaunchKernelGGL((k_smooth_solution<REAL>), g, b, 0, stream, (const REAL*)d_tmp0, (const REAL*)d_tmp1, d_tmp0, (uint32_t)n_layers);
        hipLaunchKernelGGL((k_grad_lb<REAL, REAL>), g, b, 0, stream, (const REAL*)d_tmp0, (const REAL*)d_gr_in0, d_bdd, lo, hi, (uint32_t)n_layers);
    } else {
        if ((rc = backward_run())) return rc;
        HIPCHK(hipMemsetAsync(d_sol, 0, n_layers, stream));
        if ((rc = launch_fwd(FWD_SOLUTION, nullptr, REAL(0), BDDMMA_K_OTHER))) return rc;
        hipLaunchKernelGGL((k_grad_lb<REAL, char>), g, b, 0, stream, (const char*)d_sol, (const REAL*)d_gr_in0, d_bdd, lo, hi, (uint32_t)n_layers);
    }
    HIPCHK(hipGetLastError());
    if (!on_device) {
        HIPCHK(hipMemcpyAsync(grad_lo, lo, n_layers * sizeof(REAL), hipMemcpyDeviceToHost, stream));
        HIPCHK(hipMemcpyAsync(grad_hi, hi, n_layers * sizeof(REAL), hipMemcpyDeviceToHost, stream));
    }
    HIPCHK(hipStreamSynchronize(stream));
    return BDDMMA_OK;
}

template <typename REAL>
int SolverT<REAL>::gr_distribute_delta(const void* grad_lo, const void* grad_hi, void* grad_deferred_mm, int on_device)
{
    HIPCHK(hipSetDevice(device));
    if (!mm_consumed_valid) {
        err = "grad_distribute_delta: no distribute_delta has run on this solver (its deferred differences are what this call reads)";
        return BDDMMA_ERR_STATE;
    }
    int rc;
    if ((rc = gr_inputs(true))) return rc;
    if (on_device) {
        const LoadSpec in[2] = {{d_gr_in0, grad_lo, "grad_lo", false}, {d_gr_in1, grad_hi, "grad_hi", false}};
        if ((rc = gr_load_device(in, 2, n_layers, "grad_distribute_delta"))) return rc;
    } else {
        if ((rc = gr_load(d_gr_in0, grad_lo, n_layers, 0, "grad_distribute_delta: grad_lo"))) return rc;
        if ((rc = gr_load(d_gr_in1, grad_hi, n_layers, 0, "grad_distribute_delta: grad_hi"))) return rc;
    }
    REAL* const dst = on_device ? (REAL*)grad_deferred_mm : d_tmp0;
    hipLaunchKernelGGL((k_grad_distribute<REAL>), dim3(cdiv(n_layers, 256)), dim3(256), 0, stream, (const REAL*)d_gr_in0, (const REAL*)d_gr_in1,
                       (const REAL*)d_mm_consumed, d_lpos, dst, (uint32_t)n_layers);
    HIPCHK(hipGetLastError());
    if (!on_device) return copy_out(grad_deferred_mm, dst, n_layers * sizeof(REAL), 0);
    HIPCHK(hipStreamSynchronize(stream));
    return BDDMMA_OK;
}

template <typename REAL>
int SolverT<REAL>::gr_cost_perturbation(const void* grad_lo, const void* grad_hi, void* grad_lo_pert, void* grad_hi_pert, int on_device)
{
    HIPCHK(hipSetDevice(device));
    int rc;
    if ((rc = gr_inputs(true))) return rc;
    if (on_device) {
        const LoadSpec in[2] = {{d_gr_in0, grad_lo, "grad_lo", false}, {d_gr_in1, grad_hi, "grad_hi", false}};
        if ((rc = gr_load_device(in, 2, n_layers, "grad_cost_perturbation"))) return rc;
    } else {
        if ((rc = gr_load(d_gr_in0, grad_lo, n_layers, 0, "grad_cost_perturbation: grad_lo"))) return rc;
        if ((rc = gr_load(d_gr_in1, grad_hi, n_layers, 0, "grad_cost_perturbation: grad_hi"))) return rc;
    }
    REAL* const lo = on_device ? (REAL*)grad_lo_pert : d_delta_c;  // 2V scratch of the explicit forward_mm / backward_mm calls
    REAL* const hi = on_device ? (REAL*)grad_hi_pert : d_delta_c + n_vars;
    hipLaunchKernelGGL((k_grad_perturb<REAL>), dim3(cdiv(n_vars, 256)), dim3(256), 0, stream, (const REAL*)d_gr_in0, (const REAL*)d_gr_in1, d_var_ptr, d_var_layers,
                       lo, hi, (uint32_t)n_vars);
    HIPCHK(hipGetLastError());
    if (!on_device) {
        HIPCHK(hipMemcpyAsync(grad_lo_pert, lo, n_vars * sizeof(REAL), hipMemcpyDeviceToHost, stream));
        HIPCHK(hipMemcpyAsync(grad_hi_pert, hi, n_vars * sizeof(REAL), hipMemcpyDeviceToHost, stream));
    }
    HIPCHK(hipStreamSynchronize(stream));
    return BDDMMA_OK;
}

}  // namespace bddmma
