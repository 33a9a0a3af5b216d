// solver_gi.hpp — the backward of the learned iterations for SolverT<REAL> (bdd_cuda_learned_mma.cu:308-385, grad_iterations): the reverse
// sweeps of kernels/graditer.hpp around replays of the iterations themselves.  Included by solver_gi_f32.hip / solver_gi_f64.hip only, so
// that these kernels compile in translation units of their own.  The parent tables are the sum-marginals' (SolverT::sm_prepare).
#pragma once
#include "solver_impl.hpp"
#include "kernels/graditer.hpp"

namespace bddmma {

// Every buffer of the call, allocated before the solver is touched: one block of per-layer / per-slot / per-variable arrays (first call) and
// the caches of {lo, hi} + deferred differences (3 L each; more only when a call asks for more than any call before it).
template <typename REAL>
int SolverT<REAL>::gi_prepare(uint64_t n_caches)
{
    HIPCHK(hipSetDevice(device));
    int rc;
    const uint64_t L = n_layers, N = n_slots, V = n_vars;
    if (!gi_ready) {
        if ((rc = sm_prepare())) return rc;
        const PullSweep<REAL, GiArgs<REAL>> dn{&k_gi_down<REAL, true, false, true>, &k_gi_down<REAL, false, false, true>, &k_gi_down<REAL, false, true, true>, &gi_lds_bytes, nullptr};
        const PullSweep<REAL, GiArgs<REAL>> dt{&k_gi_down<REAL, true, false, false>, &k_gi_down<REAL, false, false, false>, &k_gi_down<REAL, false, true, false>, &gi_lds_bytes, nullptr};
        const PullSweep<REAL, GiArgs<REAL>> up{&k_gi_up<REAL, true, false>, &k_gi_up<REAL, false, false>, &k_gi_up<REAL, false, true>, &gi_lds_bytes, nullptr};
        if ((rc = pull_wide_lds("grad_learned_iterations", dn, up)) || (rc = pull_wide_lds("grad_learned_iterations", dt, up))) return rc;
        if (!d_alpha_ent && (rc = dalloc(&d_alpha_ent, L))) return rc;
        if (!d_omega_lay && (rc = dalloc(&d_omega_lay, L))) return rc;
        if (hb_.n_packs && !d_gi_scratch && (rc = dalloc(&d_gi_scratch, (uint64_t)hb_.n_packs * gi_lds_bytes(sizeof(REAL), huge_pack_width)))) return rc;
        if ((rc = dalloc(&d_gi, 20 * L + 3 * N + 6 * V + 1))) return rc;  // the take() list of gi_grad_learned_iterations
        gi_ready = true;
    }
    while (gi_caches.size() < n_caches) {
        REAL* p = nullptr;
        if ((rc = dalloc(&p, 3 * L))) return rc;
        gi_caches.push_back(p);
    }
    return BDDMMA_OK;
}

template <typename REAL>
int SolverT<REAL>::gi_grad_learned_iterations(const void* w, int w_dev, double omega, const void* omega_vec, int ov_dev, void* grad_lo, void* grad_hi, void* grad_mm,
                                              void* grad_w_out, void* grad_omega_out, uint64_t after, uint64_t n, uint64_t num_caches, int on_device)
{
    HIPCHK(hipSetDevice(device));
    int rc;
    const char* const me = "grad_learned_iterations";
    if (!w || !grad_lo || !grad_hi || !grad_mm || !grad_w_out || !grad_omega_out) { err = std::string(me) + ": null pointer"; return BDDMMA_ERR_INVALID_ARGUMENT; }
    if (*lbfgs_attached > 0) { err = std::string(me) + ": an L-BFGS wrapper is attached to this solver"; return BDDMMA_ERR_STATE; }
    if (run_stop) { err = std::string(me) + ": run_solver is queueing iterations"; return BDDMMA_ERR_STATE; }
    const bool ov = omega_vec != nullptr;
    if (!ov && !(omega >= 0.0 && omega < std::numeric_limits<double>::infinity())) { err = std::string(me) + ": omega is negative or not finite"; return BDDMMA_ERR_INVALID_ARGUMENT; }
    // the reference's interval rule (bdd_cuda_learned_mma.h:12-23)
    const uint64_t nc = std::max<uint64_t>(num_caches, 1);
    const uint64_t interval = std::max<uint64_t>((n + nc - 1) / nc, 1);
    const uint64_t max_cached = n ? std::min(interval * (nc - 1), n - 1) : 0;
    const uint64_t n_cached = n ? 1 + max_cached / interval : 0;
    if (ov && !ov_ready) {
        if ((rc = ov_prepare())) return rc;
        ov_ready = true;
    }
    if ((rc = gi_prepare(n_cached))) return rc;
    const uint64_t L = n_layers, N = n_slots, V = n_vars;
    REAL* p = d_gi;
    auto take = [&](uint64_t k) { REAL* r = p; p += k; return r; };
    REAL *s_lohi = take(2 * L), *s_mm = take(L), *s_dlay = take(2 * L), *s_dvar = take(2 * V);          // the entry state
    REAL *c0 = take(2 * L), *c1 = take(2 * L), *d0 = take(L), *mm1 = take(L), *mm2 = take(L);            // what the reverse sweeps read
    REAL *T0 = take(N), *gT = take(N), *gF = take(N), *S = take(2 * V), *gSv = take(2 * V), *gS = take(2 * L);
    REAL *alpha = take(L), *g_lo = take(L), *g_hi = take(L), *g_mm = take(L), *g_alpha = take(L), *g_omega = take(L), *g_omega1 = take(1);
    // ---- the arguments: nothing below this block fails on them, nothing in it writes the solver's state
    // (load_layer_values names its caller "learned_iterations: ...")
    if (w_dev && on_device && (!ov || ov_dev)) {
        // all on the device: one launch copies and checks them, one read of the counts (same order, same first offender, same words)
        LoadSpec in[LOAD_MAX_ARRAYS];
        int k = 0;
        if (ov) in[k++] = {d_omega_lay, omega_vec, "omega_vec", true};
        in[k++] = {alpha, w, "dist_weights", true};
        in[k++] = {g_lo, grad_lo, "grad_lo", false};
        in[k++] = {g_hi, grad_hi, "grad_hi", false};
        in[k++] = {g_mm, grad_mm, "grad_mm", false};
        if ((rc = gr_load_device(in, k, L, me))) return rc;
    } else {
        if (ov && (rc = load_layer_values(d_omega_lay, omega_vec, ov_dev, "omega_vec"))) { err = "grad_" + err; return rc; }
        if ((rc = load_layer_values(alpha, w, w_dev, "dist_weights"))) { err = "grad_" + err; return rc; }
        if ((rc = gr_load(g_lo, grad_lo, L, on_device, "grad_learned_iterations: grad_lo"))) return rc;
        if ((rc = gr_load(g_hi, grad_hi, L, on_device, "grad_learned_iterations: grad_hi"))) return rc;
        if ((rc = gr_load(g_mm, grad_mm, L, on_device, "grad_learned_iterations: grad_mm"))) return rc;
    }
    const hipMemcpyKind out_kind = on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    const uint64_t n_omega = ov ? L : 1;
    HIPCHK(hipMemsetAsync(g_alpha, 0, L * sizeof(REAL), stream));
    HIPCHK(hipMemsetAsync(g_omega, 0, (L + 1) * sizeof(REAL), stream));
    if (n == 0) {
        HIPCHK(hipMemcpyAsync(grad_w_out, g_alpha, L * sizeof(REAL), out_kind, stream));
        HIPCHK(hipMemcpyAsync(grad_omega_out, g_omega, n_omega * sizeof(REAL), out_kind, stream));
        HIPCHK(hipStreamSynchronize(stream));
        return BDDMMA_OK;
    }
    const dim3 gl(cdiv(L, 256)), gv(cdiv(V, 256)), blk(256);
    const hipMemcpyKind dd = hipMemcpyDeviceToDevice;
    hipLaunchKernelGGL((k_layers_to_entries<REAL>), gl, blk, 0, stream, (const REAL*)alpha, d_lpos, d_alpha_ent, (uint32_t)L);
    // ---- the entry state: arc costs, deferred differences, delta
    HIPCHK(hipMemcpyAsync(s_lohi, d_lohi, 2 * L * sizeof(REAL), dd, stream));
    HIPCHK(hipMemcpyAsync(s_mm, d_mm_binned, L * sizeof(REAL), dd, stream));
    HIPCHK(hipMemcpyAsync(s_dlay, d_delta_lay, 2 * L * sizeof(REAL), dd, stream));
    HIPCHK(hipMemcpyAsync(s_dvar, d_delta_var, 2 * V * sizeof(REAL), dd, stream));
    const bool s_dvar_valid = delta_var_valid;
    const REAL omega_r = (REAL)omega;
    auto restore = [&](const REAL* lohi, const REAL* mm) -> int {
        HIPCHK(hipMemcpyAsync(d_lohi, lohi, 2 * L * sizeof(REAL), dd, stream));
        HIPCHK(hipMemcpyAsync(d_mm_binned, mm, L * sizeof(REAL), dd, stream));
        costs_changed();
        return BDDMMA_OK;
    };
    auto leave = [&](int code) -> int {  // the entry state back, whatever happened
        const std::string keep = err;
        (void)restore(s_lohi, s_mm);
        (void)hipMemcpyAsync(d_delta_lay, s_dlay, 2 * L * sizeof(REAL), dd, stream);
        (void)hipMemcpyAsync(d_delta_var, s_dvar, 2 * V * sizeof(REAL), dd, stream);
        delta_var_valid = s_dvar_valid;
        (void)hipStreamSynchronize(stream);
        if (code) err = keep;
        return code;
    };
    // a device error after the solver has been touched: the entry state back first
#define GICHK(expr)                                                        \
    do {                                                                   \
        hipError_t e_ = (expr);                                            \
        if (e_ != hipSuccess) {                                            \
            err = std::string(#expr) + ": " + hipGetErrorString(e_);       \
            return leave(BDDMMA_ERR_DEVICE);                               \
        }                                                                  \
    } while (0)
    // bddmma_time_kernel kinds 13 - 17 (gi_time_kernel): the launch group of that kind runs gi_timing.reps times between two events
    auto timed = [&](int kind, auto&& fn) -> int {
        if (gi_timing.kind != kind) return fn();
        if (int r = fn()) return r;  // warm-up
        if (hipEventRecord(ev_t0, stream) != hipSuccess) return BDDMMA_ERR_DEVICE;
        for (uint64_t i = 0; i < gi_timing.reps; ++i)
            if (int r = fn()) return r;
        if (hipEventRecord(ev_t1, stream) != hipSuccess || hipEventSynchronize(ev_t1) != hipSuccess) return BDDMMA_ERR_DEVICE;
        return hipEventElapsedTime(&gi_timing.ms, ev_t0, ev_t1) == hipSuccess ? BDDMMA_OK : BDDMMA_ERR_DEVICE;
    };
    auto iterate = [&]() -> int {
        weighted_exchange();
        if (int r = mma_forward(omega_r, d_delta_lay, ov)) return r;
        weighted_exchange();
        return mma_backward(omega_r, d_delta_lay, ov);
    };
    auto to_layers = [&](REAL* dst) { hipLaunchKernelGGL((k_entries_to_layers<REAL>), gl, blk, 0, stream, (const REAL*)d_mm_binned, d_lpos, dst, (uint32_t)L); };
    // the elementwise part of a pass's reverse: before the sweep the sums of what it consumed, behind it the gradient of that
    auto sums = [&](const REAL* dl) { hipLaunchKernelGGL((k_gi_sums<REAL>), gv, blk, 0, stream, dl, d_var_ptr, d_var_layers, S, (uint32_t)V); };
    auto consumed = [&](const REAL* dl) {
        hipLaunchKernelGGL((k_gi_var_sums<REAL>), gv, blk, 0, stream, (const REAL*)gS, d_var_ptr, d_var_layers, gSv, (uint32_t)V);
        hipLaunchKernelGGL((k_gi_gd<REAL>), gl, blk, 0, stream, dl, (const REAL*)gSv, d_var, g_mm, (uint32_t)L);
    };
    GiArgs<REAL> a{};
    a.S = S; a.var = d_var; a.alpha = alpha; a.omega_lay = ov ? d_omega_lay : nullptr; a.omega = omega_r;
    a.g_lo = g_lo; a.g_hi = g_hi; a.g_mm = g_mm; a.gS = gS; a.g_alpha = g_alpha; a.g_omega = g_omega;
    const PullSweep<REAL, GiArgs<REAL>> dn{&k_gi_down<REAL, true, false, true>, &k_gi_down<REAL, false, false, true>, &k_gi_down<REAL, false, true, true>, &gi_lds_bytes, d_gi_scratch};
    const PullSweep<REAL, GiArgs<REAL>> dt{&k_gi_down<REAL, true, false, false>, &k_gi_down<REAL, false, false, false>, &k_gi_down<REAL, false, true, false>, &gi_lds_bytes, d_gi_scratch};
    const PullSweep<REAL, GiArgs<REAL>> up{&k_gi_up<REAL, true, false>, &k_gi_up<REAL, false, false>, &k_gi_up<REAL, false, true>, &gi_lds_bytes, d_gi_scratch};

    for (uint64_t i = 0; i < after; ++i)
        if ((rc = iterate())) return leave(rc);
    const uint64_t last_cached = (n_cached - 1) * interval;  // <= max_cached: nobody reads an iteration replayed past it
    for (uint64_t it = 0; it <= last_cached; ++it) {
        if (it % interval == 0) {
            REAL* c = gi_caches[it / interval];
            GICHK(hipMemcpyAsync(c, d_lohi, 2 * L * sizeof(REAL), dd, stream));
            GICHK(hipMemcpyAsync(c + 2 * L, d_mm_binned, L * sizeof(REAL), dd, stream));
        }
        if (it < last_cached && (rc = iterate())) return leave(rc);
    }
    GICHK(hipMemsetAsync(gT, 0, N * sizeof(REAL), stream));
    for (uint64_t itr = n; itr-- > 0;) {
        // the input of iteration itr: the nearest cache, replayed forward
        const uint64_t ci = std::min(itr / interval, n_cached - 1);
        if ((rc = restore(gi_caches[ci], gi_caches[ci] + 2 * L))) return leave(rc);
        for (uint64_t k = ci * interval; k < itr; ++k)
            if ((rc = iterate())) return leave(rc);
        // the iteration itself, keeping what its two reverse sweeps read
        if ((rc = backward_run())) return leave(rc);
        GICHK(hipMemcpyAsync(T0, d_T, N * sizeof(REAL), dd, stream));
        GICHK(hipMemcpyAsync(c0, d_lohi, 2 * L * sizeof(REAL), dd, stream));
        to_layers(d0);
        weighted_exchange();
        if ((rc = mma_forward(omega_r, d_delta_lay, ov))) return leave(rc);
        GICHK(hipMemcpyAsync(c1, d_lohi, 2 * L * sizeof(REAL), dd, stream));
        to_layers(mm1);
        weighted_exchange();
        if ((rc = mma_backward(omega_r, d_delta_lay, ov))) return leave(rc);
        to_layers(mm2);
        // the reverse of the backward pass: F of the forward pass, T of the new costs
        sums(mm1);
        GICHK(hipMemsetAsync(gF, 0, N * sizeof(REAL), stream));
        a.F = d_F; a.T = d_T; a.pre = c1; a.post = d_lohi; a.mm = mm2; a.g_in = gT; a.g_out = gF;
        if ((rc = timed(13, [&]() { return launch_pull(dn, a); }))) return leave(rc);
        consumed(mm1);
        // the reverse of the forward pass: the same F, the T it read
        sums(d0);
        GICHK(hipMemsetAsync(gT, 0, N * sizeof(REAL), stream));
        a.T = T0; a.pre = c0; a.post = c1; a.mm = mm1; a.g_in = gF; a.g_out = gT;
        if ((rc = timed(14, [&]() { return launch_pull(up, a); }))) return leave(rc);
        consumed(d0);
    }
    // what is left of gT goes through T(lo, hi) of the first tracked iteration's input: c0 and T0 still hold them
    a.T = T0; a.post = c0; a.g_in = gT; a.g_out = nullptr;
    if ((rc = timed(15, [&]() { return launch_pull(dt, a); }))) return leave(rc);
    if (gi_timing.kind == 16 || gi_timing.kind == 17) {
        // what one reversed iteration does besides its sweeps, once more behind them (the copies are idempotent here): 16 the copies and
        // memsets that keep what the reverse reads, 17 the six elementwise launches
        auto copies = [&]() -> int {
            hipError_t e = hipMemcpyAsync(T0, d_T, N * sizeof(REAL), dd, stream);
            if (e == hipSuccess) e = hipMemcpyAsync(c0, d_lohi, 2 * L * sizeof(REAL), dd, stream);
            if (e == hipSuccess) e = hipMemcpyAsync(c1, d_lohi, 2 * L * sizeof(REAL), dd, stream);
            to_layers(d0); to_layers(mm1); to_layers(mm2);
            if (e == hipSuccess) e = hipMemsetAsync(gF, 0, N * sizeof(REAL), stream);
            if (e == hipSuccess) e = hipMemsetAsync(gT, 0, N * sizeof(REAL), stream);
            return e == hipSuccess ? BDDMMA_OK : BDDMMA_ERR_DEVICE;
        };
        auto elementwise = [&]() -> int { sums(mm1); consumed(mm1); sums(d0); consumed(d0); return BDDMMA_OK; };
        if ((rc = timed(16, copies)) || (rc = timed(17, elementwise))) return leave(rc);
    }
    if (!ov) hipLaunchKernelGGL((k_gi_omega_sum<REAL>), dim3(1), dim3(256), 0, stream, (const REAL*)g_omega, g_omega1, (uint32_t)L);
    GICHK(hipGetLastError());
    GICHK(hipMemcpyAsync(grad_lo, g_lo, L * sizeof(REAL), out_kind, stream));
    GICHK(hipMemcpyAsync(grad_hi, g_hi, L * sizeof(REAL), out_kind, stream));
    GICHK(hipMemcpyAsync(grad_mm, g_mm, L * sizeof(REAL), out_kind, stream));
    GICHK(hipMemcpyAsync(grad_w_out, g_alpha, L * sizeof(REAL), out_kind, stream));
    GICHK(hipMemcpyAsync(grad_omega_out, ov ? g_omega : g_omega1, n_omega * sizeof(REAL), out_kind, stream));
    return leave(BDDMMA_OK);
#undef GICHK
}

// bddmma_time_kernel kinds 13 - 17: one reversed iteration (one tracked iteration, one cache, zero incoming gradients, isotropic weights) in
// which the launch group of that kind is repeated between two events: 13 k_gi_down, 14 k_gi_up, 15 the final through-T sweep, 16 the
// copies and memsets that keep what the reverse reads, 17 the elementwise launches.  The solver's state is that of the entry on return.
template <typename REAL>
int SolverT<REAL>::gi_time_kernel(int kind, uint64_t reps, double* ms)
{
    HIPCHK(hipSetDevice(device));
    const uint64_t L = n_layers;
    REAL* buf = nullptr;
    HIPCHK(hipMalloc((void**)&buf, (6 * L + 1) * sizeof(REAL)));
    hipError_t e = hipMemsetAsync(buf, 0, (6 * L + 1) * sizeof(REAL), stream);
    hipLaunchKernelGGL((k_isotropic_alpha<REAL>), dim3(cdiv(L, 256)), dim3(256), 0, stream, d_var, d_nbdds, buf, (uint32_t)L);
    int rc = e == hipSuccess ? BDDMMA_OK : BDDMMA_ERR_DEVICE;
    gi_timing.kind = kind;
    gi_timing.reps = reps;
    gi_timing.ms = 0.f;
    if (!rc) rc = gi_grad_learned_iterations(buf, 1, 0.5, nullptr, 0, buf + L, buf + 2 * L, buf + 3 * L, buf + 4 * L, buf + 5 * L, 0, 1, 1, 1);
    gi_timing.kind = 0;
    *ms = gi_timing.ms;
    (void)hipFree(buf);
    return rc;
}

}  // namespace bddmma
