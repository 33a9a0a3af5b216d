// kernels/gradsmall.hpp — the backward of the learned iterations for a batch of one-workgroup instances in ONE launch
// (bddmma_grad_learned_iterations_batch; BatchT::grad_learned_iterations, solver_bt.hpp), and with every member's own iteration counts
// (bddmma_grad_learned_iterations_counts_batch; BatchT::grad_learned_iterations_counts: the two kernels at the end).  Behind kernels.hpp and
// graditer.hpp; the kernels themselves are instantiated in solver_gs_f32.hip / solver_gs_f64.hip only.
//
// Workgroup b runs member b through what SolverT::gi_grad_learned_iterations does with ~25 launches and copies per tracked iteration; every
// launch or copy of that path is a phase between two __syncthreads() here:
//   forward   the n tracked iterations once by small_iterate<.., LEARNED, RECORD> (kernels/small.hpp), which writes what the reverse of each
//             iteration reads to the member's slab of the batch workspace — no cache, no replay (bddmma's num_caches does not change the
//             result, so none is needed where every iteration's inputs fit);
//   reverse   last tracked iteration to first: the per-variable sums of the consumed differences | the reverse of the backward pass | the
//             per-variable sums of gS | gd — and the same for the forward pass; at the end the FULL = false sweep through T(lo, hi) and the
//             scalar omega's sum.  A wave per pack: fused-small packs are narrow packs, so a pack's reverse sweep is gi_down_body / gi_up_body
//             <NARROW> with tid = lane, T = 64, the wave's own gi_lds_bytes of the dynamic LDS (the area the forward used: the phases do not
//             overlap) and a wave-level ordering point as the barrier — packs of one member have different hop counts and must not meet at a
//             workgroup barrier inside a sweep;
//   exit      the results to the outputs, the entry state (saved by k_grad_small_load) back into the member.
// The elementwise phases run the bodies of k_gi_sums / k_gi_var_sums / k_gi_gd / k_gi_omega_sum in their orders (the variable -> layer table;
// 256 strided partial sums in double, then the tree — also where the workgroup has fewer than 256 threads), and nothing is accumulated
// atomically, so a member's results are those of its own bddmma_grad_learned_iterations wherever its fused forward is bit-equal to the
// four-launch one (include/bdd_mma.h).
#pragma once
#include "graditer.hpp"

namespace bddmma {

// A member's slab of the batch workspace, in values of REAL; ls / ss / vs: its layer, slot and variable counts rounded up to 4 (every
// array starts 16-byte aligned).  [0, gs_fixed_values): the entry state, the arguments, the reverse's scratch; behind it the records of
// SmallRecord for n tracked iterations.
__host__ __device__ inline uint64_t gs_fixed_values(uint32_t ls, uint32_t ss, uint32_t vs) { return 13ull * ls + 4ull * vs + 2ull * ss; }
__host__ __device__ inline uint64_t gs_slab_values(uint32_t ls, uint32_t ss, uint32_t vs, uint64_t n)
{
    return gs_fixed_values(ls, ss, vs) + (2 * n + 1) * (3ull * ls + ss);
}
template <typename REAL>
struct GradSmallSlab {
    REAL *e_lohi, *e_mm, *e_dlay;                      // the entry state: arc costs, deferred differences (binned entry order), delta per entry
    REAL *alpha, *g_lo, *g_hi, *g_mm, *g_alpha, *g_omega, *gS, *S, *gSv, *gT, *gF;
    SmallRecord<REAL> rec;
};
template <typename REAL>
__host__ __device__ inline GradSmallSlab<REAL> gs_slab(REAL* ws, uint32_t ls, uint32_t ss, uint32_t vs)
{
    GradSmallSlab<REAL> s;
    REAL* p = ws;
    auto take = [&](uint64_t k) { REAL* r = p; p += k; return r; };
    s.e_lohi = take(2ull * ls); s.e_mm = take(ls); s.e_dlay = take(2ull * ls);
    s.alpha = take(ls); s.g_lo = take(ls); s.g_hi = take(ls); s.g_mm = take(ls); s.g_alpha = take(ls); s.g_omega = take(ls);
    s.gS = take(2ull * ls); s.S = take(2ull * vs); s.gSv = take(2ull * vs); s.gT = take(ss); s.gF = take(ss);
    s.rec = SmallRecord<REAL>{p, ls, ss};
    return s;
}

struct GsWaveBar {   // the pack is one wave's: its LDS traffic in order, no workgroup barrier inside a sweep
    static __device__ __forceinline__ void sync() { wave_sync(); }
};
template <typename REAL>
struct GradSmallItem {
    SmallLearnItem<REAL> fw;             // the member's item of k_learned_small_batch
    const uint32_t *par_ptr, *par;       // the narrow words' parent tables (SolverT::sm_prepare)
    const int32_t* var;                  // variable of a layer
    const uint32_t *var_ptr, *var_layers;
    const uint32_t* lpos;                // layer -> binned entry
    REAL *alpha_ent, *omega_lay;         // where the forward reads its weights and omega_vec
    REAL* ws;                            // the member's slab
    uint32_t ww;                         // slots of a narrow pack
    uint32_t L, N, V, ls, ss, vs;
    uint32_t src, member;                // first value of the member in the concatenated arrays; its index in the caller's order
};
// The concatenated arrays of one call (device addresses)
template <typename REAL>
struct GradSmallIO {
    const REAL *w, *ov, *in_lo, *in_hi, *in_mm;
    REAL *lo, *hi, *mm, *gw, *gom;
};

// The arguments of one call in one launch, workgroup b those of member b: checked in the per-member call's order (bad[0..4]: the smallest
// member index with an offending omega_vec / weight / grad_lo / grad_hi / grad_mm; the caller presets them to 0xFFFFFFFF) and moved where
// the kernel reads them; g_alpha and g_omega zeroed; the member's entry state saved.  Reads the members, writes none of their state.
template <typename REAL>
__global__ void __launch_bounds__(256) k_grad_small_load(const GradSmallItem<REAL>* __restrict__ items, GradSmallIO<REAL> io, uint32_t* __restrict__ bad)
{
    const GradSmallItem<REAL>& it = items[blockIdx.x];
    const GradSmallSlab<REAL> s = gs_slab(it.ws, it.ls, it.ss, it.vs);
    const REAL inf = REAL(__builtin_huge_val());
    uint32_t b = 0;
    for (uint32_t l = threadIdx.x; l < it.L; l += blockDim.x) {
        const size_t g = (size_t)it.src + l;
        if (io.ov != nullptr) {
            const REAL o = io.ov[g];
            b |= !(o >= REAL(0) && o < inf) ? 1u : 0u;   // NaN fails both tests
            it.omega_lay[l] = o;
        }
        const REAL a = io.w[g];
        b |= !(a >= REAL(0) && a < inf) ? 2u : 0u;
        s.alpha[l] = a;
        it.alpha_ent[it.lpos[l]] = a;
        const REAL x0 = io.in_lo[g], x1 = io.in_hi[g], x2 = io.in_mm[g];
        b |= !(x0 > -inf && x0 < inf) ? 4u : 0u;
        b |= !(x1 > -inf && x1 < inf) ? 8u : 0u;
        b |= !(x2 > -inf && x2 < inf) ? 16u : 0u;
        s.g_lo[l] = x0;
        s.g_hi[l] = x1;
        s.g_mm[l] = x2;
        s.g_alpha[l] = REAL(0);
        s.g_omega[l] = REAL(0);
        s.e_mm[l] = it.fw.d.mm_binned[l];
    }
    for (uint32_t i = threadIdx.x; i < 2 * it.L; i += blockDim.x) {
        s.e_lohi[i] = it.fw.d.lohi[i];
        s.e_dlay[i] = it.fw.d.delta_lay[i];
    }
    for (uint32_t k = 0; k < 5; ++k)
        if (b & (1u << k)) atomicMin(bad + k, it.member);
}

// One member's whole call in its workgroup: shared by k_grad_small_batch (one n for the launch) and k_grad_small_counts_batch (the member's own).
// (`item` by pointer and dereferenced below the thread indices, where the kernel used to do it: the form that moves k_grad_small_batch's
// instruction streams least — profiles/batch_grad_counts_isa.txt.)
template <typename REAL, int NW, bool RL>
__device__ __forceinline__ void grad_small_body(const GradSmallItem<REAL>* __restrict__ item, REAL omega, uint32_t n, uint32_t use_ov, const GradSmallIO<REAL>& io)
{
    constexpr uint32_t NT = 64 * NW;
    extern __shared__ __attribute__((aligned(16))) unsigned char dyn_lds[];
    const uint32_t tid = threadIdx.x;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6)), lane = tid & 63u;

    // ---- forward over the tracked iterations, once, recording
    const GradSmallItem<REAL>& it = *item;
    {
        const SmallRecord<REAL> rec{it.ws + gs_fixed_values(it.ls, it.ss, it.vs), it.ls, it.ss};
        SmallLearn<REAL> ln = it.fw.ln;
        if (!use_ov) ln.omega_lay = nullptr;
        small_iterate<REAL, NW, RL, true, true>(it.fw.sm, it.fw.d, it.fw.pk, omega, n, RunStep{}, &ln, &rec);
    }
    __syncthreads();   // the records are written, the forward's LDS is dead
    const uint32_t L = it.L, N = it.N, V = it.V, ww = it.ww;
    const GradSmallSlab<REAL> s = gs_slab(it.ws, it.ls, it.ss, it.vs);
    const DevPtrs<REAL>& d = it.fw.d;
    const PackDev& pk = it.fw.pk;

    // ---- reverse
    const bool has_pack = wave < pk.n_packs;
    PullPack<REAL> pc{};
    if (has_pack) {
        const uint32_t q0 = pk.pack_hop_ptr[wave];
        pc = PullPack<REAL>{reinterpret_cast<REAL*>(dyn_lds + (size_t)wave * gi_lds_bytes(sizeof(REAL), ww)), q0, pk.pack_hop_ptr[wave + 1],
                            pk.pack_word_off[wave] - pk.hop_node_off[q0], ww, lane, 64u};
    }
    auto zero = [&](REAL* p) {
        for (uint32_t j = tid; j < N; j += NT) p[j] = REAL(0);
    };
    auto sums = [&](const REAL* dl) {
        for (uint32_t v = tid; v < V; v += NT) gi_sums_at(dl, it.var_ptr, it.var_layers, s.S, v);
    };
    auto var_sums = [&]() {
        for (uint32_t v = tid; v < V; v += NT) gi_var_sums_at((const REAL*)s.gS, it.var_ptr, it.var_layers, s.gSv, v);
    };
    auto gd = [&](const REAL* dl) {
        for (uint32_t l = tid; l < L; l += NT) gi_gd_at(dl, (const REAL*)s.gSv, it.var, s.g_mm, l);
    };
    GiArgs<REAL> a{};
    a.S = s.S; a.var = it.var; a.alpha = s.alpha; a.omega_lay = use_ov ? it.omega_lay : nullptr; a.omega = omega;
    a.g_lo = s.g_lo; a.g_hi = s.g_hi; a.g_mm = s.g_mm; a.gS = s.gS; a.g_alpha = s.g_alpha; a.g_omega = s.g_omega;
    zero(s.gT);
    for (uint32_t itr = n; itr-- > 0;) {
        const REAL *c0 = s.rec.c(itr), *post = s.rec.c(itr + 1), *c1 = s.rec.c1(itr);
        const REAL *d0 = s.rec.dm(itr), *mm2 = s.rec.dm(itr + 1), *mm1 = s.rec.mm1(itr);
        const REAL *T0 = s.rec.T(itr), *T2 = s.rec.T(itr + 1), *F = s.rec.F(itr);
        // the reverse of the backward pass: F of the forward pass, T of the new costs
        sums(mm1);
        zero(s.gF);
        __syncthreads();
        a.F = F; a.T = T2; a.pre = c1; a.post = post; a.mm = mm2; a.g_in = s.gT; a.g_out = s.gF;
        if (has_pack) gi_down_body<REAL, true, true, GsWaveBar, true>(d, pk, pc, it.par_ptr, it.par, ww, a);
        __syncthreads();
        var_sums();
        __syncthreads();
        gd(mm1);
        // the reverse of the forward pass: the same F, the T it read
        sums(d0);
        zero(s.gT);
        __syncthreads();
        a.T = T0; a.pre = c0; a.post = c1; a.mm = mm1; a.g_in = s.gF; a.g_out = s.gT;
        if (has_pack) gi_up_body<REAL, true, GsWaveBar, true>(d, pk, pc, it.par_ptr, it.par, ww, a);
        __syncthreads();
        var_sums();
        __syncthreads();
        gd(d0);
        __syncthreads();
    }
    __syncthreads();   // (n == 0 is the host's case; this orders zero(gT) all the same)
    // what is left of gT goes through T(lo, hi) of the first tracked iteration's input
    a.T = s.rec.T(0); a.post = s.rec.c(0); a.g_in = s.gT; a.g_out = nullptr;
    if (has_pack) gi_down_body<REAL, true, false, GsWaveBar, true>(d, pk, pc, it.par_ptr, it.par, ww, a);
    __syncthreads();

    // ---- exit: the results, the scalar omega's sum (k_gi_omega_sum's 256 partial sums and tree), the entry state
    for (uint32_t l = tid; l < L; l += NT) {
        const size_t g = (size_t)it.src + l;
        io.lo[g] = s.g_lo[l];
        io.hi[g] = s.g_hi[l];
        io.mm[g] = s.g_mm[l];
        io.gw[g] = s.g_alpha[l];
        if (use_ov) io.gom[g] = s.g_omega[l];
        d.mm_binned[l] = s.e_mm[l];
    }
    for (uint32_t i = tid; i < 2 * L; i += NT) {
        d.lohi[i] = s.e_lohi[i];
        const_cast<REAL*>(d.delta_lay)[i] = s.e_dlay[i];
    }
    if (!use_ov) {
        double* const sh = reinterpret_cast<double*>(dyn_lds);
        for (uint32_t t = tid; t < 256u; t += NT) {
            double acc = 0.0;
            for (uint32_t i = t; i < L; i += 256u) acc += (double)s.g_omega[i];
            sh[t] = acc;
        }
        __syncthreads();
        for (uint32_t k = 128; k > 0; k >>= 1) {
            for (uint32_t t = tid; t < k; t += NT) sh[t] += sh[t + k];
            __syncthreads();
        }
        if (tid == 0) io.gom[it.member] = (REAL)sh[0];
    }
}
template <typename REAL, int NW, bool RL>
__global__ void __launch_bounds__(64 * NW) k_grad_small_batch(const GradSmallItem<REAL>* __restrict__ items, REAL omega, uint32_t n, uint32_t use_ov, GradSmallIO<REAL> io)
{
    grad_small_body<REAL, NW, RL>(items + blockIdx.x, omega, n, use_ov, io);
}

// bddmma_grad_learned_iterations_counts_batch (BatchT::grad_learned_iterations_counts): every member with its own two counts, uint32 arrays on
// the device in the caller's member order, read by scalar loads at a uniform address.
//
// The untracked iterations in front: member i runs min(chunk, after[i] - first) learned iterations where after[i] > first — launched over
// first = 0, chunk, 2 chunk, .. up to the largest after[i]; two launches of a and b iterations leave what one of a + b leaves.  A member that
// is through (or whose tracked count is 0: the host gives it after[i] = 0) returns at its first instruction: a learned launch of 0
// iterations would still run the exit exchange and the epilogue.  Same items, groups and dynamic LDS as the kernels above.
template <typename REAL, int NW, bool RL>
__global__ void __launch_bounds__(64 * NW) k_grad_small_untracked_batch(const GradSmallItem<REAL>* __restrict__ items, REAL omega, uint32_t use_ov, uint32_t first,
                                                                        uint32_t chunk, const uint32_t* __restrict__ after)
{
    const GradSmallItem<REAL>& it = items[blockIdx.x];
    const uint32_t a = after[it.member];
    if (a <= first) return;
    const uint32_t left = a - first;
    SmallLearn<REAL> ln = it.fw.ln;
    if (!use_ov) ln.omega_lay = nullptr;
    small_iterate<REAL, NW, RL, true>(it.fw.sm, it.fw.d, it.fw.pk, omega, left < chunk ? left : chunk, RunStep{}, &ln);
}
// The call itself: k_grad_small_batch's body with n = tracked[member].  A member whose count is 0 is the per-member call with n == 0: its
// in-out arrays pass through (a copy onto themselves with device arrays, into the staging buffer's output half with host arrays), both
// outputs are zero, and nothing of the member is written — k_grad_small_load has only read it, so there is nothing to put back.
// The call's arrays come from memory (`iop`, behind the counts in the buffer the host copies once per call), not as twenty words of kernel
// arguments that are live from the first instruction.  The empty asm hides from the optimiser that n is not 0 behind the test: knowing it,
// it reshapes the body's loops and takes 7 to 9 VGPRs more than k_grad_small_batch (the 16-wave streaming form: 76 bytes of scratch for 36).
template <typename REAL, int NW, bool RL>
__global__ void __launch_bounds__(64 * NW) k_grad_small_counts_batch(const GradSmallItem<REAL>* __restrict__ items, REAL omega, uint32_t use_ov, const GradSmallIO<REAL>* __restrict__ iop,
                                                                     const uint32_t* __restrict__ tracked)
{
    const GradSmallIO<REAL>& io = *iop;
    const GradSmallItem<REAL>& it = items[blockIdx.x];
    const uint32_t n = tracked[it.member];
    if (n == 0) {
        for (uint32_t l = threadIdx.x; l < it.L; l += 64 * NW) {
            const size_t g = (size_t)it.src + l;
            io.lo[g] = io.in_lo[g];
            io.hi[g] = io.in_hi[g];
            io.mm[g] = io.in_mm[g];
            io.gw[g] = REAL(0);
            if (use_ov) io.gom[g] = REAL(0);
        }
        if (!use_ov && threadIdx.x == 0) io.gom[it.member] = REAL(0);
        return;
    }
    uint32_t n_body = n;
    asm volatile("" : "+s"(n_body));
    grad_small_body<REAL, NW, RL>(&it, omega, n_body, use_ov, io);
}

}  // namespace bddmma
