// C++ test of the gradient members of the drop-in class bdd_hip_parallel_mma<REAL> (grad_mm_diff_all_hops, grad_lower_bound_per_bdd,
// grad_distribute_delta, grad_cost_perturbation) on a small protocol instance: a three-variable simplex plus one knapsack row.  The expected
// values come from the NumPy restatement tests/grad_restatement.py (itself pinned to enumeration); the costs are tie-free (smallest decision
// gap 0.25), so they are exact sums of the incoming gradient's values.  Needs a GPU; run by tests/test_gpu_gradients_cpp.py.
#include <cmath>
#include <hip/hip_runtime_api.h>

#include <cstdio>
#include <string>
#include <vector>

#include "../../bdd_amd/csrc/bdd_hip_parallel_mma.hpp"
#include "../../bdd_amd/csrc/host/bdd_store.hpp"

using namespace LPMP;
using bddmma_host::bdd_store;

static int failures = 0;
#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) { std::printf("  FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } \
    } while (0)
#define CHECK_NEAR(a, b, tol)                                                                              \
    do {                                                                                                   \
        const double a_ = (a), b_ = (b);                                                                   \
        if (!(std::fabs(a_ - b_) <= (tol))) { std::printf("  FAILED %s:%d: %s = %.12g, expected %.12g\n", __FILE__, __LINE__, #a, a_, b_); ++failures; } \
    } while (0)

// x_0 + x_1 + x_2 = 1 and 2 x_0 + 3 x_1 + 4 x_2 + x_3 <= 5, costs 1.5, -2, 0.75, -1.25 (split evenly over a variable's BDDs).
// Incoming gradient of the min-marginal differences: g = -0.5 (v + 1) in the simplex, (v + 1) in the knapsack row.
// [knapsack?][variable] = {grad_lo, grad_hi}, then the arg-min path x
static const double WANT[2][4][2] = {{{0.5, -0.5}, {-1.0, 1.0}, {0.5, -0.5}, {0, 0}}, {{-1.0, 1.0}, {2.0, -2.0}, {-3.0, 3.0}, {-4.0, 4.0}}};
static const double WANT_X[2][4] = {{0, 1, 0, 0}, {0, 1, 0, 1}};

template <typename REAL>
static void test_class()
{
    bdd_store col;
    col.add_simplex({0, 1, 2});
    CHECK(col.add_linear({2, 3, 4, 1}, bddmma_host::ineq_t::le, 5, {0, 1, 2, 3}) == bddmma_host::row_status::ok);
    const std::vector<double> c{1.5, -2, 0.75, -1.25};
    bdd_hip_parallel_mma<REAL> s(col, c);
    const size_t L = s.nr_layers(), V = s.nr_variables(), B = s.nr_bdds();
    CHECK(L == 7 && V == 4 && B == 2);
    const auto var = s.get_primal_variable_index();
    const auto bdd = s.get_bdd_index();
    int knap_bdd = -1;
    for (size_t l = 0; l < L; ++l)
        if (var[l] == 3) knap_bdd = bdd[l];
    CHECK(knap_bdd >= 0);
    std::vector<int> knap(L);
    std::vector<REAL> g(L);
    for (size_t l = 0; l < L; ++l) {
        knap[l] = bdd[l] == knap_bdd;
        g[l] = REAL(knap[l] ? var[l] + 1 : -0.5 * (var[l] + 1));
    }
    const double lb = s.lower_bound();
    CHECK_NEAR(lb, -3.25, 1e-6);

    // the backward of the min-marginal differences: host vectors, then device buffers bit for bit
    const auto gr = s.grad_mm_diff_all_hops(g);
    for (size_t l = 0; l < L; ++l) {
        CHECK_NEAR(gr.first[l], WANT[knap[l]][var[l]][0], 0.0);
        CHECK_NEAR(gr.second[l], WANT[knap[l]][var[l]][1], 0.0);
    }
    REAL *dg = nullptr, *dlo = nullptr, *dhi = nullptr, *dglb = nullptr, *dv0 = nullptr, *dv1 = nullptr;
    CHECK(hipMalloc((void**)&dg, L * sizeof(REAL)) == hipSuccess && hipMalloc((void**)&dlo, L * sizeof(REAL)) == hipSuccess &&
          hipMalloc((void**)&dhi, L * sizeof(REAL)) == hipSuccess && hipMalloc((void**)&dglb, B * sizeof(REAL)) == hipSuccess &&
          hipMalloc((void**)&dv0, V * sizeof(REAL)) == hipSuccess && hipMalloc((void**)&dv1, V * sizeof(REAL)) == hipSuccess);
    CHECK(hipMemcpy(dg, g.data(), L * sizeof(REAL), hipMemcpyHostToDevice) == hipSuccess);
    s.grad_mm_diff_all_hops(dg, dlo, dhi);
    std::vector<REAL> hlo(L), hhi(L);
    CHECK(hipMemcpy(hlo.data(), dlo, L * sizeof(REAL), hipMemcpyDeviceToHost) == hipSuccess && hipMemcpy(hhi.data(), dhi, L * sizeof(REAL), hipMemcpyDeviceToHost) == hipSuccess);
    for (size_t l = 0; l < L; ++l) CHECK(hlo[l] == gr.first[l] && hhi[l] == gr.second[l]);
    CHECK_NEAR(s.lower_bound(), lb, 0.0);

    // the per-BDD lower bound: x glb / (1 - x) glb with the arg-min paths; the smooth one sums to glb per layer as well
    std::vector<REAL> glb(B);
    for (size_t b = 0; b < B; ++b) glb[b] = REAL((int)b == knap_bdd ? -3 : 2);
    const auto gl = s.grad_lower_bound_per_bdd(glb);
    const auto gs = s.grad_lower_bound_per_bdd(glb, true);
    for (size_t l = 0; l < L; ++l) {
        const double w = knap[l] ? -3 : 2, x = WANT_X[knap[l]][var[l]];
        CHECK_NEAR(gl.second[l], x * w, 0.0);
        CHECK_NEAR(gl.first[l], (1 - x) * w, 0.0);
        CHECK_NEAR(gs.first[l] + gs.second[l], w, sizeof(REAL) == 4 ? 1e-6 : 1e-14);
        CHECK(gs.second[l] / w > 0 && gs.second[l] / w < 1);
    }
    CHECK(hipMemcpy(dglb, glb.data(), B * sizeof(REAL), hipMemcpyHostToDevice) == hipSuccess);
    s.grad_lower_bound_per_bdd(dglb, dlo, dhi);
    CHECK(hipMemcpy(hlo.data(), dlo, L * sizeof(REAL), hipMemcpyDeviceToHost) == hipSuccess && hipMemcpy(hhi.data(), dhi, L * sizeof(REAL), hipMemcpyDeviceToHost) == hipSuccess);
    for (size_t l = 0; l < L; ++l) CHECK(hlo[l] == gl.first[l] && hhi[l] == gl.second[l]);

    // the cost perturbation: the mean over a variable's layers
    const auto gp = s.grad_cost_perturbation(gr.first, gr.second);
    for (size_t v = 0; v < V; ++v) {
        const double n = v < 3 ? 2 : 1;
        CHECK_NEAR(gp.first[v], (WANT[0][v][0] + WANT[1][v][0]) / n, 0.0);
        CHECK_NEAR(gp.second[v], (WANT[0][v][1] + WANT[1][v][1]) / n, 0.0);
    }
    CHECK(hipMemcpy(dlo, gr.first.data(), L * sizeof(REAL), hipMemcpyHostToDevice) == hipSuccess && hipMemcpy(dhi, gr.second.data(), L * sizeof(REAL), hipMemcpyHostToDevice) == hipSuccess);
    s.grad_cost_perturbation(dlo, dhi, dv0, dv1);
    std::vector<REAL> hv0(V), hv1(V);
    CHECK(hipMemcpy(hv0.data(), dv0, V * sizeof(REAL), hipMemcpyDeviceToHost) == hipSuccess && hipMemcpy(hv1.data(), dv1, V * sizeof(REAL), hipMemcpyDeviceToHost) == hipSuccess);
    for (size_t v = 0; v < V; ++v) CHECK(hv0[v] == gp.first[v] && hv1[v] == gp.second[v]);

    // distribute_delta: refused before the first distribute_delta(); afterwards by the sign of the deferred differences it applied
    bool threw = false;
    try {
        (void)s.grad_distribute_delta(gr.first, gr.second);
    } catch (const std::exception&) {
        threw = true;
    }
    CHECK(threw);
    auto costs = s.get_solver_costs();
    for (size_t l = 0; l < L; ++l) std::get<2>(costs)[l] = REAL(l % 2 ? 0.5 : -0.25);
    s.set_solver_costs(costs);
    s.distribute_delta();
    const auto gd = s.grad_distribute_delta(gr.first, gr.second);
    for (size_t l = 0; l < L; ++l) CHECK_NEAR(gd[l], l % 2 ? gr.second[l] : -gr.first[l], 0.0);
    s.grad_distribute_delta(dlo, dhi, dg);
    CHECK(hipMemcpy(hlo.data(), dg, L * sizeof(REAL), hipMemcpyDeviceToHost) == hipSuccess);
    for (size_t l = 0; l < L; ++l) CHECK(hlo[l] == gd[l]);
    (void)hipFree(dg); (void)hipFree(dlo); (void)hipFree(dhi); (void)hipFree(dglb); (void)hipFree(dv0); (void)hipFree(dv1);
}

int main()
{
    struct { const char* name; void (*fn)(); } tests[] = {{"class<float>", test_class<float>}, {"class<double>", test_class<double>}};
    for (auto& t : tests) {
        const int before = failures;
        try {
            t.fn();
        } catch (const std::exception& e) {
            std::printf("  EXCEPTION: %s\n", e.what());
            ++failures;
        }
        std::printf("[%s] %s\n", failures == before ? " OK " : "FAIL", t.name);
    }
    std::printf("%d failure(s)\n", failures);
    return failures ? 1 : 0;
}
