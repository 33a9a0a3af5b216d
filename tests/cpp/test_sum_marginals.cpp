// C++ test of the sum-marginal members of the drop-in class bdd_hip_parallel_mma<REAL> (sum_marginals_cuda, sum_marginals,
// smooth_solution_cuda) and of bdd_solver::sum_marginals, on the two-simplex problem of the reference's own test
// (test/test_bdd_cuda_sum_marginals.cpp): closed forms at its 1e-5.  Needs a GPU; run by tests/test_gpu_sum_marginals.py.
#include <cmath>
#include <hip/hip_runtime_api.h>

#include <cstdio>
#include <string>
#include <vector>

#include "../../bdd_amd/csrc/bdd_hip_parallel_mma.hpp"
#include "../../bdd_amd/csrc/host/bdd_solver.hpp"
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

// (lo, hi) probabilities of variables 0..5: x_1 + x_2 + x_3 = 2 with costs 2, 3, 4 and x_4 + x_5 + x_6 = 1 with costs 1, 2, -1
static const double WANT[6][2] = {
    {std::exp(-7.0), std::exp(-5.0) + std::exp(-6.0)}, {std::exp(-6.0), std::exp(-5.0) + std::exp(-7.0)}, {std::exp(-5.0), std::exp(-6.0) + std::exp(-7.0)},
    {std::exp(-2.0) + std::exp(1.0), std::exp(-1.0)},  {std::exp(-1.0) + std::exp(1.0), std::exp(-2.0)},  {std::exp(-1.0) + std::exp(-2.0), std::exp(1.0)}};

template <typename REAL>
static void test_class()
{
    bdd_store col;
    CHECK(col.add_linear({1, 1, 1}, bddmma_host::ineq_t::eq, 2, {0, 1, 2}) == bddmma_host::row_status::ok);
    col.add_simplex({3, 4, 5});
    const std::vector<double> c{2, 3, 4, 1, 2, -1};
    bdd_hip_parallel_mma<REAL> s(col, c);
    const double lb = s.lower_bound();
    for (int logp = 0; logp < 2; ++logp) {
        const auto sm = s.sum_marginals(logp != 0);
        CHECK(sm.size() == 6);
        for (size_t v = 0; v < 6 && v < sm.size(); ++v) {
            CHECK(sm[v].size() == 1);
            CHECK_NEAR(logp ? std::exp(sm[v][0][0]) : sm[v][0][0], WANT[v][0], 1e-5);
            CHECK_NEAR(logp ? std::exp(sm[v][0][1]) : sm[v][0][1], WANT[v][1], 1e-5);
        }
    }
    // device buffers against host vectors, bit for bit; the smooth solution against the formula of the logs
    const size_t L = s.nr_layers();
    CHECK(L == 6);
    const auto host = s.sum_marginals_cuda(false, true);
    int32_t* dv = nullptr;
    REAL *d0 = nullptr, *d1 = nullptr, *ds = nullptr;
    CHECK(hipMalloc((void**)&dv, L * sizeof(int32_t)) == hipSuccess && hipMalloc((void**)&d0, L * sizeof(REAL)) == hipSuccess &&
          hipMalloc((void**)&d1, L * sizeof(REAL)) == hipSuccess && hipMalloc((void**)&ds, L * sizeof(REAL)) == hipSuccess);
    s.sum_marginals_cuda(dv, d0, d1, false, true);
    s.smooth_solution_cuda(ds);
    std::vector<int32_t> hv(L);
    std::vector<REAL> h0(L), h1(L), hs(L);
    CHECK(hipMemcpy(hv.data(), dv, L * sizeof(int32_t), hipMemcpyDeviceToHost) == hipSuccess && hipMemcpy(h0.data(), d0, L * sizeof(REAL), hipMemcpyDeviceToHost) == hipSuccess &&
          hipMemcpy(h1.data(), d1, L * sizeof(REAL), hipMemcpyDeviceToHost) == hipSuccess && hipMemcpy(hs.data(), ds, L * sizeof(REAL), hipMemcpyDeviceToHost) == hipSuccess);
    const auto sm_host = s.smooth_solution();
    for (size_t l = 0; l < L; ++l) {
        CHECK(hv[l] == std::get<0>(host)[l] && h0[l] == std::get<1>(host)[l] && h1[l] == std::get<2>(host)[l] && hs[l] == sm_host[l]);
        const double a = h0[l], b = h1[l], m = std::max(a, b);
        CHECK_NEAR(hs[l], std::exp(b - m) / (std::exp(a - m) + std::exp(b - m)), sizeof(REAL) == 4 ? 1e-6 : 1e-14);
        CHECK_NEAR(hs[l], WANT[hv[l]][1] / (WANT[hv[l]][0] + WANT[hv[l]][1]), 1e-5);
    }
    (void)hipFree(dv); (void)hipFree(d0); (void)hipFree(d1); (void)hipFree(ds);
    CHECK_NEAR(s.lower_bound(), lb, 0.0);   // state contract: the bound is recomputed from untouched costs
}

static void test_driver()
{
    const std::string lp = "Minimize\\n2 x_1 + 3 x_2 + 4 x_3\\n+1 x_4 + 2 x_5 - 1 x_6\\nSubject To\\nx_1 + x_2 + x_3 = 2\\nx_4 + x_5 + x_6 = 1\\nEnd\\n";
    bddmma_host::bdd_solver s("{\"input\": \"" + lp + "\", \"relaxation solver\": \"cuda parallel mma\", \"precision\": \"double\", "
                              "\"termination criteria\": {\"maximum iterations\": 0, \"improvement slope\": 0.0, \"minimum improvement\": 0.0}}", true);
    s.solve();
    const auto sm = s.sum_marginals(false);
    CHECK(sm.size() == 6);
    // after 0 iterations the costs are the objective's: the same closed forms
    for (size_t v = 0; v < 6 && v < sm.size(); ++v) {
        CHECK(sm[v].size() == 1);
        CHECK_NEAR(sm[v][0][0], WANT[v][0], 1e-5);
        CHECK_NEAR(sm[v][0][1], WANT[v][1], 1e-5);
    }
}

int main()
{
    struct { const char* name; void (*fn)(); } tests[] = {{"class<float>", test_class<float>}, {"class<double>", test_class<double>}, {"driver", test_driver}};
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
