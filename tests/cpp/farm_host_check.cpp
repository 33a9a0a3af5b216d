// farm_host_check.cpp — the farm's host-only parts under the host sanitizers, as a program of its own: fuse_key on config texts and
// solve_batch's queue / parking / error bookkeeping with configs that fail before any device call.  Needs no GPU.
//   hipcc -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined tests/cpp/farm_host_check.cpp \
//         bdd_amd/csrc/host/bdd_solver.cpp bdd_amd/csrc/host/bdd_store.cpp bdd_amd/csrc/host/ilp.cpp \
//         -Lbdd_amd/csrc -lbdd_mma_hip -Wl,-rpath,$PWD/bdd_amd/csrc -o farm_host_check && ./farm_host_check
#include <cstdio>
#include <string>
#include <vector>

#include "../../bdd_amd/csrc/host/bdd_solver.hpp"

static int failures = 0;
#define EXPECT(c)                                                    \
    do {                                                             \
        if (!(c)) {                                                  \
            std::printf("FAILED line %d: %s\n", __LINE__, #c);       \
            ++failures;                                              \
        }                                                            \
    } while (0)

int main()
{
    using bddmma_host::fuse_key;
    const std::string lp = "Minimize\\nx1 + x2\\nSubject To\\nx1 + x2 >= 1\\nBounds\\nBinaries\\nx1\\nx2\\nEnd\\n";
    const std::string a = "{\"input\": \"" + lp + "\"}";
    const std::string k = fuse_key(a);
    EXPECT(!k.empty());
    EXPECT(k == fuse_key("{\"input\": \"other\", \"device\": 5, \"precision\": \"double\", \"relaxation solver\": \"hip parallel mma\"}"));
    EXPECT(k == fuse_key("{\"input\": \"x\", \"termination criteria\": {\"maximum iterations\": 1000, \"minimum improvement\": 1e-6, \"improvement slope\": 1e-9, "
                         "\"time limit\": 3600}}"));
    EXPECT(k != fuse_key("{\"input\": \"x\", \"precision\": \"float\"}"));
    EXPECT(k != fuse_key("{\"input\": \"x\", \"termination criteria\": {\"time limit\": 10}}"));
    const std::string r = fuse_key("{\"input\": \"x\", \"perturbation rounding\": {}}");
    EXPECT(r != k && r.size() > k.size());
    EXPECT(r == fuse_key("{\"input\": \"x\", \"perturbation rounding\": {\"initial perturbation\": 0.1, \"perturbation growth rate\": 1.1, \"inner iterations\": 100, "
                         "\"outer iterations\": 100, \"seed\": 0}}"));
    EXPECT(r != fuse_key("{\"input\": \"x\", \"perturbation rounding\": {\"seed\": 4294967295}}"));
    EXPECT(r != fuse_key("{\"input\": \"x\", \"perturbation rounding\": {\"outer iterations\": 1e18}}"));
    for (const char* name : {"lbfgs cuda mma", "cuda lbfgs parallel mma", "lbfgs hip mma", "hip lbfgs parallel mma", "sequential mma", "no such solver"})
        EXPECT(fuse_key(std::string("{\"input\": \"x\", \"relaxation solver\": \"") + name + "\"}").empty());
    bool threw = false;
    try {
        (void)fuse_key("[1, 2]");
    } catch (const std::exception&) {
        threw = true;
    }
    EXPECT(threw);

    // the queue with fuse_small: every config fails in construct() (no input, an unknown order, a CPU solver, an infeasible row — or, on a
    // machine without a device, at bddmma_create), so nothing is parked and every key's flush sees an empty group
    std::vector<std::string> configs;
    for (int i = 0; i < 40; ++i) {
        configs.push_back("{\"precision\": \"double\"}");
        configs.push_back("{\"input\": \"" + lp + "\", \"variable order\": \"bfs\"}");
        configs.push_back("{\"input\": \"" + lp + "\", \"relaxation solver\": \"sequential mma\"}");
        configs.push_back("{\"input\": \"Minimize\\nx\\nSubject To\\nx >= 2\\nBounds\\nBinaries\\nx\\nEnd\\n\"}");
        configs.push_back("not json at all");
    }
    for (const std::vector<int>& devices : {std::vector<int>{0}, std::vector<int>{0, 0, 0}}) {
        for (uint32_t max_group : {1u, 2u, 256u}) {
            bddmma_host::batch_options opt;
            opt.fuse_small = true;
            opt.max_group = max_group;
            const auto res = bddmma_host::solve_batch(configs, devices, true, opt);
            EXPECT(res.size() == configs.size());
            for (size_t i = 0; i < res.size(); ++i) {
                EXPECT(res[i].config == configs[i]);
                EXPECT(!res[i].ok && !res[i].error.empty() && !res[i].fused && res[i].device == 0);
            }
        }
    }
    threw = false;
    try {
        bddmma_host::batch_options opt;
        opt.fuse_small = true;
        opt.max_group = 0;
        (void)bddmma_host::solve_batch(configs, {0}, true, opt);
    } catch (const std::exception&) {
        threw = true;
    }
    EXPECT(threw);
    std::printf(failures ? "farm_host_check: %d FAILED\n" : "farm_host_check: ok\n", failures);
    return failures ? 1 : 0;
}
