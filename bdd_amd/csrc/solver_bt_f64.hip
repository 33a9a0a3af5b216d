// solver_bt_f64.hip — BatchT<double> (solver_bt.hpp) and the batch kernels it launches, as one translation unit.
#include "solver_bt.hpp"

namespace bddmma {
int make_batch_f64(BatchBase** out, SolverBase* const* members, uint64_t n, std::string& err)
{
    std::unique_ptr<BatchT<double>> b(new BatchT<double>());
    const int rc = b->init(members, n);
    if (rc) err = b->err;
    else *out = b.release();
    return rc;
}
}  // namespace bddmma
