// solver_bt_f32.hip — BatchT<float> (solver_bt.hpp) and the batch kernels it launches, as one translation unit.
#include "solver_bt.hpp"

namespace bddmma {
int make_batch_f32(BatchBase** out, SolverBase* const* members, uint64_t n, std::string& err)
{
    std::unique_ptr<BatchT<float>> b(new BatchT<float>());
    const int rc = b->init(members, n);
    if (rc) err = b->err;
    else *out = b.release();
    return rc;
}
}  // namespace bddmma
