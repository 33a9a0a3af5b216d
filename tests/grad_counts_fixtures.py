"""The exact fixtures of the batch backward with per-member counts (bddmma_grad_learned_iterations_counts_batch), for
tests/test_batch_grad_counts_abi.py (CPU) and tests/test_gpu_batch_grad_counts.py (GPU).

One row per shape of tests/grad_small_fixtures.py and form of omega: the member's own (untracked, tracked) counts and the first seed of
exact_fixtures.exact_iteration_inputs, from 1 on, for which the restatement alone meets grad_small_fixtures.meets_conditions with those
counts — float32 gives longdouble's bits, at most 2^20 grid steps of headroom, at least a fifth of the deciding minima exact ties, both
signs of mm.  The counts differ from member to member in both kinds, and every kind has a 0 in front of tracked iterations.
tests/test_batch_grad_counts_abi.py asserts each row on the CPU.  Test helper only."""
from grad_small_fixtures import MIXED

# name -> ((untracked, tracked, seed) with a scalar omega, (untracked, tracked, seed) with omega_vec)
COUNT_ROWS = {
    "assign3": ((0, 3, 1), (3, 1, 3)),
    "assign8": ((3, 1, 3), (2, 2, 2)),
    "assign9": ((4, 2, 1), (2, 2, 1)),
    "cover40x60": ((0, 1, 1), (0, 3, 1)),
    "cover67x100": ((3, 1, 1), (2, 1, 1)),
    "cover147x220": ((1, 2, 1), (0, 2, 1)),
    "cover200x300": ((0, 3, 1), (1, 1, 1)),   # float only
    MIXED: ((3, 1, 1), (1, 2, 4)),
}
# the member that tracks nothing: a second handle of this shape with these counts, left untouched by the call
IDLE = ("assign8", 5, 0)


def row(name, omega_vec):
    """(untracked, tracked, seed)"""
    return COUNT_ROWS[name][1 if omega_vec else 0]
