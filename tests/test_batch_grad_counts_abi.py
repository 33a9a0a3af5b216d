"""The batch backward of the learned iterations with per-member counts (include/bdd_mma.h: bddmma_grad_learned_iterations_counts_batch),
checked without a GPU: the entry point through the header, the ctypes table, the built library, the Python classes and the C++ header;
and the rows of tests/grad_counts_fixtures.py as facts about the restatement — every row meets the conditions of
tests/grad_small_fixtures.py with its own counts, and no earlier seed does.  Each row prints its figures (pytest -s).
tests/test_gpu_batch_grad_counts.py runs the call on the MI355X."""
import ctypes as C
import inspect
import os
import re

import pytest

from bdd_amd import capi
from bdd_amd.solver import bdd_hip_batch
from exact_fixtures import HEADROOM
from grad_counts_fixtures import COUNT_ROWS, IDLE, row
from grad_small_fixtures import MIN_TIE_SHARE, SHAPES, fixture_figures, meets_conditions
from test_batch_stop_abi import _header_arguments
from test_capi_symbols import declared_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "bddmma_grad_learned_iterations_counts_batch"


def test_entry_point_is_declared_exported_and_bound_alike():
    assert NAME in declared_symbols()
    assert _header_arguments(NAME) == [
        "bddmma_batch* b", "const void* dist_weights", "const void* omega_vec", "double omega", "void* grad_lo", "void* grad_hi", "void* grad_mm",
        "void* grad_dist_weights_out", "void* grad_omega_out", "const uint64_t* track_grad_after_itr", "const uint64_t* track_grad_for_num_itr",
        "uint64_t num_caches", "int on_device"]
    # the call it extends: the same 13 arguments, the two counts by value
    old = _header_arguments("bddmma_grad_learned_iterations_batch")
    assert len(old) == 13 and old[9:11] == ["uint64_t track_grad_after_itr", "uint64_t track_grad_for_num_itr"]
    assert [a for k, a in enumerate(old) if k not in (9, 10)] == [a for k, a in enumerate(_header_arguments(NAME)) if k not in (9, 10)]
    res, argtypes = capi.SIGNATURES[NAME]
    V, U, P = C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)
    assert res is C.c_int and argtypes == [V, V, V, C.c_double, V, V, V, V, V, P, P, U, C.c_int]
    f = getattr(capi.lib(), NAME)   # AttributeError: the built library does not export it
    assert f.restype is C.c_int and len(f.argtypes) == 13
    counts = (C.c_uint64 * 1)(1)
    assert f(None, None, None, 0.5, None, None, None, None, None, counts, counts, 1, 0) == capi.ERR_INVALID_ARGUMENT   # a null handle, before any device call


def test_python_and_cpp_classes_carry_the_call():
    p = inspect.signature(bdd_hip_batch.grad_iterations_counts).parameters
    assert list(p) == ["self", "dist_weights", "grad_lo", "grad_hi", "grad_mm", "track_grad_after_itr", "track_grad_for_num_itr", "omega", "num_caches",
                       "omega_vec", "out"]
    q = inspect.signature(bdd_hip_batch.grad_iterations).parameters
    for name in ("omega", "num_caches", "omega_vec", "out"):
        assert p[name].default == q[name].default, name
    assert p["track_grad_after_itr"].default is inspect.Parameter.empty and p["track_grad_for_num_itr"].default is inspect.Parameter.empty
    hpp = open(os.path.join(ROOT, "bdd_amd", "csrc", "bdd_hip_parallel_mma.hpp")).read()
    assert re.search(r"void\s+grad_iterations_counts_dev\(", hpp) and NAME + "(" in hpp
    assert hpp.index("void grad_iterations_dev(") < hpp.index("void grad_iterations_counts_dev(")


def test_the_table_has_every_shape_and_counts_that_differ():
    assert set(COUNT_ROWS) == {n for n, _, _ in SHAPES}
    assert IDLE[0] in COUNT_ROWS and IDLE[1] > 0 and IDLE[2] == 0
    for omega_vec in (False, True):
        rows = [row(n, omega_vec) for n in COUNT_ROWS]
        assert len({r[0] for r in rows}) >= 3 and len({r[1] for r in rows}) >= 3, rows
        assert any(r[0] == 0 for r in rows) and all(r[1] > 0 for r in rows), rows


@pytest.mark.parametrize("omega_vec", [False, True], ids=["omega", "omega_vec"])
@pytest.mark.parametrize("name", [n for n, _, _ in SHAPES])
def test_row_is_the_first_seed_that_meets_the_conditions(name, omega_vec):
    untracked, tracked, seed = row(name, omega_vec)
    f = fixture_figures(name, seed, omega_vec, untracked, tracked)
    print(f"{name} seed {seed} {'omega_vec' if omega_vec else 'omega'} {untracked}+{tracked}: grid {f['q']:g}, headroom {f['headroom']:g} of {HEADROOM:g}, "
          f"scalar omega's sum {f['omega_sum']:g} grid steps; exact ties {f['ties']} of {f['decided']} deciding minima ({f['ties'] / max(f['decided'], 1):.1%}); "
          f"tracked mm > 0 in {f['pos']}, < 0 in {f['neg']}")
    assert f["exact"], "float32 and longdouble differ"
    assert f["headroom"] <= HEADROOM == 2.0 ** 20
    assert f["decided"] > 0 and f["ties"] >= MIN_TIE_SHARE * f["decided"] and MIN_TIE_SHARE == 0.20
    assert f["pos"] > 0 and f["neg"] > 0
    assert meets_conditions(f)
    for earlier in range(1, seed):
        assert not meets_conditions(fixture_figures(name, earlier, omega_vec, untracked, tracked)), earlier
