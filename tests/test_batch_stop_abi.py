"""The entry points of a batch's learned iterations with the stopping rule (include/bdd_mma.h: bddmma_learned_iterations_stop_batch,
bddmma_fused_small_stop), checked without a GPU: through the header, the ctypes table, the built library, the Python classes and the C++
header.  tests/test_gpu_batch_stop.py runs them on the MI355X."""
import ctypes as C
import inspect
import os
import re

from bdd_amd import capi
from bdd_amd.solver import bdd_hip_batch, bdd_hip_parallel_mma

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_arguments(name):
    text = open(os.path.join(ROOT, "include", "bdd_mma.h")).read()
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", text, re.S)
    assert m, name
    args = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    return [" ".join(a.split()) for a in args.split(",")]


def test_header_ctypes_table_and_library_agree():
    lib = capi.lib()
    V, D, U, I = C.c_void_p, C.c_double, C.c_uint64, C.c_int
    assert _header_arguments("bddmma_fused_small_stop") == ["const bddmma_solver* s"]
    assert _header_arguments("bddmma_learned_iterations_stop_batch") == [
        "bddmma_batch* b", "const void* dist_weights", "const void* omega_vec", "double omega", "uint64_t num_itr", "double improvement_slope",
        "void* sol_avg", "void* lb_first_diff_avg", "void* lb_second_diff_avg", "uint64_t compute_history_for_itr", "double history_avg_beta",
        "int on_device", "uint64_t* iterations_done"]
    assert capi.SIGNATURES["bddmma_fused_small_stop"] == (I, [V])
    assert capi.SIGNATURES["bddmma_learned_iterations_stop_batch"] == (I, [V, V, V, D, U, D, V, V, V, U, D, I, V])
    # the call this one extends keeps its signature
    assert capi.SIGNATURES["bddmma_learned_iterations_history_batch"] == (I, [V, V, V, D, U, V, V, V, U, D, I])
    # null handles are refused before any device call
    assert lib.bddmma_fused_small_stop(None) == -1
    done = (C.c_uint64 * 1)(7)
    assert lib.bddmma_learned_iterations_stop_batch(None, None, None, 0.5, 1, 1e-3, None, None, None, 0, 0.9, 0, done) == capi.ERR_INVALID_ARGUMENT
    assert done[0] == 7


def test_python_classes_carry_the_stopping_form():
    assert callable(bdd_hip_parallel_mma.fused_small_stop)
    p = inspect.signature(bdd_hip_batch.learned_iterations_stopping).parameters
    assert list(p) == ["self", "dist_weights", "num_itr", "omega", "improvement_slope", "omega_vec", "compute_history_for_itr", "history_avg_beta", "sol_avg",
                       "lb_first_diff_avg", "lb_second_diff_avg"]
    # the defaults of the per-solver method it stands for
    q = inspect.signature(bdd_hip_parallel_mma.learned_iterations).parameters
    for name in ("omega", "improvement_slope", "compute_history_for_itr", "history_avg_beta"):
        assert p[name].default == q[name].default, name


def test_cpp_classes_carry_the_stopping_form():
    hpp = open(os.path.join(ROOT, "bdd_amd", "csrc", "bdd_hip_parallel_mma.hpp")).read()
    assert re.search(r"bool\s+fused_small_stop\(\)\s*const\s*\{\s*return\s+bddmma_fused_small_stop\(h_\)\s*==\s*1;", hpp)
    assert re.search(r"std::vector<size_t>\s+learned_iterations_stopping\(", hpp) and re.search(r"std::vector<size_t>\s+learned_iterations_stopping_dev\(", hpp)
    assert hpp.count("bddmma_learned_iterations_stop_batch(") >= 2
