"""The entry points of the fused learned iterations, checked without a GPU: bddmma_fused_small_learned and bddmma_learned_iterations_batch are
declared in include/bdd_mma.h, exported by the built library and bound in bdd_amd/capi.py with the header's argument counts, and the Python
classes carry the methods.  tests/test_gpu_small_learned.py has the numbers."""
import ctypes as C
import inspect
import os
import re

from bdd_amd import capi
from bdd_amd.solver import bdd_hip_batch, bdd_hip_parallel_mma
from test_capi_symbols import declared_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"bddmma_fused_small_learned": 1, "bddmma_learned_iterations_batch": 6}   # name -> arguments


def _header_arguments(name):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bdd_mma.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
    assert m, f"{name} is not declared in include/bdd_mma.h as a function returning int"
    return [a.strip() for a in m.group(1).split(",")]


def test_entry_points_are_declared_exported_and_bound_alike():
    lib = capi.lib()
    for name, n_args in NEW.items():
        assert name in declared_symbols()
        args = _header_arguments(name)
        assert len(args) == n_args, (name, args)
        res, argtypes = capi.SIGNATURES[name]
        assert res is C.c_int and len(argtypes) == n_args, (name, argtypes)
        f = getattr(lib, name)   # AttributeError: the built library does not export it
        assert f.restype is C.c_int and len(f.argtypes) == n_args
    assert _header_arguments("bddmma_fused_small_learned") == ["const bddmma_solver* s"]
    assert capi.SIGNATURES["bddmma_learned_iterations_batch"][1] == [C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_uint64, C.c_int]
    # null handles are refused before any device call
    assert lib.bddmma_fused_small_learned(None) == -1
    assert lib.bddmma_learned_iterations_batch(None, None, None, 0.5, 1, 0) == capi.ERR_INVALID_ARGUMENT


def test_python_classes_carry_the_methods():
    assert callable(bdd_hip_parallel_mma.fused_small_learned)
    p = inspect.signature(bdd_hip_batch.learned_iterations).parameters
    assert list(p) == ["self", "dist_weights", "num_itr", "omega", "omega_vec"]
    assert p["omega"].default == 0.5 and p["omega_vec"].default is None
    hpp = open(os.path.join(ROOT, "bdd_amd", "csrc", "bdd_hip_parallel_mma.hpp")).read()
    assert "bddmma_learned_iterations_batch(" in hpp
