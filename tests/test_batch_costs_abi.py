"""The entry points of a batch's cost transfer, checked without a GPU: bddmma_set_solver_costs_batch, bddmma_get_solver_costs_batch,
bddmma_stream_wait_batch and bddmma_stream_signal_batch are declared in include/bdd_mma.h, exported by the built library and bound in
bdd_amd/capi.py with the header's argument counts, the Python and C++ classes carry the methods, and a null batch is refused before
any device call.  tests/test_gpu_batch_costs.py has the numbers."""
import ctypes as C
import inspect
import os
import re

from bdd_amd import capi
from bdd_amd.solver import bdd_hip_batch
from test_capi_symbols import declared_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"bddmma_set_solver_costs_batch": 5, "bddmma_get_solver_costs_batch": 5, "bddmma_stream_wait_batch": 2,
       "bddmma_stream_signal_batch": 2}   # name -> arguments


def _header_arguments(name):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bdd_mma.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
    assert m, f"{name} is not declared in include/bdd_mma.h as a function returning int"
    return [" ".join(a.split()) for a in m.group(1).split(",")]


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
    assert _header_arguments("bddmma_set_solver_costs_batch") == ["bddmma_batch* b", "const void* lo", "const void* hi", "const void* mm", "int on_device"]
    assert _header_arguments("bddmma_get_solver_costs_batch") == ["bddmma_batch* b", "void* lo", "void* hi", "void* mm", "int on_device"]
    for name in ("bddmma_stream_wait_batch", "bddmma_stream_signal_batch"):
        assert _header_arguments(name) == ["bddmma_batch* b", "void* hip_stream"]
        assert capi.SIGNATURES[name][1] == [C.c_void_p, C.c_void_p]
    for name in ("bddmma_set_solver_costs_batch", "bddmma_get_solver_costs_batch"):
        assert capi.SIGNATURES[name][1] == [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]


def test_a_null_batch_is_refused_before_any_device_call():
    lib = capi.lib()
    buf = (C.c_double * 4)()
    for on_device in (0, 1):
        assert lib.bddmma_set_solver_costs_batch(None, buf, buf, buf, on_device) == capi.ERR_INVALID_ARGUMENT
        assert lib.bddmma_get_solver_costs_batch(None, buf, buf, buf, on_device) == capi.ERR_INVALID_ARGUMENT
    assert lib.bddmma_set_solver_costs_batch(None, None, None, None, 0) == capi.ERR_INVALID_ARGUMENT
    assert lib.bddmma_stream_wait_batch(None, None) == capi.ERR_INVALID_ARGUMENT
    assert lib.bddmma_stream_signal_batch(None, None) == capi.ERR_INVALID_ARGUMENT


def test_python_and_cpp_classes_carry_the_methods():
    p = inspect.signature(bdd_hip_batch.set_solver_costs).parameters
    assert list(p) == ["self", "lo", "hi", "mm"]
    p = inspect.signature(bdd_hip_batch.get_solver_costs).parameters
    assert list(p) == ["self", "out"] and p["out"].default is None
    for name in ("stream_wait", "stream_signal"):
        p = inspect.signature(getattr(bdd_hip_batch, name)).parameters
        assert list(p) == ["self", "hip_stream"] and p["hip_stream"].default == 0
    hpp = open(os.path.join(ROOT, "bdd_amd", "csrc", "bdd_hip_parallel_mma.hpp")).read()
    batch_class = hpp[hpp.index("class bdd_hip_batch {"):]
    batch_class = batch_class[:batch_class.index("\n};")]
    for name in NEW:
        assert name + "(b_" in batch_class, name
    for member in ("void set_solver_costs(", "get_solver_costs(", "void stream_wait(", "void stream_signal("):
        assert member in batch_class, member
