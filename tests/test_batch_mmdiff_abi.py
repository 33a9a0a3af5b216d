"""The entry points of a batch's min-marginal differences and their gradient, checked without a GPU: bddmma_min_marginal_diff_batch and
bddmma_grad_min_marginal_diff_batch are declared in include/bdd_mma.h with exactly their argument lists, exported by the built library and
bound in bdd_amd/capi.py alike, the Python and C++ classes carry the methods, and a null batch is refused before any device call.
tests/test_gpu_batch_mmdiff.py has the numbers."""
import ctypes as C
import inspect
import os

from bdd_amd import capi
from bdd_amd.solver import bdd_hip_batch, bdd_hip_parallel_mma
from test_batch_costs_abi import _header_arguments
from test_capi_symbols import declared_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_V, _I = C.c_void_p, C.c_int
NEW = {"bddmma_min_marginal_diff_batch": (["bddmma_batch* b", "void* out", "int on_device"], [_V, _V, _I]),
       "bddmma_grad_min_marginal_diff_batch": (["bddmma_batch* b", "const void* grad_mm", "void* grad_lo_out", "void* grad_hi_out", "int on_device"],
                                               [_V, _V, _V, _V, _I])}


def test_entry_points_are_declared_exported_and_bound_alike():
    lib = capi.lib()
    for name, (args, argtypes) in NEW.items():
        assert name in declared_symbols()
        assert _header_arguments(name) == args
        res, bound = capi.SIGNATURES[name]
        assert res is C.c_int and bound == argtypes, (name, bound)
        f = getattr(lib, name)   # AttributeError: the built library does not export it
        assert f.restype is C.c_int and list(f.argtypes) == argtypes


def test_a_null_batch_is_refused_before_any_device_call():
    lib = capi.lib()
    buf = (C.c_double * 4)()
    for on_device in (0, 1):
        assert lib.bddmma_min_marginal_diff_batch(None, buf, on_device) == capi.ERR_INVALID_ARGUMENT
        assert lib.bddmma_min_marginal_diff_batch(None, None, on_device) == capi.ERR_INVALID_ARGUMENT
        assert lib.bddmma_grad_min_marginal_diff_batch(None, buf, buf, buf, on_device) == capi.ERR_INVALID_ARGUMENT
        assert lib.bddmma_grad_min_marginal_diff_batch(None, None, None, None, on_device) == capi.ERR_INVALID_ARGUMENT


def test_python_and_cpp_classes_carry_the_methods():
    """names and out= conventions are the member class's"""
    for name, params in (("min_marginal_diff", ["self", "out"]), ("grad_all_min_marginal_differences", ["self", "grad_mm", "out"])):
        p = inspect.signature(getattr(bdd_hip_batch, name)).parameters
        assert list(p) == params and p["out"].default is None, name
        assert list(inspect.signature(getattr(bdd_hip_parallel_mma, name)).parameters) == params, name
    hpp = open(os.path.join(ROOT, "bdd_amd", "csrc", "bdd_hip_parallel_mma.hpp")).read()
    batch_class = hpp[hpp.index("class bdd_hip_batch {"):]
    batch_class = batch_class[:batch_class.index("\n};")]
    for name in NEW:
        assert name + "(b_" in batch_class, name
    for member in ("void min_marginal_diff(", "void grad_mm_diff_all_hops("):
        assert member in batch_class, member
