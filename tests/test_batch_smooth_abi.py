"""The entry points of a batch's sum-marginals, smooth solutions and smooth bound gradient, checked without a GPU:
bddmma_sum_marginals_batch, bddmma_smooth_solution_batch and bddmma_grad_smooth_lower_bound_per_bdd_batch are declared in
include/bdd_mma.h with exactly their argument lists, exported by the built library and bound in bdd_amd/capi.py alike, the Python and C++
classes carry the methods, a null batch is refused before any device call, and the LDS a launch asks for (kernels/batchsm.hpp) is what
the design states and fits the chip.  tests/test_gpu_batch_smooth.py has the numbers."""
import ctypes as C
import inspect
import os
import re

from bdd_amd import capi
from bdd_amd.solver import bdd_hip_batch, bdd_hip_parallel_mma
from test_batch_costs_abi import _header_arguments
from test_capi_symbols import declared_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bdd_amd", "csrc")
_V, _I = C.c_void_p, C.c_int
NEW = {"bddmma_sum_marginals_batch": (["bddmma_batch* b", "int log_probs", "void* sm0", "void* sm1", "int on_device"], [_V, _I, _V, _V, _I]),
       "bddmma_smooth_solution_batch": (["bddmma_batch* b", "void* out", "int on_device"], [_V, _V, _I]),
       "bddmma_grad_smooth_lower_bound_per_bdd_batch": (["bddmma_batch* b", "const void* grad_lb_per_bdd", "void* grad_lo_out", "void* grad_hi_out", "int on_device"],
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
        for log_probs in (0, 1):
            assert lib.bddmma_sum_marginals_batch(None, log_probs, buf, buf, on_device) == capi.ERR_INVALID_ARGUMENT
            assert lib.bddmma_sum_marginals_batch(None, log_probs, None, None, on_device) == capi.ERR_INVALID_ARGUMENT
        assert lib.bddmma_smooth_solution_batch(None, buf, on_device) == capi.ERR_INVALID_ARGUMENT
        assert lib.bddmma_smooth_solution_batch(None, None, on_device) == capi.ERR_INVALID_ARGUMENT
        assert lib.bddmma_grad_smooth_lower_bound_per_bdd_batch(None, buf, buf, buf, on_device) == capi.ERR_INVALID_ARGUMENT
        assert lib.bddmma_grad_smooth_lower_bound_per_bdd_batch(None, None, None, None, on_device) == capi.ERR_INVALID_ARGUMENT


def test_python_and_cpp_classes_carry_the_methods():
    """names and out= conventions are the member class's; the batch's sum_marginals_cuda has no get_sorted (unsorted only, no var output)"""
    for name, params in (("sum_marginals_cuda", ["self", "get_log_probs", "out"]), ("smooth_solution_per_bdd", ["self", "out"]),
                         ("grad_smooth_lower_bound_per_bdd", ["self", "grad_lb", "out"])):
        p = inspect.signature(getattr(bdd_hip_batch, name)).parameters
        assert list(p) == params and p["out"].default is None, name
        assert hasattr(bdd_hip_parallel_mma, name), name
    assert list(inspect.signature(bdd_hip_parallel_mma.sum_marginals_cuda).parameters) == ["self", "get_sorted", "get_log_probs", "out"]
    hpp = open(os.path.join(CSRC, "bdd_hip_parallel_mma.hpp")).read()
    batch_class = hpp[hpp.index("class bdd_hip_batch {"):]
    batch_class = batch_class[:batch_class.index("\n};")]
    for name in NEW:
        assert name + "(b_" in batch_class, name
    for member in ("void sum_marginals_cuda(", "void smooth_solution_per_bdd(", "void grad_smooth_lower_bound_per_bdd("):
        assert member in batch_class, member


def _return_expression(path, function):
    """the expression a one-line `inline ... function(...) { return EXPR; }` of a header returns"""
    text = open(path).read()
    m = re.search(r"inline \w+ " + function + r"\(([^)]*)\)\s*\{\s*return (.*?);\s*\}", text)
    assert m, function
    return [a.split()[-1] for a in m.group(1).split(",")], m.group(2)


def _evaluate(expr, **values):
    """a C integer expression of + * & ~ and casts, in Python (32-bit ~)"""
    expr = re.sub(r"\((?:size_t|uint32_t)\)", "", expr)
    expr = re.sub(r"(\d+)u\b", r"\1", expr)
    expr = re.sub(r"~(\d+)", lambda m: str(0xFFFFFFFF ^ int(m.group(1))), expr)
    assert re.fullmatch(r"[\w\s+*&(),]+", expr), expr
    return eval(expr, {"__builtins__": {}}, values)


def test_a_launch_asks_for_the_lds_the_design_states_and_it_fits_the_chip():
    """a pack's region is sm_lds_bytes(real size, 64 slots) rounded up to 16: 2 048 B in float, 3 840 B in double; the largest request,
    16 regions in double, is below the LDS per compute unit the layout code assumes for the chip (layout.hpp: ChipInfo)"""
    args, sm = _return_expression(os.path.join(CSRC, "kernels", "summarg.hpp"), "sm_lds_bytes")
    assert args == ["real_size", "ww"]
    sm_lds_bytes = lambda real_size, ww: _evaluate(sm, real_size=real_size, ww=ww)
    args, region = _return_expression(os.path.join(CSRC, "kernels", "batchsm.hpp"), "bsm_region_bytes")
    assert args == ["real_size", "ww"]
    bsm_region_bytes = lambda real_size, ww: _evaluate(region, real_size=real_size, ww=ww, sm_lds_bytes=sm_lds_bytes)
    assert sm_lds_bytes(4, 64) == 2048 and sm_lds_bytes(8, 64) == 3840
    assert bsm_region_bytes(4, 64) == 2048 and bsm_region_bytes(8, 64) == 3840
    for real_size in (4, 8):
        for ww in (1, 3, 63, 64):
            r = bsm_region_bytes(real_size, ww)
            assert r % 16 == 0 and 0 <= r - sm_lds_bytes(real_size, ww) < 16
    m = re.search(r"uint32_t lds_bytes = (\d+) \* 1024;", open(os.path.join(CSRC, "layout.hpp")).read())
    assert m, "layout.hpp: ChipInfo::lds_bytes"
    lds_cu = int(m.group(1)) * 1024
    assert lds_cu == 160 * 1024
    assert 16 * bsm_region_bytes(8, 64) == 61440 < 64 * 1024 < lds_cu
