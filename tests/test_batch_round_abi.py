"""The entry points of a batch's primal rounding, checked without a GPU: bddmma_perturb_primal_costs_batch and
bddmma_incremental_mm_agreement_rounding_batch are declared in include/bdd_mma.h with exactly their argument lists, exported by the built
library and bound in bdd_amd/capi.py alike, the Python and C++ classes carry the methods, and a null batch is refused before any device
call.  tests/test_gpu_batch_round.py has the numbers."""
import ctypes as C
import inspect
import os

from bdd_amd import capi
from bdd_amd.solver import bdd_hip_batch, bdd_hip_parallel_mma
from test_batch_costs_abi import _header_arguments
from test_capi_symbols import declared_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bdd_amd", "csrc")
_V, _I, _D, _U32, _U64 = C.c_void_p, C.c_int, C.c_double, C.c_uint32, C.c_uint64
NEW = {"bddmma_perturb_primal_costs_batch": (["bddmma_batch* b", "double cur_delta", "uint32_t round_index", "uint32_t seed", "uint32_t* counts", "char* sol",
                                              "void* cost_delta_0", "void* cost_delta_1"], [_V, _D, _U32, _U32, C.POINTER(_U32), _V, _V, _V]),
       "bddmma_incremental_mm_agreement_rounding_batch": (["bddmma_batch* b", "double init_delta", "double delta_growth_rate", "uint64_t num_itr_lb",
                                                           "uint64_t num_rounds", "uint32_t seed", "char* sol", "int* found", "uint64_t* rounds"],
                                                          [_V, _D, _D, _U64, _U64, _U32, _V, C.POINTER(_I), C.POINTER(_U64)])}


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
    counts, sol, c = (C.c_uint32 * 8)(), (C.c_char * 8)(), (C.c_double * 8)()
    found, rounds = (C.c_int * 2)(), (C.c_uint64 * 2)()
    inv = capi.ERR_INVALID_ARGUMENT
    assert lib.bddmma_perturb_primal_costs_batch(None, 0.1, 0, 0, counts, sol, c, c) == inv
    assert lib.bddmma_perturb_primal_costs_batch(None, 0.1, 0, 0, counts, sol, None, None) == inv
    assert lib.bddmma_perturb_primal_costs_batch(None, 0.1, 0, 0, None, None, None, None) == inv
    assert lib.bddmma_incremental_mm_agreement_rounding_batch(None, 0.1, 1.2, 5, 2, 0, sol, found, rounds) == inv
    assert lib.bddmma_incremental_mm_agreement_rounding_batch(None, 0.1, 1.2, 5, 2, 0, sol, found, None) == inv
    assert lib.bddmma_incremental_mm_agreement_rounding_batch(None, -1.0, 0.0, 5, 2, 0, None, None, None) == inv
    assert list(counts) == [0] * 8 and list(found) == [0, 0] and list(rounds) == [0, 0]


def test_python_and_cpp_classes_carry_the_methods():
    """names and defaults are the member class's; the batch has no L-BFGS form and no verbose"""
    p = inspect.signature(bdd_hip_batch.perturb_primal_costs).parameters
    assert list(p) == ["self", "delta", "round_index", "seed"] and p["round_index"].default == 0 and p["seed"].default == 0
    p = inspect.signature(bdd_hip_batch.primal_rounding_incremental).parameters
    assert list(p)[:6] == ["self", "init_delta", "delta_growth_rate", "num_itr_lb", "num_rounds", "seed"]
    assert p["num_rounds"].default == 500 and p["seed"].default == 0 and "verbose" not in p
    q = inspect.signature(bdd_hip_parallel_mma.primal_rounding_incremental).parameters
    assert q["num_rounds"].default == 500 and q["seed"].default == 0
    hpp = open(os.path.join(CSRC, "bdd_hip_parallel_mma.hpp")).read()
    batch_class = hpp[hpp.index("class bdd_hip_batch {"):]
    batch_class = batch_class[:batch_class.index("\n};")]
    assert "bddmma_incremental_mm_agreement_rounding_batch(b_" in batch_class
    assert "std::vector<std::vector<char>> incremental_mm_agreement_rounding(" in batch_class
