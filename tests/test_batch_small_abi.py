"""The batch entry points (include/bdd_mma.h: bddmma_batch_*) are declared, exported and bound, and refuse bad member lists before
touching a device — CPU only, no compute."""
import ctypes as C
import os
import re

from bdd_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCH = ["bddmma_batch_create", "bddmma_batch_destroy", "bddmma_batch_iterations", "bddmma_batch_last_error", "bddmma_batch_lower_bounds",
         "bddmma_batch_run_solver", "bddmma_batch_size", "bddmma_batch_time_iterations"]


def test_batch_symbols_are_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "bdd_mma.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = sorted(set(re.findall(r"\b(bddmma_batch_[a-z0-9_]+)\s*\(", text)))
    assert declared == BATCH
    L = capi.lib()
    for s in BATCH:
        assert hasattr(L, s), f"{s} declared in include/bdd_mma.h but not exported"
        assert s in capi.SIGNATURES, f"{s} has no ctypes signature in bdd_amd/capi.py"


def test_python_and_cpp_classes_exist():
    import bdd_amd
    from bdd_amd.solver import bdd_hip_batch
    assert bdd_amd.bdd_hip_batch is bdd_hip_batch
    for name in ("iterations", "run_solver", "lower_bounds"):
        assert callable(getattr(bdd_hip_batch, name))
    hpp = open(os.path.join(ROOT, "bdd_amd", "csrc", "bdd_hip_parallel_mma.hpp")).read()
    assert "class bdd_hip_batch" in hpp


def test_null_and_empty_member_lists_are_invalid_arguments_without_a_device():
    L = capi.lib()
    h = C.c_void_p(0xDEAD)
    one = (C.c_void_p * 1)(None)
    assert L.bddmma_batch_create(None, one, 1) == capi.ERR_INVALID_ARGUMENT            # null output pointer
    assert L.bddmma_batch_create(C.byref(h), None, 1) == capi.ERR_INVALID_ARGUMENT      # null member array
    assert h.value is None                                                              # *out is cleared on failure
    assert b"null" in L.bddmma_batch_last_error(None)
    assert L.bddmma_batch_create(C.byref(h), one, 0) == capi.ERR_INVALID_ARGUMENT       # n == 0
    assert L.bddmma_batch_create(C.byref(h), one, 1) == capi.ERR_INVALID_ARGUMENT       # a null member
    assert b"member 0" in L.bddmma_batch_last_error(None)
    assert h.value is None


def test_null_batch_handles_are_rejected():
    L = capi.lib()
    assert L.bddmma_batch_size(None) == 0
    assert L.bddmma_batch_iterations(None, 0.5, 1) == capi.ERR_INVALID_ARGUMENT
    assert L.bddmma_batch_run_solver(None, 1, 0.0, 0.0, 1.0, None) == capi.ERR_INVALID_ARGUMENT
    assert L.bddmma_batch_lower_bounds(None, None) == capi.ERR_INVALID_ARGUMENT
    assert L.bddmma_batch_time_iterations(None, 0.5, 1, None) == capi.ERR_INVALID_ARGUMENT
    L.bddmma_batch_destroy(None)
    assert L.bddmma_batch_last_error(None) is not None
