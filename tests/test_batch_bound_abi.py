"""bddmma_lower_bound_batch (include/bdd_mma.h) is declared, exported and bound, and the farm's fuse_small front ends exist: the key two
configs must share (bdd_solver_py.fuse_key) and solve_batch's keywords — CPU only, no compute."""
import ctypes as C
import copy
import json
import os
import re

import pytest

from bdd_amd import bdd_solver_py, capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LP = "Minimize\nx1 + x2\nSubject To\nx1 + x2 >= 1\nBounds\nBinaries\nx1\nx2\nEnd\n"
TC_DEFAULTS = {"maximum iterations": 1000, "minimum improvement": 1e-6, "improvement slope": 1e-9, "time limit": 3600}
PR_DEFAULTS = {"initial perturbation": 0.1, "perturbation growth rate": 1.1, "inner iterations": 100, "outer iterations": 100, "seed": 0}
LBFGS_NAMES = ("lbfgs cuda mma", "cuda lbfgs parallel mma", "lbfgs hip mma", "hip lbfgs parallel mma")


def test_the_entry_point_is_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "bdd_mma.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bint\s+bddmma_lower_bound_batch\s*\(\s*bddmma_batch\s*\*\s*\w+\s*,\s*double\s*\*\s*\w+\s*,\s*int\s+\w+\s*\)\s*;", text)
    L = capi.lib()
    assert hasattr(L, "bddmma_lower_bound_batch")
    restype, argtypes = capi.SIGNATURES["bddmma_lower_bound_batch"]
    assert restype is C.c_int and list(argtypes) == [C.c_void_p, C.POINTER(C.c_double), C.c_int]
    assert L.bddmma_lower_bound_batch.argtypes == argtypes


def test_null_arguments_are_invalid_without_a_device():
    L = capi.lib()
    assert L.bddmma_lower_bound_batch(None, None, 0) == capi.ERR_INVALID_ARGUMENT
    out = (C.c_double * 1)(7.0)
    assert L.bddmma_lower_bound_batch(None, out, 0) == capi.ERR_INVALID_ARGUMENT
    assert L.bddmma_lower_bound_batch(None, out, 1) == capi.ERR_INVALID_ARGUMENT
    assert out[0] == 7.0


def test_python_and_cpp_classes_take_a_device_array():
    import inspect
    from bdd_amd.solver import bdd_hip_batch
    assert list(inspect.signature(bdd_hip_batch.lower_bounds).parameters) == ["self", "out"]
    assert inspect.signature(bdd_hip_batch.lower_bounds).parameters["out"].default is None
    hpp = open(os.path.join(ROOT, "bdd_amd", "csrc", "bdd_hip_parallel_mma.hpp")).read()
    assert "bddmma_lower_bound_batch(b_, " in hpp


def base(rounding=False, **kw):
    c = {"input": LP, "precision": "double", "relaxation solver": "cuda parallel mma"}
    if rounding:
        c["perturbation rounding"] = {}
    c.update(kw)
    return c


def key(c):
    return bdd_solver_py.fuse_key(json.dumps(c))


def test_fuse_key_ignores_the_input_and_the_device():
    a = base()
    assert key(a) != ""
    assert key(a) == key(dict(a, input=LP.replace("x1 + x2 >= 1", "x1 + x2 >= 2"))) == key(dict(a, device=3))
    assert key(a) == bdd_solver_py.fuse_key(a)                       # a dict, as the bdd_solver constructor takes one
    assert key(base(**{"relaxation solver": "hip parallel mma"})) == key(a)
    assert key({"input": LP}) == key(a)                              # precision and solver name at their defaults


def test_fuse_key_tells_the_precisions_apart():
    assert key(base(precision="float")) != key(base(precision="double"))
    assert key(base(precision="float")) == key(base(precision="single"))


@pytest.mark.parametrize("name", list(TC_DEFAULTS))
def test_fuse_key_holds_each_termination_criterion(name):
    default = TC_DEFAULTS[name]
    assert key(base()) == key(base(**{"termination criteria": {}})) == key(base(**{"termination criteria": {name: default}}))
    assert key(base(**{"termination criteria": {name: default * 2}})) != key(base())
    full = dict(TC_DEFAULTS)
    other = copy.deepcopy(full)
    other[name] = default * 2
    assert key(base(**{"termination criteria": full})) == key(base())
    assert key(base(**{"termination criteria": other})) != key(base(**{"termination criteria": full}))


def test_fuse_key_holds_whether_rounding_is_asked_for():
    assert key(base(rounding=True)) != key(base())
    assert key(base(rounding=True)) == key(base(**{"perturbation rounding": dict(PR_DEFAULTS)}))


@pytest.mark.parametrize("name", list(PR_DEFAULTS))
def test_fuse_key_holds_each_rounding_value(name):
    default = PR_DEFAULTS[name]
    assert key(base(**{"perturbation rounding": {name: default}})) == key(base(rounding=True))
    assert key(base(**{"perturbation rounding": {name: default * 2 + 1}})) != key(base(rounding=True))


@pytest.mark.parametrize("name", LBFGS_NAMES)
def test_fuse_key_is_empty_for_an_lbfgs_solver(name):
    assert key(base(**{"relaxation solver": name})) == ""
    assert key(base(rounding=True, **{"relaxation solver": name})) == ""


def test_solve_batch_accepts_the_new_keywords():
    assert bdd_solver_py.solve_batch([], devices=[0], quiet=True, fuse_small=True, max_group=4) == []
    assert bdd_solver_py.solve_batch(configs=[], fuse_small=False) == []
    doc = bdd_solver_py.solve_batch.__doc__
    for kw in ("configs", "devices", "quiet", "fuse_small", "max_group"):
        assert kw in doc, kw
    with pytest.raises(RuntimeError, match="max_group"):
        bdd_solver_py.solve_batch([], fuse_small=True, max_group=0)
