"""CPU tests of bdd_amd/autograd.py and of the two stream-ordering entry points it rests on: what can be checked without a GPU — the
module is opt-in, its batch bookkeeping, its refusals (which come before any solver is touched), and that bddmma_stream_wait /
bddmma_stream_signal are declared alike in the header and in the ctypes binding.  tests/test_gpu_autograd.py has the numbers."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _fresh_python(code):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)


def test_importing_the_package_does_not_import_torch():
    r = _fresh_python("import sys, bdd_amd; assert 'torch' not in sys.modules, 'torch imported'; "
                      "assert 'bdd_amd.autograd' not in sys.modules; print('ok')")
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stderr


def test_the_module_imports_without_a_gpu_and_exports_the_reference_names():
    import bdd_amd.autograd as A
    import torch
    names = {"DualIterations", "DistributeDeferredDelta", "ComputeAllMinMarginalsDiff", "PerturbPrimalCosts", "ComputeLowerBoundperBDD",
             "ComputePerBDDSolutionsIdentityBackward", "ComputePerBDDSolutions", "GetSumMarginals", "GetMarginalProbability",
             "ComputePrimalSolution", "batch_index"}
    assert names <= set(A.__all__) and all(hasattr(A, n) for n in names)
    for n in ("DualIterations", "DistributeDeferredDelta", "ComputeAllMinMarginalsDiff", "PerturbPrimalCosts", "ComputeLowerBoundperBDD",
              "ComputePerBDDSolutionsIdentityBackward"):
        assert issubclass(getattr(A, n), torch.autograd.Function)


class StubSolver:
    """the sizes of a solver and a record of every other method called on it"""

    def __init__(self, layers, bdds, variables, value_type=np.float32, device=0):
        self.value_type = value_type
        self._sizes = (layers, bdds, variables, device)
        self.calls = []

    def nr_layers(self): return self._sizes[0]
    def nr_bdds(self): return self._sizes[1]
    def nr_variables(self): return self._sizes[2]
    def device(self): return self._sizes[3]
    def get_primal_variable_index(self): return (np.arange(self._sizes[0]) % self._sizes[2]).astype(np.int32)
    def get_bdd_index(self): return (np.arange(self._sizes[0]) % self._sizes[1]).astype(np.int32)

    def __getattr__(self, name):
        if name.startswith("_"):
            raise AttributeError(name)
        return lambda *a, **k: self.calls.append(name)


def _stubs(value_type=np.float32):
    return [StubSolver(7, 3, 4, value_type), StubSolver(5, 2, 5, value_type), StubSolver(11, 4, 6, value_type)]


def test_batch_index_offsets_on_stub_solvers():
    import torch
    from bdd_amd.autograd import batch_index
    st = _stubs()
    ix = batch_index(st)
    assert ix.layer_offsets == [0, 7, 12, 23] and ix.bdd_offsets == [0, 3, 5, 9] and ix.variable_offsets == [0, 4, 9, 15]
    assert ix.layer_variables.dtype == torch.int64 and ix.layer_bdds.dtype == torch.int64
    assert ix.layer_variables.shape == (23,) and ix.layer_bdds.shape == (23,)
    for i, s in enumerate(st):
        a, b = ix.layer_offsets[i], ix.layer_offsets[i + 1]
        np.testing.assert_array_equal(ix.layer_variables[a:b].numpy(), s.get_primal_variable_index() + ix.variable_offsets[i])
        np.testing.assert_array_equal(ix.layer_bdds[a:b].numpy(), s.get_bdd_index() + ix.bdd_offsets[i])
    assert all(not s.calls for s in st)
    one = batch_index(st[1:2])
    assert one.layer_offsets == [0, 5] and one.layer_bdds.tolist() == [0, 1, 0, 1, 0]


L, B, V = 23, 9, 15   # the batch sizes of _stubs()


def _entry_points():
    """name -> (the tensor arguments in order as (name, size, may hold one value instead), call(solvers, *tensors))"""
    import bdd_amd.autograd as A
    lo, hi, mm, w = ("lo_costs_batch", L, False), ("hi_costs_batch", L, False), ("def_mm_batch", L, False), ("dist_weights_batch", L, False)
    return {
        "DualIterations": ([lo, hi, mm, w, ("omega", L, True)], lambda s, a, b, c, d, e: A.DualIterations.apply(s, a, b, c, d, 3, e, 1, 0.0, 1, 0, 0.9)),
        "DistributeDeferredDelta": ([lo, hi, mm], lambda s, a, b, c: A.DistributeDeferredDelta.apply(s, a, b, c)),
        "ComputeAllMinMarginalsDiff": ([lo, hi], lambda s, a, b: A.ComputeAllMinMarginalsDiff.apply(s, a, b)),
        "PerturbPrimalCosts": ([("lo_costs_pert_batch", V, False), ("hi_costs_pert_batch", V, False), lo, hi],
                               lambda s, a, b, c, d: A.PerturbPrimalCosts.apply(s, a, b, c, d)),
        "ComputeLowerBoundperBDD": ([lo, hi], lambda s, a, b: A.ComputeLowerBoundperBDD.apply(s, a, b, 0.0)),
        "ComputePerBDDSolutionsIdentityBackward": ([lo, hi], lambda s, a, b: A.ComputePerBDDSolutionsIdentityBackward.apply(s, a, b, None)),
        "ComputePerBDDSolutions": ([lo, hi], lambda s, a, b: A.ComputePerBDDSolutions(s, a, b)),
        "GetSumMarginals": ([lo, hi], lambda s, a, b: A.GetSumMarginals(s, a, b, True)),
        "GetMarginalProbability": ([lo, hi], lambda s, a, b: A.GetMarginalProbability(s, a, b)),
        "ComputePrimalSolution": ([lo, hi, mm], lambda s, a, b, c: A.ComputePrimalSolution(s, a, b, c, 0.1, 1.1, 10)),
    }


@pytest.mark.parametrize("value_type", [np.float32, np.float64], ids=["float", "double"])
@pytest.mark.parametrize("entry", ["DualIterations", "DistributeDeferredDelta", "ComputeAllMinMarginalsDiff", "PerturbPrimalCosts", "ComputeLowerBoundperBDD",
                                   "ComputePerBDDSolutionsIdentityBackward", "ComputePerBDDSolutions", "GetSumMarginals", "GetMarginalProbability",
                                   "ComputePrimalSolution"])
def test_every_validation_names_its_argument_and_touches_no_solver(entry, value_type):
    import torch
    args, call = _entry_points()[entry]
    right = torch.float64 if value_type == np.float64 else torch.float32
    wrong = torch.float32 if value_type == np.float64 else torch.float64
    good = lambda: [torch.zeros(n, dtype=right, requires_grad=True) for _, n, _ in args]
    st = _stubs(value_type)
    tried = 0
    for k, (name, n, one_ok) in enumerate(args):
        bad = {
            "dtype": torch.zeros(n, dtype=wrong),
            "integer dtype": torch.zeros(n, dtype=torch.int64),
            "too long": torch.zeros(n + 1, dtype=right),
            "too short": torch.zeros(n - 1, dtype=right),
            "two-dimensional": torch.zeros(n, 1, dtype=right),
            "not contiguous": torch.zeros(2 * n, dtype=right)[::2],
            "not a tensor": np.zeros(n, value_type),
        }
        if not one_ok:
            bad["one value"] = torch.zeros(1, dtype=right)
        for what, t in bad.items():
            ts = good()
            ts[k] = t
            with pytest.raises(ValueError, match=r"^" + re.escape(name) + r" "):
                call(st, *ts)
            tried += 1
    # tensors of the right form that live on the host: the device check, which names the first of them
    with pytest.raises(ValueError, match=r"^" + re.escape(args[0][0]) + r" is on cpu"):
        call(st, *good())
    if any(one_ok for _, _, one_ok in args):   # one value is a valid form for omega: it gets as far as the device check too
        ts = good()
        ts[-1] = torch.zeros(1, dtype=right)
        with pytest.raises(ValueError, match=r" is on cpu"):
            call(st, *ts)
    assert tried >= 7 * len(args)
    assert all(not s.calls for s in st), [s.calls for s in st]


def test_solver_lists_no_batch_can_be_formed_from_are_refused():
    import torch
    import bdd_amd.autograd as A
    z = torch.zeros(12)
    with pytest.raises(ValueError, match="^solvers"):
        A.ComputeAllMinMarginalsDiff.apply([], z, z)
    mixed = [StubSolver(7, 3, 4, np.float32), StubSolver(5, 2, 5, np.float64)]
    with pytest.raises(ValueError, match="^solvers.*precision"):
        A.ComputeAllMinMarginalsDiff.apply(mixed, z, z)
    two = [StubSolver(7, 3, 4, device=0), StubSolver(5, 2, 5, device=1)]
    with pytest.raises(ValueError, match="^solvers.*device"):
        A.ComputeAllMinMarginalsDiff.apply(two, z, z)
    assert all(not s.calls for s in mixed + two)


def test_stream_entry_points_are_declared_alike_in_the_header_and_the_binding():
    from bdd_amd import capi
    from bdd_amd.solver import bdd_hip_parallel_mma
    from test_capi_symbols import declared_symbols
    text = open(os.path.join(ROOT, "include", "bdd_mma.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ("bddmma_stream_wait", "bddmma_stream_signal"):
        assert name in declared_symbols()
        m = re.search(r"\bint\s+" + name + r"\s*\(\s*bddmma_solver\s*\*\s*\w+\s*,\s*void\s*\*\s*\w+\s*\)\s*;", text)
        assert m, f"{name} is not declared as int {name}(bddmma_solver*, void*)"
        assert capi.SIGNATURES[name] == (C.c_int, [C.c_void_p, C.c_void_p])
        f = getattr(capi.lib(), name)
        assert f.restype is C.c_int and list(f.argtypes) == [C.c_void_p, C.c_void_p]
        assert f(None, None) == capi.ERR_INVALID_ARGUMENT   # a null handle is refused before any device call
    assert callable(bdd_hip_parallel_mma.stream_wait) and callable(bdd_hip_parallel_mma.stream_signal)
    hpp = open(os.path.join(ROOT, "bdd_amd", "csrc", "bdd_hip_parallel_mma.hpp")).read()
    assert "void stream_wait(void* hip_stream)" in hpp and "void stream_signal(void* hip_stream)" in hpp
