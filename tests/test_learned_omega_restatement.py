"""CPU tests of learned iterations with one omega per layer: the NumPy restatement (tests/learned_omega_restatement.py) with a constant
omega vector is the scalar restatement exactly, and the C-ABI entry bddmma_learned_iterations_omega_vec and the Python argument omega_vec
exist.  The GPU side: tests/test_gpu_learned_omega_vec.py."""
import inspect

import numpy as np
import pytest

from bdd_amd import capi
from bdd_amd.solver import bdd_hip_parallel_mma
from learned_mma_restatement import LearnedMma
from learned_omega_restatement import LearnedOmegaMma
from test_capi_symbols import declared_symbols
from util import GOLDEN, load_golden


def _pair(name, precision):
    _, z = load_golden(name)
    out = []
    for cls in (LearnedMma, LearnedOmegaMma):
        m = cls(z["instr"], z["delims"], precision)
        m.update_costs_hi(np.asarray(z["costs"], np.float64))
        out.append(m)
    return out


@pytest.mark.parametrize("name", GOLDEN)
@pytest.mark.parametrize("precision", ["double", "float"])
def test_constant_omega_vector_is_the_scalar_restatement(name, precision):
    a, b = _pair(name, precision)
    rng = np.random.Generator(np.random.PCG64(5))
    alpha = rng.uniform(0.0, 0.8, a.n_layers).astype(a.dt)
    for omega in (0.5, 0.3):
        vec = np.full(b.n_layers, omega, b.dt)
        ran_a = a.iterations(alpha, 4, omega, improvement_slope=0.0)
        ran_b = b.iterations(alpha, 4, vec, improvement_slope=0.0)
        assert ran_a == ran_b == 4
        for x, y in ((a.lo, b.lo), (a.hi, b.hi), (a.mm, b.mm), (a.T, b.T)):
            np.testing.assert_array_equal(x, y)
        assert a.lower_bound() == b.lower_bound()


@pytest.mark.parametrize("precision", ["double", "float"])
def test_omega_vector_is_per_layer(precision):
    """a zero omega on one layer leaves that layer's deferred difference at 0 and is not the scalar run"""
    a, b = _pair("matching_3x3_first_row", precision)
    vec = np.full(b.n_layers, 0.5, b.dt)
    vec[::2] = 0
    alpha = a.isotropic_alpha()
    a.learned_iteration(alpha, 0.5)
    b.learned_iteration(alpha, vec)
    assert np.all(b.mm[::2] == 0)
    assert not np.array_equal(a.mm, b.mm)


def test_omega_vec_entry_point_is_declared_exported_and_bound():
    assert "bddmma_learned_iterations_omega_vec" in declared_symbols()
    assert "bddmma_learned_iterations_omega_vec" in capi.SIGNATURES
    restype, argtypes = capi.SIGNATURES["bddmma_learned_iterations_omega_vec"]
    assert len(argtypes) == 14
    assert hasattr(capi.lib(), "bddmma_learned_iterations_omega_vec")


def test_learned_iterations_accepts_omega_vec():
    p = inspect.signature(bdd_hip_parallel_mma.learned_iterations).parameters
    assert "omega_vec" in p and p["omega_vec"].default is None
    assert list(p)[-1] == "omega_vec"
