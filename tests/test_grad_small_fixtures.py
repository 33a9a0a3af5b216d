"""CPU tests that pin the yardstick of tests/test_gpu_grad_small.py, with the restatement alone: on every exact fixture of
tests/grad_small_fixtures.py float32 gives longdouble's bits on the five outputs of grad_iterations and on the end state, every value
stays within 2^20 grid steps, at least a fifth of the deciding minima are exact ties and both signs of mm occur — so the seeds recorded
there are a checked fact.  Each case prints its figures (pytest -s).  And, without a GPU as well: the new entry point is declared,
exported and bound alike, and the Python and C++ classes carry the call."""
import ctypes as C
import inspect
import os

import pytest

from bdd_amd import capi
from bdd_amd.solver import bdd_hip_batch, bdd_hip_parallel_mma
from exact_fixtures import HEADROOM
from grad_small_fixtures import EXACT_LONG, EXACT_SEEDS, MIN_TIE_SHARE, MIXED, SHAPES, fixture_figures, instance, meets_conditions, pack_hops
from test_capi_symbols import declared_symbols
from test_small_learned_abi import _header_arguments

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "bddmma_grad_learned_iterations_batch"


def _check(name, seed, omega_vec, untracked, tracked):
    f = fixture_figures(name, seed, omega_vec, untracked, tracked)
    print(f"{name} seed {seed} {'omega_vec' if omega_vec else 'omega'} {untracked}+{tracked}: grid {f['q']:g}, headroom {f['headroom']:g} of {HEADROOM:g}, "
          f"scalar omega's sum {f['omega_sum']:g} grid steps; exact ties {f['ties']} of {f['decided']} deciding minima ({f['ties'] / max(f['decided'], 1):.1%}); "
          f"tracked mm > 0 in {f['pos']}, < 0 in {f['neg']}")
    assert f["exact"], "float32 and longdouble differ"
    assert f["headroom"] <= HEADROOM and f["omega_sum"] <= 2.0 ** 24
    assert f["decided"] > 0 and f["ties"] >= MIN_TIE_SHARE * f["decided"]
    assert f["pos"] > 0 and f["neg"] > 0
    assert meets_conditions(f)
    return f


@pytest.mark.parametrize("omega_vec", [False, True], ids=["omega", "omega_vec"])
@pytest.mark.parametrize("name", [n for n, _, _ in SHAPES])
def test_exact_fixture(name, omega_vec):
    seed = EXACT_SEEDS[name][omega_vec]
    _check(name, seed, omega_vec, 1, 2)
    for earlier in range(1, seed):   # the recorded seed is the first that meets the conditions
        assert not meets_conditions(fixture_figures(name, earlier, omega_vec)), earlier


@pytest.mark.parametrize("name", sorted(EXACT_LONG))
def test_exact_fixture_of_five_tracked_iterations(name):
    _check(name, EXACT_LONG[name], False, 2, 5)


def test_every_shape_has_seeds_and_the_mixed_cover_has_packs_of_two_lengths():
    assert set(EXACT_SEEDS) == {n for n, _, _ in SHAPES}
    hops = pack_hops(instance(MIXED)[0])
    assert sorted(set(hops)) == [3, 9] and hops.count(3) >= 2 and hops.count(9) >= 2, hops


def test_entry_point_is_declared_exported_and_bound_alike():
    assert NAME in declared_symbols()
    args = _header_arguments(NAME)
    assert len(args) == 13 and args[0] == "bddmma_batch* b" and args[-1] == "int on_device", args
    res, argtypes = capi.SIGNATURES[NAME]
    V, U = C.c_void_p, C.c_uint64
    assert res is C.c_int and argtypes == [V, V, V, C.c_double, V, V, V, V, V, U, U, U, C.c_int]
    f = getattr(capi.lib(), NAME)   # AttributeError: the built library does not export it
    assert f.restype is C.c_int and len(f.argtypes) == 13
    assert f(None, None, None, 0.5, None, None, None, None, None, 0, 1, 1, 0) == capi.ERR_INVALID_ARGUMENT   # a null handle, before any device call


def test_python_and_cpp_classes_carry_the_call():
    p = inspect.signature(bdd_hip_batch.grad_iterations).parameters
    assert list(p) == list(inspect.signature(bdd_hip_parallel_mma.grad_iterations).parameters)
    assert [p[k].default for k in ("omega", "track_grad_after_itr", "track_grad_for_num_itr", "num_caches", "omega_vec", "out")] == [0.5, 0, 1, 1, None, None]
    hpp = open(os.path.join(ROOT, "bdd_amd", "csrc", "bdd_hip_parallel_mma.hpp")).read()
    assert NAME + "(" in hpp
