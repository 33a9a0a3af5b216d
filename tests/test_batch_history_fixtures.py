"""What tests/test_gpu_batch_history.py relies on, checked without a GPU: the decision margins of the cost seeds its double cases use
(tests/batch_history_fixtures.py), and the entry points of the history batch call (include/bdd_mma.h:
bddmma_learned_iterations_history_batch, bddmma_fused_small_history) through the header, the ctypes table, the built library and the classes."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from batch_history_fixtures import MARGIN, NUM_ITR, OMEGA, REJECTED, SEEDS, LearnedMma, decision_margins, major_inputs, member_keys
from bdd_amd import capi
from bdd_amd.solver import bdd_hip_batch, bdd_hip_parallel_mma
from test_gpu_small_learned import REF_TOL, SHAPES, instance

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COVERS = [(name, seed) for name, _, fused_in, _ in SHAPES if name.startswith("cover") and "double" in fused_in for seed in SEEDS[name]]


def test_the_member_table():
    assert MARGIN == REF_TOL["double"] == 1e-9
    assert set(SEEDS) == {name for name, *_ in SHAPES}
    assert all(min(s) >= 1 and list(s) == sorted(s) for s in SEEDS.values())
    # seeds are taken from 1 upwards: one that is skipped is listed as rejected, with its reason
    for name, seeds in SEEDS.items():
        skipped = set(range(1, max(seeds))) - set(seeds)
        assert skipped == set(REJECTED.get(name, {})), (name, skipped)
    assert len(member_keys("float", SHAPES)) == 12 and len(member_keys("double", SHAPES)) == 10
    assert [k[0] for k in member_keys("double", SHAPES)[:5]] == ["assign3", "assign8", "cover40x60", "cover67x100", "cover147x220"]


@pytest.mark.parametrize("name,seed", COVERS)
def test_every_tracked_decision_of_the_double_cases_has_a_margin(name, seed):
    """the smallest |hi_path - lo_path| over the on-path nodes, in each of the ten iterations the GPU cases track (a history of 10 tracks
    all of them), with the scalar omega and with omega_vec: at least 1e-9 times the larger of 1 and the largest cost magnitude"""
    col, costs = instance(name, seed)
    layer_var = LearnedMma(col.instr, col.delims, "double").layer_var
    w, ov = major_inputs(layer_var, name, seed, np.float64)
    for label, omega in (("omega", OMEGA), ("omega_vec", ov)):
        for itr, (margin, scale) in enumerate(decision_margins(col, costs, w, omega, NUM_ITR)):
            assert margin >= MARGIN * max(1.0, scale), (name, seed, label, itr, margin, scale)


def _header_arguments(name):
    text = open(os.path.join(ROOT, "include", "bdd_mma.h")).read()
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", text, re.S)
    assert m, name
    args = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    return [" ".join(a.split()) for a in args.split(",")]


def test_header_ctypes_table_and_library_agree():
    lib = capi.lib()
    V, D, U, I = C.c_void_p, C.c_double, C.c_uint64, C.c_int
    assert _header_arguments("bddmma_fused_small_history") == ["const bddmma_solver* s"]
    assert _header_arguments("bddmma_learned_iterations_history_batch") == [
        "bddmma_batch* b", "const void* dist_weights", "const void* omega_vec", "double omega", "uint64_t num_itr", "void* sol_avg", "void* lb_first_diff_avg",
        "void* lb_second_diff_avg", "uint64_t compute_history_for_itr", "double history_avg_beta", "int on_device"]
    assert capi.SIGNATURES["bddmma_fused_small_history"] == (I, [V])
    assert capi.SIGNATURES["bddmma_learned_iterations_history_batch"] == (I, [V, V, V, D, U, V, V, V, U, D, I])
    # the call this one extends keeps its signature
    assert capi.SIGNATURES["bddmma_learned_iterations_batch"] == (I, [V, V, V, D, U, I])
    # null handles are refused before any device call
    assert lib.bddmma_fused_small_history(None) == -1
    assert lib.bddmma_learned_iterations_history_batch(None, None, None, 0.5, 1, None, None, None, 1, 0.9, 0) == capi.ERR_INVALID_ARGUMENT


def test_classes_carry_the_history_form():
    assert callable(bdd_hip_parallel_mma.fused_small_history)
    p = inspect.signature(bdd_hip_batch.learned_iterations_history).parameters
    assert list(p) == ["self", "dist_weights", "num_itr", "omega", "omega_vec", "compute_history_for_itr", "history_avg_beta", "sol_avg", "lb_first_diff_avg",
                       "lb_second_diff_avg"]
    assert p["compute_history_for_itr"].default == 0 and p["history_avg_beta"].default == 0.9
    hpp = open(os.path.join(ROOT, "bdd_amd", "csrc", "bdd_hip_parallel_mma.hpp")).read()
    assert "bddmma_learned_iterations_history_batch(" in hpp and "bddmma_fused_small_history(" in hpp
