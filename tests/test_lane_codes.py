"""The lane-affine predicate and the lane codes of the lane-per-BDD solve sweeps (csrc/layout.hpp: LaneCodes, kernels/narrow5.hpp) — CPU.

Against a restatement written from the layer records alone (tests/lane_sweep_shapes.py): which of the shapes of
tests/onchip_forward_shapes.py are lane-affine, their codes bit for bit, a fixture on which the predicate is false (the restatement finds
the cross-lane arc there), the dyadic fixtures tests/test_gpu_lane_sweeps.py runs against the oracle, and the two new symbols of the C
ABI."""
import os
import re

import numpy as np
import pytest

from bdd_amd import capi
from lane_sweep_shapes import (A, B, BOT, CODE_HOPS, NOT_AFFINE_OPTS, REAL, TOP, TWO, lane_codes, layer_records, not_affine_rows, pack_words,
                               restate)
from onchip_forward_shapes import HOPS, PACK_FILL, rows
from test_layout import Layout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def hops_of(lay):
    return np.diff(lay.sets[0]["pack_hop_ptr"]).astype(int)


def check_against_restatement(lay):
    """-> (usable, affine by the restatement, cross-lane arcs); the library's answer equals the restatement's, codes included"""
    rec, rec_off = layer_records(lay)
    assert rec is not None
    hops = hops_of(lay)
    affine, codes, cross = restate(rec, rec_off, hops)
    ok, lib_affine, words, code_off = lane_codes(lay)
    assert lib_affine == affine
    assert ok == (affine and hops.max() <= CODE_HOPS)
    assert bool(cross) <= (not affine)
    if ok:
        assert words.shape[0] == 64 * len(codes)                       # one table per structure template
        for p in range(lay.np_n):
            got = words[int(code_off[p]):int(code_off[p]) + 64]
            np.testing.assert_array_equal(got, pack_words(codes[int(rec_off[p])]), err_msg=f"pack {p}")
        same_template = {}
        for p in range(lay.np_n):                                      # packs share a table exactly where they share their records
            assert same_template.setdefault(int(rec_off[p]), int(code_off[p])) == int(code_off[p])
    return ok, affine, cross


@pytest.mark.parametrize("wpb", [4, 8])
@pytest.mark.parametrize("shape", sorted(HOPS))
def test_shapes_against_the_restatement(shape, wpb):
    col, _ = rows(shape)
    lay = Layout(col, pack_width=128, waves_per_block=wpb, pack_fill=PACK_FILL.get(shape, 0), chip=(4, 0, 0))
    ok, affine, cross = check_against_restatement(lay)
    # rows packed longest first: the BDD of a lane never changes, whatever the mix of lengths (pinned to what the restatement says)
    assert affine and not cross
    assert ok == (HOPS[shape][1] <= CODE_HOPS)                         # rows13: affine, but beyond the code words


def test_codes_use_every_target_and_both_flags():
    """the restatement's codes of a mixed shape name all four targets, one- and two-node layers and lanes without a layer"""
    col, _ = rows("rows2_10")
    lay = Layout(col, pack_width=128, waves_per_block=4, chip=(4, 0, 0))
    rec, rec_off = layer_records(lay)
    _, codes, _ = restate(rec, rec_off, hops_of(lay))
    arcs, flags = set(), set()
    for tab in codes.values():
        real = (tab >> 8) & REAL != 0
        flags |= set(np.unique(tab >> 8).tolist())
        for k in range(2):
            arcs |= set(np.unique((tab[real] >> (2 * k)) & 3).tolist())
        two = (tab >> 8) & TWO != 0
        for k in range(2, 4):
            arcs |= set(np.unique((tab[two] >> (2 * k)) & 3).tolist())
        assert np.all(tab[~real] & 0xFF == 0xFF)                       # lanes without a layer: four arcs at BOT
    assert arcs == {A, B, TOP, BOT} and flags == {0, REAL, REAL | TWO}


@pytest.mark.parametrize("wpb", [4, 8])
def test_a_shorter_bdd_before_a_longer_one_is_not_lane_affine(wpb):
    col, _ = not_affine_rows()
    lay = Layout(col, waves_per_block=wpb, chip=(4, 0, 0), **NOT_AFFINE_OPTS)
    assert lay.np_n > wpb
    ok, affine, cross = check_against_restatement(lay)
    assert not ok and not affine
    assert cross                                                       # the restatement finds an arc into another lane's layer ...
    assert min(h for _, h, _, _ in cross) == 3                         # ... first where the rows of 4 end: hop 3's arcs of the rows of 9
    # the same rows in the default order (longest first) are lane-affine
    lay = Layout(col, pack_width=128, waves_per_block=wpb, chip=(4, 0, 0))
    ok, affine, cross = check_against_restatement(lay)
    assert ok and affine and not cross


@pytest.mark.parametrize("shape", ["rows10", "rows2_10", "rows11", "rows2"])
def test_dyadic_fixtures_are_lane_affine(shape):
    """the premise of tests/test_gpu_lane_sweeps.py::test_against_the_double_oracle"""
    import dyadic_fixtures
    fill = {"rows11": 76, "rows2": 64}                                 # as tests/test_gpu_dyadic_parity.py: ONCHIP_FILL
    col, _ = dyadic_fixtures.rows(shape)
    for wpb in (4, 8):
        lay = Layout(col, pack_width=128, waves_per_block=wpb, pack_fill=fill.get(shape, 0), chip=(4, 0, 0))
        ok, affine, _ = check_against_restatement(lay)
        assert ok and affine


def test_refused_without_layer_records():
    """no layer records (packs of 64 slots): no codes either, and the query says so"""
    col, _ = rows("hop3")
    lay = Layout(col, pack_width=64)
    rec, _ = layer_records(lay)
    assert rec is None
    assert lane_codes(lay) == (False, False, None, None)


# ---------------------------------------------------------------- C ABI (as tests/test_onchip_hops_abi.py)
def read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def test_symbols_are_declared_defined_and_bound():
    h, c = read("include", "bdd_mma.h"), read("bdd_amd", "csrc", "capi.cpp")
    assert re.search(r"^int bddmma_lane_sweeps\(const bddmma_solver\* s\);", h, re.M)
    assert h.index("int bddmma_onchip_hops(") < h.index("int bddmma_lane_sweeps(") < h.index("int bddmma_precision(")
    assert re.search(r"^int bddmma_lane_sweeps\(const bddmma_solver\* s\)\s*\{", c, re.M)
    assert re.search(r"^int bddmma_layout_lane_codes\(const bddmma_layout\* l, int real_size, uint32_t\* info, uint32_t\* words, uint32_t\* code_off\);", h, re.M)
    assert h.index("int bddmma_layout_layer_records(") < h.index("int bddmma_layout_lane_codes(") < h.index("int bddmma_layout_seg_exchange(")
    assert re.search(r"^int bddmma_layout_lane_codes\(const bddmma_layout\* l, int real_size, uint32_t\* info, uint32_t\* words, uint32_t\* code_off\)\s*\{", c, re.M)
    assert capi.SIGNATURES["bddmma_lane_sweeps"] == capi.SIGNATURES["bddmma_onchip_hops"]
    assert capi.SIGNATURES["bddmma_layout_lane_codes"] == capi.SIGNATURES["bddmma_layout_layer_records"]
    L = capi.lib()
    assert L.bddmma_lane_sweeps(None) == -1                            # no solver: the error value of the diagnostics next to it
    info = np.zeros(5, np.uint32)
    assert L.bddmma_layout_lane_codes(None, 4, info.ctypes.data_as(capi.C.c_void_p), None, None) == capi.ERR_INVALID_ARGUMENT
    from bdd_amd.solver import bdd_hip_parallel_mma
    assert callable(getattr(bdd_hip_parallel_mma, "lane_sweeps"))


def test_bit_and_getter_are_documented():
    h = read("include", "bdd_mma.h")
    m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int bddmma_lane_sweeps", h, re.S)
    assert m and all(w in m.group(1) for w in ("narrow5", "bit 24", "-1 without"))
    assert re.search(r"bit 24: no lane-per-BDD sweeps", h)
