"""What tests/test_lane_codes.py (CPU) and tests/test_gpu_lane_sweeps.py (GPU) share: a restatement of the lane-affine predicate and the lane
codes (csrc/layout.hpp: LaneCodes) written from the layer records alone, and a fixture on which the predicate is false."""
import ctypes as C

import numpy as np

from bdd_amd import BddCollection, capi

W = 128
A, B, TOP, BOT = 0, 1, 2, 3
TWO, REAL = 1, 2
CODE_HOPS = 12
NO_LANE_SWEEPS = 0x1000000   # variant_flags bit 24


def layer_records(lay, real_size=4):
    info = np.zeros(5, np.uint32)
    capi.check(lay.L.bddmma_layout_layer_records(lay.h, real_size, info.ctypes.data_as(C.c_void_p), None, None), None)
    if not info[0]:
        return None, None
    words, off = np.zeros(int(info[1]), np.uint32), np.zeros(lay.np_n, np.uint32)
    capi.check(lay.L.bddmma_layout_layer_records(lay.h, real_size, info.ctypes.data_as(C.c_void_p), words.ctypes.data_as(C.c_void_p),
                                                 off.ctypes.data_as(C.c_void_p)), None)
    return words.reshape(-1, 4), off


def lane_codes(lay, real_size=4):
    """-> (usable, affine, words [n, 4] or None, code_off or None)"""
    info = np.zeros(5, np.uint32)
    capi.check(lay.L.bddmma_layout_lane_codes(lay.h, real_size, info.ctypes.data_as(C.c_void_p), None, None), None)
    if not info[0]:
        assert info[1] == 0
        return False, bool(info[2]), None, None
    words, off = np.zeros(int(info[1]), np.uint32), np.zeros(lay.np_n, np.uint32)
    capi.check(lay.L.bddmma_layout_lane_codes(lay.h, real_size, info.ctypes.data_as(C.c_void_p), words.ctypes.data_as(C.c_void_p),
                                              off.ctypes.data_as(C.c_void_p)), None)
    return True, bool(info[2]), words.reshape(-1, 4), off


def restate(rec, rec_off, hops, S=4):
    """The predicate and the codes from the layer records: -> (affine, {first record of a template: codes [64 lanes][hops] of 10 bits},
    cross) where cross lists (first record, hop, lane, arc) of arcs that end outside the lane's own layer one hop down and its sinks."""
    codes, cross, affine = {}, [], True
    for p, first in enumerate(rec_off):
        first, nh = int(first), int(hops[p])
        if first in codes:
            continue
        tab = np.zeros((64, nh), np.uint32)
        for h in range(nh):
            r = rec[first + h * 64:first + (h + 1) * 64].astype(np.int64)
            rn = rec[first + (h + 1) * 64:first + (h + 2) * 64].astype(np.int64) if h + 1 < nh else None
            for l in range(64):
                top, bot = (W + 2 * l) * S, (W + 2 * l + 1) * S
                flags = int(r[l, 2] >> 16)
                real, two = bool(flags & REAL), bool(flags & TWO)
                if h == 0 and real and (two or int(r[l, 2] & 0xFFFF) != l * S):
                    affine = False
                nflags = int(rn[l, 2] >> 16) if rn is not None else 0
                na = int(rn[l, 2] & 0xFFFF) if nflags & REAL else None
                nb = na + S if (nflags & REAL) and (nflags & TWO) else None
                code = flags << 8
                for k in range(4):
                    off = int(r[l, k // 2] >> (16 * (k & 1))) & 0xFFFF
                    present = real and (k < 2 or two)
                    if not present:
                        c = BOT
                        if off != bot:
                            affine = False
                    elif off == top:
                        c = TOP
                    elif off == bot:
                        c = BOT
                    elif off == na:
                        c = A
                    elif off == nb:
                        c = B
                    else:
                        c = BOT
                        affine = False
                        cross.append((first, h, l, k))
                    code |= c << (2 * k)
                tab[l, h] = code
        codes[first] = tab
    return affine, codes, cross


def pack_words(tab):
    """[64][hops] codes -> the [64][4] words of the table: three hops per word from bit 0 up, absent hops as lanes without a layer"""
    out = np.zeros((64, 4), np.uint32)
    for h in range(CODE_HOPS):
        c = tab[:, h] if h < tab.shape[1] else np.full(64, 0xFF, np.uint32)
        out[:, h // 3] |= c.astype(np.uint32) << np.uint32(10 * (h % 3))
    return out


V = 500


def not_affine_rows():
    """Covering / simplex rows of 4 and 9 variables alternating, to be packed in input order (keep_bdd_order = 1): a shorter BDD sits before
    a longer one in every pack, so from hop 4 on the longer BDD's layer moves to a lower lane."""
    rng = np.random.Generator(np.random.PCG64(151))
    col = BddCollection()
    for i in range(800):
        k = 4 if i % 2 == 0 else 9
        (col.add_covering if rng.random() < 0.5 else col.add_simplex)(np.sort(rng.choice(V, size=k, replace=False)))
    costs = rng.normal(0, 3, col.nr_variables()).round(3)
    return col, costs


NOT_AFFINE_OPTS = dict(pack_width=128, keep_bdd_order=1)
