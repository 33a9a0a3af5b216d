"""The instances of tests/test_onchip_forward_layout.py (CPU: each one really lands on k_fwd_narrow4 / k_bwd_narrow4) and
tests/test_gpu_onchip_forward.py (GPU: those kernels against their twin).  V = 500, a few hundred rows, numpy PCG64 seeds below."""
import numpy as np

from bdd_amd import BddCollection

V = 500
SEEDS = {"hop1": 141, "hop2": 142, "hop3": 143, "rows2_10": 144, "rows11": 145, "rows12": 146, "rows10_12": 147, "rows13": 148}
# slots a pack fills per hop (0: all 128).  128 one-variable rows would be 128 layers in a hop, twice what a lane per layer serves; full
# packs of 11-13 hops would be more than the 640 layers of one stage group
PACK_FILL = {"hop1": 64, "rows11": 76, "rows12": 76, "rows10_12": 76, "rows13": 76}
# hops of the (shortest, longest) pack
HOPS = {"hop1": (1, 1), "hop2": (2, 2), "hop3": (3, 3), "rows2_10": (2, 10), "rows11": (11, 11), "rows12": (12, 12), "rows10_12": (10, 12),
        "rows13": (13, 13)}
# hop capacity of the on-chip kernels that serve the shape (bddmma_onchip_hops)
CAPACITY = {"hop1": 10, "hop2": 10, "hop3": 10, "rows2_10": 10, "rows11": 12, "rows12": 12, "rows10_12": 12, "rows13": 16}


def _mixed(col, rng, n, size):
    for i in range(n):
        k = size(i)
        (col.add_covering if rng.random() < 0.5 else col.add_simplex)(np.sort(rng.choice(V, size=k, replace=False)))


def _rows(shape):
    rng = np.random.Generator(np.random.PCG64(SEEDS[shape]))
    col = BddCollection()
    if shape == "hop1":          # 300 covering rows of one variable: the upward walk is its gather-only step alone, every child a sink
        for _ in range(300):
            col.add_covering(np.sort(rng.choice(V, size=1, replace=False)))
    elif shape == "hop2":        # 400 rows of two: one scattering hop, then the gather-only one
        _mixed(col, rng, 400, lambda i: 2)
    elif shape == "hop3":        # 400 rows of three: the shortest pack in which both sT buffers are written
        _mixed(col, rng, 400, lambda i: 3)
    elif shape == "rows2_10":    # 775 rows of 2-10 (13 packs): packs of different hop counts in one workgroup, a last workgroup with missing packs
        _mixed(col, rng, 775, lambda i: int(rng.integers(2, 11)))
    elif shape == "rows11":      # the 12-hop kernels, one hop short of their capacity
        _mixed(col, rng, 400, lambda i: 11)
    elif shape == "rows12":      # ... and at it
        _mixed(col, rng, 400, lambda i: 12)
    elif shape == "rows10_12":   # rows of 10 and 12 alternating every 64 BDDs: the 12-hop kernels with shorter packs beside full ones
        _mixed(col, rng, 500, lambda i: 12 if (i // 64) % 2 else 10)
    else:                        # rows of 13: beyond the forward form's reach (the 16-hop backward kernel behind k_fwd_narrow3)
        _mixed(col, rng, 400, lambda i: 13)
    costs = rng.normal(0, 3, col.nr_variables()).round(3)
    return col, costs


_CACHE = {}


def rows(shape):
    if shape not in _CACHE:
        _CACHE[shape] = _rows(shape)
    return _CACHE[shape]
