"""CPU side of tests/test_gpu_onchip_forward.py: every instance of tests/onchip_forward_shapes.py really lands on the solve sweeps that
keep the potentials on chip (kernels/narrow4.hpp) with the packs the GPU test is about — so that an instance that silently falls back
cannot pass there as a twin-equals-twin comparison.  The rule of init() (solver_impl.hpp): narrow packs of 128 slots alone, layer
records the third generation accepts, resident headers (one stage group per pack), and the longest pack within the kernels' capacity:
10 hops, 12 hops (both potentials on chip), 16 hops (F on chip behind k_fwd_narrow3)."""
import ctypes as C

import numpy as np
import pytest

from bdd_amd import capi
from onchip_forward_shapes import CAPACITY, HOPS, PACK_FILL, rows
from test_layout import Layout


@pytest.mark.parametrize("wpb", [4, 8])
@pytest.mark.parametrize("shape", sorted(HOPS))
def test_shape_lands_on_the_on_chip_sweeps(shape, wpb):
    col, _ = rows(shape)
    lay = Layout(col, pack_width=128, waves_per_block=wpb, pack_fill=PACK_FILL.get(shape, 0), chip=(4, 0, 0))
    assert lay.pack_width == 128 and lay.wpb == wpb
    assert lay.np_n > 0 and lay.np_w == 0 and lay.np_h == 0          # narrow packs alone
    info = np.zeros(5, np.uint32)
    capi.check(lay.L.bddmma_layout_layer_records(lay.h, 4, info.ctypes.data_as(C.c_void_p), None, None), None)
    assert info[0] == 1                                              # a lane per layer: <= 2 nodes per layer, <= 64 layers per hop
    assert lay.res_ok                                                # resident headers
    np.testing.assert_array_equal(np.diff(lay.pack_group_ptr), 1)    # one stage group per pack
    assert lay.res_max_layers <= 640
    hops = (lay.pack_hdr[:, 5] & 0xFFFF).astype(int)
    np.testing.assert_array_equal(hops, np.diff(lay.sets[0]["pack_hop_ptr"]))
    assert (hops.min(), hops.max()) == HOPS[shape]
    assert min(c for c in (10, 12, 16) if hops.max() <= c) == CAPACITY[shape]   # the smallest capacity that holds the longest pack
    assert lay.np_n > 4                                              # four packs per workgroup: more than one workgroup
    groups = [hops[i:i + wpb] for i in range(0, lay.np_n, wpb)]
    if shape == "rows2_10":
        assert lay.np_n > wpb and lay.np_n % wpb != 0                # several workgroups, the last one with missing packs
    if shape in ("rows2_10", "rows10_12"):
        assert any(len(set(g)) > 1 for g in groups)                  # packs of different hop counts in one workgroup
