"""bddmma_onchip_hops is declared in the C header next to bddmma_potentials_on_chip, defined in the library's C-ABI source, exported by
the built library, bound in capi.py and reachable from the Python class."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def test_symbol_is_declared_defined_and_bound():
    h = read("include", "bdd_mma.h")
    assert re.search(r"^int bddmma_onchip_hops\(const bddmma_solver\* s\);", h, re.M)
    assert h.index("int bddmma_potentials_on_chip(") < h.index("int bddmma_onchip_hops(") < h.index("int bddmma_precision(")
    assert re.search(r"^int bddmma_onchip_hops\(const bddmma_solver\* s\)\s*\{", read("bdd_amd", "csrc", "capi.cpp"), re.M)
    from bdd_amd import capi
    assert capi.SIGNATURES["bddmma_onchip_hops"] == capi.SIGNATURES["bddmma_potentials_on_chip"]
    assert capi.lib().bddmma_onchip_hops(None) == -1   # no solver: the error value of the diagnostics next to it
    from bdd_amd.solver import bdd_hip_parallel_mma
    assert callable(getattr(bdd_hip_parallel_mma, "onchip_hops"))


def test_capacities_are_documented():
    m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int bddmma_onchip_hops", read("include", "bdd_mma.h"), re.S)
    assert m and all(w in m.group(1) for w in ("0 (", "10 or", "12 (", "16 ("))
