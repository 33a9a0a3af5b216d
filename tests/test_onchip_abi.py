"""bddmma_potentials_on_chip is declared in the C header, defined in the library's C-ABI source, bound in capi.py and reachable from the
Python class; variant_flags bit 21 is documented in the header."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def test_symbol_is_declared_defined_and_bound():
    assert re.search(r"^int bddmma_potentials_on_chip\(const bddmma_solver\* s\);", read("include", "bdd_mma.h"), re.M)
    assert re.search(r"^int bddmma_potentials_on_chip\(const bddmma_solver\* s\)\s*\{", read("bdd_amd", "csrc", "capi.cpp"), re.M)
    from bdd_amd import capi
    res, args = capi.SIGNATURES["bddmma_potentials_on_chip"]
    assert (res, args) == capi.SIGNATURES["bddmma_nontemporal_loads"]
    from bdd_amd.solver import bdd_hip_parallel_mma
    assert callable(getattr(bdd_hip_parallel_mma, "potentials_on_chip"))


def test_bit_21_is_documented():
    h = read("include", "bdd_mma.h")
    m = re.search(r"bit 21:([^\n]*)", h)
    assert m and "keep F and T in memory" in m.group(1)
