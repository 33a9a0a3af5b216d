"""The entry points of a batch's per-BDD solutions, cost updates and perturbation gradient, checked without a GPU:
bddmma_bdds_solution_batch, bddmma_update_costs_batch and bddmma_grad_cost_perturbation_batch are declared in include/bdd_mma.h with
exactly their argument lists, exported by the built library and bound in bdd_amd/capi.py alike, the Python and C++ classes carry the
methods, a null batch is refused before any device call, and the LDS the solution launch asks for is the bound gradient's region
(kernels/batchbound.hpp) and fits the chip.  tests/test_gpu_batch_perturb.py has the numbers."""
import ctypes as C
import inspect
import os
import re

from bdd_amd import capi
from bdd_amd.solver import bdd_hip_batch, bdd_hip_parallel_mma
from test_batch_costs_abi import _header_arguments
from test_batch_smooth_abi import _evaluate, _return_expression
from test_capi_symbols import declared_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bdd_amd", "csrc")
_V, _I = C.c_void_p, C.c_int
NEW = {"bddmma_bdds_solution_batch": (["bddmma_batch* b", "char* sol", "int on_device"], [_V, _V, _I]),
       "bddmma_update_costs_batch": (["bddmma_batch* b", "const void* lo", "const void* hi", "int elem_precision", "int on_device"], [_V, _V, _V, _I, _I]),
       "bddmma_grad_cost_perturbation_batch": (["bddmma_batch* b", "const void* grad_lo", "const void* grad_hi", "void* grad_lo_pert_out",
                                                "void* grad_hi_pert_out", "int on_device"], [_V, _V, _V, _V, _V, _I])}


def test_entry_points_are_declared_exported_and_bound_alike():
    lib = capi.lib()
    for name, (args, argtypes) in NEW.items():
        assert name in declared_symbols()
        assert _header_arguments(name) == args
        res, bound = capi.SIGNATURES[name]
        assert res is C.c_int and bound == argtypes, (name, bound)
        f = getattr(lib, name)   # AttributeError: the built library does not export it
        assert f.restype is C.c_int and list(f.argtypes) == argtypes


def test_a_null_batch_is_refused_before_any_device_call():
    lib = capi.lib()
    buf = (C.c_double * 4)()
    for on_device in (0, 1):
        assert lib.bddmma_bdds_solution_batch(None, buf, on_device) == capi.ERR_INVALID_ARGUMENT
        assert lib.bddmma_bdds_solution_batch(None, None, on_device) == capi.ERR_INVALID_ARGUMENT
        for prec in (capi.F32, capi.F64):
            assert lib.bddmma_update_costs_batch(None, buf, buf, prec, on_device) == capi.ERR_INVALID_ARGUMENT
            assert lib.bddmma_update_costs_batch(None, None, None, prec, on_device) == capi.ERR_INVALID_ARGUMENT
        assert lib.bddmma_grad_cost_perturbation_batch(None, buf, buf, buf, buf, on_device) == capi.ERR_INVALID_ARGUMENT
        assert lib.bddmma_grad_cost_perturbation_batch(None, None, None, None, None, on_device) == capi.ERR_INVALID_ARGUMENT


def test_python_and_cpp_classes_carry_the_methods():
    """names and out= conventions are the member class's"""
    for name, params in (("bdds_solution_vec", ["self", "out"]), ("update_costs", ["self", "cost_delta_0", "cost_delta_1"]),
                         ("grad_cost_perturbation", ["self", "grad_lo", "grad_hi", "out"])):
        p = inspect.signature(getattr(bdd_hip_batch, name)).parameters
        assert list(p) == params, name
        assert "out" not in p or p["out"].default is None, name
        assert list(inspect.signature(getattr(bdd_hip_parallel_mma, name)).parameters) == params, name
    hpp = open(os.path.join(CSRC, "bdd_hip_parallel_mma.hpp")).read()
    batch_class = hpp[hpp.index("class bdd_hip_batch {"):]
    batch_class = batch_class[:batch_class.index("\n};")]
    for name in NEW:
        assert name + "(b_" in batch_class, name
    for member in ("void bdds_solution_vec(char* dev_out)", "void update_costs(const REAL* dev_cost_delta_0, const REAL* dev_cost_delta_1)",
                   "void grad_cost_perturbation(const REAL* dev_grad_lo, const REAL* dev_grad_hi, REAL* dev_grad_lo_pert_out, REAL* dev_grad_hi_pert_out)"):
        assert member in batch_class, member


def test_the_solution_launch_asks_for_the_bound_gradients_region_and_it_fits_the_chip():
    """a pack's region of k_small_solution_batch is bound_region_bytes — the resident region, 64 marks and a decision per layer, rounded
    up to 16 — because the kernel runs bound_path_pass, which addresses exactly that; the launch passes the LDS of the bound gradient's
    group.  At the capacities of a pack of 64 slots and 64 layers 16 regions in double are below the LDS of a compute unit."""
    fns = {}
    for name in ("res2_f_off", "res2_c_off", "res2_wave_bytes"):
        args, expr = _return_expression(os.path.join(CSRC, "layout.hpp"), name)
        fns[name] = (lambda a, e: lambda *v: _evaluate(e, **dict(zip(a, v)), **{k: f for k, f in fns.items()}))(args, expr)
    text = open(os.path.join(CSRC, "kernels", "batchbound.hpp")).read()
    m = re.search(r"inline uint32_t bound_region_bytes\(uint32_t real_size, uint32_t ns, uint32_t nl\)\s*\{\s*return (.*?);\s*\}", text, re.S)
    assert m, "bound_region_bytes"
    region = lambda real_size, ns, nl: _evaluate(m.group(1), real_size=real_size, ns=ns, nl=nl, **fns)
    for real_size in (4, 8):
        ns, nl = 1024 // real_size, 512 // real_size   # layout.hpp: res2_slot_capacity / res2_layer_capacity of 64 slots and 64 layers
        r = region(real_size, ns, nl)
        assert r % 16 == 0 and 0 <= r - (fns["res2_wave_bytes"](real_size, ns, nl) + 64 * real_size + nl * real_size) < 16
    assert region(4, 256, 128) == 4112 and region(8, 128, 64) == 4640
    lds = re.search(r"uint32_t lds_bytes = (\d+) \* 1024;", open(os.path.join(CSRC, "layout.hpp")).read())
    assert lds, "layout.hpp: ChipInfo::lds_bytes"
    assert 16 * region(8, 128, 64) == 74240 < int(lds.group(1)) * 1024 == 160 * 1024
    # the kernel takes its region from the shared path pass and has no workgroup barrier; the host passes the bound groups' LDS
    sol = open(os.path.join(CSRC, "kernels", "batchsol.hpp")).read()
    kernel = sol[sol.index("k_small_solution_batch(const BoundItem<REAL>*"):sol.index("struct PerturbItem")]
    assert "bound_path_pass<REAL>(dyn_lds, it, p, lane" in kernel and "__syncthreads" not in kernel
    assert text.count("(hi_path - lo_path) > 0") == 1 and "hi_path" not in sol   # the tie rule exists once
    assert text.count("bound_path_pass<REAL>(dyn_lds, it, p, lane") == 1          # ... and the bound gradient calls it too
    bt = open(os.path.join(CSRC, "solver_bt.hpp")).read()
    assert "g.lds = std::max(g.lds, sm.n_packs * bound_region_bytes((uint32_t)sizeof(REAL), sm.ns, sm.nl));" in bt
    assert "hipLaunchKernelGGL(bp_sol_fn[k], dim3(G.count), dim3(G.threads), G.lds, stream, (const BoundItem<REAL>*)(d_bb_items + G.first), o);" in bt
