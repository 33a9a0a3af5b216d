"""Iteration rate of N solver objects created one after another in one process (the placement of their arrays differs from object to object):
   python tools/objects_rate.py [float|double] [objects] [V] [k] [pack_fill] [rows]
   (rows of k variables, default 10; pack_fill default 0 = full packs; rows default V / 2)"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bdd_amd import capi
if os.environ.get("BDDMMA_LIB"):
    capi.LIB_PATH = os.path.abspath(os.environ["BDDMMA_LIB"])
from bdd_amd.instances import random_set_cover_mt
from bdd_amd.solver import bdd_hip_parallel_mma
prec = sys.argv[1] if len(sys.argv) > 1 else "double"
n = int(sys.argv[2]) if len(sys.argv) > 2 else 6
V = int(sys.argv[3]) if len(sys.argv) > 3 else 1_000_000
k = int(sys.argv[4]) if len(sys.argv) > 4 else 10
fill = int(sys.argv[5]) if len(sys.argv) > 5 else 0
B = int(sys.argv[6]) if len(sys.argv) > 6 else V // 2
col, costs = random_set_cover_mt(V, B, k, 12345)
rates = []
what = ""
for i in range(n):
    s = bdd_hip_parallel_mma(col, costs, precision=prec, pack_fill=fill)
    what = f"{s.nr_bdd_nodes()} nodes, {s.nr_packs()} packs, {s.solve_sweep_kind()}, on chip {s.potentials_on_chip()}" + \
           (f" ({s.onchip_hops()} hops)" if hasattr(s, "onchip_hops") else "")
    s.iterations(300); s.synchronize()
    ms = s.time_iterations(1000)
    rates.append(1000 / ms * 1e3)
    s.close()
print(f"{os.environ.get('BDDMMA_LIB', 'shipped'):22s} {prec} V={V} B={B} k={k} fill={fill} [{what}]: " + " ".join(f"{r:6.0f}" for r in rates) + f"   mean {sum(rates) / len(rates):6.0f}", flush=True)
