"""Digests of the device layout (csrc/layout.cpp: build_layout) for a fixed list of configurations, CPU only.

A configuration is (instance, options, (real_size, n_cus, lds_bytes_per_cu)).  For each one the layout is built through
bddmma_layout_create_for_chip and one line per item is printed: a SHA-256 of every bddmma_layout_size value, of every array of the
checkpoint format (ids 1-39, fetched as 100 + id), and of narrow_words and slot_to_instr.  Two libraries (BDDMMA_LIB) or two thread
counts (BDDMMA_THREADS) build the same layouts exactly when their outputs are equal line for line:

    BDDMMA_LIB=/path/to/other/libbdd_mma_hip.so BDDMMA_THREADS=1 python tools/layout_digest.py > a.txt
    BDDMMA_THREADS=16 python tools/layout_digest.py > b.txt && cmp a.txt b.txt

    python tools/layout_digest.py --small           the configurations of tests/test_layout_digest.py only (each well under a second)
    python tools/layout_digest.py --small --write   rewrite tests/golden/layout_digests.json after a deliberate change of a rule
    python tools/layout_digest.py --brief           one line per configuration: a SHA-256 over its per-array lines (profiles/r08_layout_digest.txt)
    python tools/layout_digest.py --list            names only

What the list is for — the branches of build_layout each configuration is there to reach — stands next to each entry."""
import argparse
import ctypes as C
from functools import partial
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np

from bdd_amd import BddCollection, capi, native
from bdd_amd.instances import assignment_ilp, random_set_cover, random_set_cover_mixed, random_set_cover_mt

GOLDEN = os.path.join(ROOT, "tests", "golden", "layout_digests.json")
MI355X = (0, 0)   # n_cus, lds_bytes_per_cu: 0 = the defaults of bddmma_layout_create
SMALL_CHIP = (8, 160 * 1024)
# element type of every checkpoint array (include/bdd_mma.h: bddmma_layout_copy)
ID_DTYPE = {i: np.uint32 for i in range(1, 40)}
ID_DTYPE.update({3: np.uint64, 36: np.uint64, 37: np.uint64, 13: np.uint8, 17: np.uint8, 21: np.uint8, 23: np.uint16, 33: np.uint16, 38: np.uint16, 39: np.uint16})
N_SIZES = 25


# ---- instances -----------------------------------------------------------------------------------------------------------------------
def _families():
    import sum_marginals_restatement as sm
    split = lambda: native.lp_to_bdd_collection(assignment_ilp(8, None).write_lp(), split=True, split_length=4)
    return {   # tests/test_gpu_sum_marginals.py: FAMILIES
        "cover10_w64": (lambda: sm.cover10(seed=5, V=200, rows=300)[0], dict(pack_width=64)),
        "cover10_w128": (lambda: sm.cover10(seed=5, V=200, rows=300)[0], dict(pack_width=128)),
        "cover10_w256": (lambda: sm.cover10(seed=5, V=200, rows=300)[0], dict(pack_width=256)),
        "wide2": (lambda: sm.wide_rows()[0], dict(pack_width=64, wide_pack_width=512, resident_sweeps=1, variant_flags=0x3)),
        "mixed": (lambda: sm.wide_rows()[0], dict(pack_width=64, wide_pack_width=512, resident_sweeps=1)),
        "huge": (lambda: sm.huge_rows()[0], dict()),
        "knapsack_w64": (lambda: sm.knapsack_rows()[0], dict(pack_width=64)),
        "assignment8": (lambda: sm.assignment8()[0], dict()),
        "staggered_rows": (lambda: random_set_cover_mixed(300, 200, 3, 16, seed=4)[0], dict()),
        "split_bdds": (split, dict()),
    }


def knapsack(n_rows, k, V, max_coeff, seed, covering=0, cover_k=5):
    """n_rows general linear rows of k variables (diamond-shaped BDDs, every one its own shape) in front of `covering` covering rows"""
    rng = np.random.Generator(np.random.PCG64(seed))
    rows = []
    for _ in range(n_rows):
        co = rng.integers(1, max_coeff, size=k)
        rows.append((co, np.sort(rng.choice(V, size=k, replace=False)), "<=", int(co.sum() // 2)))
    for _ in range(covering):
        rows.append((np.ones(cover_k, int), np.sort(rng.choice(V, size=cover_k, replace=False)), ">=", 1))
    return native.rows_to_bdd_collection(rows)


def chained():   # tests/test_layout.py: test_roundtrip_chained_packs
    rng = np.random.Generator(np.random.PCG64(77))
    col = BddCollection()
    V = 60
    for lo, hi, cmax, n in ((15, 20, 40, 14), (8, 13, 12, 30)):   # layers of 59-135 nodes (wide packs), then up to ~40 (narrow packs)
        for _ in range(n):
            k = int(rng.integers(lo, hi))
            co = rng.integers(1, cmax, size=k)
            col.add_linear(co, "<=", int(co.sum() // 2), np.sort(rng.choice(V, size=k, replace=False)))
    for _ in range(40):
        col.add_covering(np.sort(rng.choice(V, size=5, replace=False)))
    return col


def uniform_runs():   # tests/test_layout.py: test_uniform_shape_runs_are_packed_in_closed_form
    rng = np.random.Generator(np.random.PCG64(3))
    col = BddCollection()
    V = 4000
    col.add_covering(np.sort(np.array([rng.choice(V, 7, replace=False) for _ in range(700)]), axis=1).astype(np.uint64))
    for r in np.sort(np.array([rng.choice(V, 4, replace=False) for _ in range(300)]), axis=1).astype(np.uint64):
        col.add_simplex(r)
    col.add_covering(np.sort(rng.choice(V, 5, replace=False)).astype(np.uint64)[None, :])   # a class of one
    col.permute(rng.permutation(col.nr_bdds()))
    return col


def fill_rows():   # tests/test_layout.py: test_pack_fill_trades_lanes_for_packs
    col, _ = random_set_cover(3000, 2000, 6, seed=7)
    col.add_linear(np.arange(1, 13), "<=", 30, np.arange(12))
    return col


def sparse_variables(V):
    """300 covering rows whose last variable is V - 1: the automatic bin size is a function of the variable count alone"""
    rng = np.random.Generator(np.random.PCG64(V))
    col = BddCollection()
    for _ in range(300):
        col.add_covering(np.sort(rng.choice(V, size=6, replace=False)))
    col.add_covering(np.array([0, 1, V - 1]))
    return col


def long_rows(packs):   # tests/test_layout.py: test_stage_groups_shrink_to_fit_the_launch_into_one_round_of_workgroups
    return random_set_cover(4000, 32 * packs, 50, seed=packs)[0]


def long_bdds():   # tests/test_layout.py: test_roundtrip_long_bdds_many_groups
    rng = np.random.Generator(np.random.PCG64(4))
    col = BddCollection()
    col.add_simplex(np.sort(rng.choice(500, size=300, replace=False)))
    for _ in range(60):
        col.add_covering(np.sort(rng.choice(500, size=int(rng.integers(2, 90)), replace=False)))
    return col


def configurations():
    """[(name, make instance, options, real_size, (n_cus, lds), small)] — instances are built lazily and shared by name of the maker"""
    cfg = []
    add = lambda name, make, opts=None, real_size=4, chip=MI355X, small=True: cfg.append((name, make, opts or {}, real_size, chip, small))
    # sweep families, both value sizes.  huge: huge packs; assignment8 / split_bdds / ...: the 64-slot retry for few packs; wide2 / mixed: wide packs
    # side by side, explicit wide_pack_width
    for fam, (make, opts) in _families().items():
        for rs in (4, 8):
            add(f"family/{fam}/r{rs}", make, opts, rs)
    # packing: closed form (classes of >= 256), classes below 256, every BDD order, pack_fill
    add("pack/uniform_runs/w128", uniform_runs, dict(pack_width=128))
    add("pack/uniform_runs/auto", uniform_runs)
    mixed9 = lambda: random_set_cover_mixed(6_000, 4_000, 3, 9, seed=4)[0]
    for kbo in (0, 1, 2):
        add(f"pack/keep_bdd_order{kbo}", mixed9, dict(keep_bdd_order=kbo))
    add("pack/fill32", fill_rows, dict(pack_width=64, pack_fill=32))
    add("pack/fill16_wpb2", fill_rows, dict(pack_width=64, pack_fill=16, waves_per_block=2))
    add("pack/fill_retry_refused", fill_rows, dict(pack_fill=100))   # the 64-slot retry fails its option check: the 128-slot layout stays
    # pack_stagger 1 / explicit, narrow and wide; (64, 0): the explicit chain of narrow packs narrows nothing (few wide BDDs)
    for pw, ww in ((64, 192), (128, 256), (64, 0)):
        add(f"stagger/side_by_side/{pw}_{ww}", chained, dict(pack_width=pw, wide_pack_width=ww, pack_stagger=1))
        add(f"stagger/explicit60/{pw}_{ww}", chained, dict(pack_width=pw, wide_pack_width=ww, pack_stagger=60))
    add("stagger/explicit60/auto_width", chained, dict(pack_stagger=60))
    # exchange: the clamps of the automatic bin size, explicit sizes, entries by variable
    add("bins/min_512", partial(sparse_variables, 3000))
    add("bins/clamp_1024", partial(sparse_variables, 300_000))
    add("bins/double_2048", partial(sparse_variables, 1_000_000), real_size=8)
    add("bins/float_above_2048", partial(sparse_variables, 1_000_000))
    add("bins/max_9728", partial(sparse_variables, 2_600_000))
    add("bins/explicit64_stage128", lambda: random_set_cover(400, 300, 6, seed=1)[0], dict(pack_width=64, vars_per_bin=64, stage_cap=128))
    add("bins/by_variable", lambda: random_set_cover(400, 300, 6, seed=1)[0], dict(pack_width=64, exchange_by_variable=2))
    for w in (0, 1, 2, 8):
        add(f"groups/long_bdds/wpb{w}", long_bdds, dict(pack_width=64, stage_cap=64, vars_per_bin=64, waves_per_block=w))
    # stage groups on an 8-CU chip: the one-round rule (100 / 116 / 126 packs), kept where it fits (80) or nothing fits (140), float; the
    # third-workgroup rule (four packs per workgroup, 80 / 140 packs); bins of fewer than 512 variables (long rows: min_vb from one_chunk_vars)
    for packs in (80, 100, 116, 126, 140):
        add(f"groups/one_round/{packs}", long_rows.__get__(packs), dict(pack_width=64), 8, SMALL_CHIP)
        add(f"groups/wpb4/{packs}", long_rows.__get__(packs), dict(pack_width=64, waves_per_block=4), 8, SMALL_CHIP)
    add("groups/one_round/100/float", partial(long_rows, 100), dict(pack_width=64), 4, SMALL_CHIP)
    add("groups/explicit640/100", partial(long_rows, 100), dict(pack_width=64, stage_cap=640), 8, SMALL_CHIP)
    add("groups/auto_width/100", partial(long_rows, 100), None, 8, SMALL_CHIP)

    # ---- the large ones (seconds each): tool only
    big = lambda name, make, opts=None, real_size=4, chip=MI355X: add(name, make, opts, real_size, chip, small=False)
    cover_res = lambda: random_set_cover(150_000, 70_400, 10, seed=5)[0]       # 2 200 packs of 64 slots
    big("wpb/resident_rule_1", cover_res, dict(pack_width=64))
    big("wpb/resident_rule_off_32cus", cover_res, dict(pack_width=64), 4, (32, 160 * 1024))
    big("wpb/resident_rule_off_by_option", cover_res, dict(pack_width=64, resident_sweeps=1))
    big("wpb/one_by_halving", lambda: random_set_cover(100_000, 50_000, 10, seed=2)[0], dict(vars_per_bin=64, pack_width=128))   # 782 packs: halved down to one
    big("wpb/two_1500_packs", lambda: random_set_cover(100_000, 96_000, 10, seed=2)[0], dict(pack_width=128))
    cover8 = lambda: random_set_cover(20_000, 262_144, 3, seed=8)[0]           # 4 096 packs of 128 slots: the smallest with eight
    big("wpb/eight", cover8, dict(vars_per_bin=64))
    big("wpb/four_long_runs", cover8)
    big("wpb/four_by_option", cover8, dict(vars_per_bin=64, waves_per_block=4))
    big("wpb/eight/double", cover8, dict(vars_per_bin=64), 8)
    cover_flat = lambda: random_set_cover(300_000, 150_000, 10, seed=1)[0]     # no retry (2 344 packs, not chained); automatic stagger finds nothing to chain
    big("retry/neither", cover_flat)
    big("stagger/auto_flat_rows_kept_order", cover_flat, dict(keep_bdd_order=1))
    big("stagger/explicit30_flat_rows_kept_order", cover_flat, dict(keep_bdd_order=1, pack_stagger=30))
    # general linear rows: automatic narrow staggering, the retry for mostly chained packs, one pack per workgroup by staggering
    rows12 = lambda: knapsack(24_000, 12, 3000, 30, seed=11)   # 3.3 M nodes
    big("stagger/auto_narrow", rows12)
    big("stagger/auto_narrow/double", rows12, None, 8)
    big("stagger/auto_narrow/w128", rows12, dict(pack_width=128))
    big("stagger/off_by_option", rows12, dict(pack_stagger=1))
    # ... with wide rows behind staggered narrow packs: the wide packs narrow to one BDD; and wide rows alone: automatic wide staggering
    big("wide/narrowed_behind_staggered", knapsack_mix)
    big("wide/narrowed_off_by_wpb", knapsack_mix, dict(waves_per_block=1))
    rows18 = lambda: knapsack(3_000, 18, 2000, 40, seed=13)
    big("wide/auto_stagger", rows18)
    big("wide/auto_stagger/option_width", rows18, dict(wide_pack_width=512))
    big("wide/share_caps_wpb", lambda: knapsack(400, 16, 5000, 30, seed=14, covering=66_000, cover_k=3), dict(pack_width=64))
    headline = lambda: random_set_cover_mt(1_000_000, 500_000, 10)[0]          # bench.py's instance, 10.5 M nodes
    big("headline/float", headline)
    big("headline/double", headline, None, 8)
    return cfg


def knapsack_mix():
    rng = np.random.Generator(np.random.PCG64(12))
    rows = []
    V = 3000
    for k, cmax, n in ((17, 40, 2500), (12, 30, 32_000)):
        for _ in range(n):
            co = rng.integers(1, cmax, size=k)
            rows.append((co, np.sort(rng.choice(V, size=k, replace=False)), "<=", int(co.sum() // 2)))
    return native.rows_to_bdd_collection(rows)


# ---- digest --------------------------------------------------------------------------------------------------------------------------
def digest(col, opts, real_size, chip):
    L = capi.lib()
    instr = np.ascontiguousarray(col.instr, dtype=np.uint64)
    delims = np.ascontiguousarray(col.delims, dtype=np.uint64)
    o = capi.Options()
    for k, v in opts.items():
        setattr(o, k, v)
    h = C.c_void_p()
    rc = L.bddmma_layout_create_for_chip(C.byref(h), instr.ctypes.data_as(C.c_void_p), delims.ctypes.data_as(C.c_void_p), col.nr_bdds(), C.byref(o),
                                         real_size, *chip)
    capi.check(rc, None)
    try:
        sizes = np.array([L.bddmma_layout_size(h, w) for w in range(N_SIZES)], np.uint64)
        out = [("sizes", hashlib.sha256(sizes.tobytes()).hexdigest())]

        def fetch(which, n, dt):
            a = np.zeros(max(n, 1), dt)
            capi.check(L.bddmma_layout_copy(h, which, a.ctypes.data_as(C.c_void_p)), None)
            return hashlib.sha256(a[:n].tobytes()).hexdigest()
        for i in range(1, 40):
            out.append((f"id{i:02d}", fetch(100 + i, int(L.bddmma_layout_size(h, 100 + i)), ID_DTYPE[i])))
        out.append(("narrow_words", fetch(0, int(sizes[1]), np.uint32)))
        out.append(("slot_to_instr", fetch(2, int(sizes[0]), np.uint64)))
        return out
    finally:
        L.bddmma_layout_destroy(h)


def run(small_only, names=None):
    made = {}
    for name, make, opts, real_size, chip, small in configurations():
        if (small_only and not small) or (names and name not in names):
            continue
        key = (make.func, make.args) if isinstance(make, partial) else make
        if key not in made:
            made.clear()   # one instance at a time: configurations of one instance follow each other
            made[key] = make()
        yield name, digest(made[key], opts, real_size, chip)


ITEMS = ["sizes"] + [f"id{i:02d}" for i in range(1, 40)] + ["narrow_words", "slot_to_instr"]   # the order digest() returns
PIN_HEX = 12   # the golden file keeps 48 bits of every digest, one string per configuration in ITEMS order


def pinned(lines):
    assert [what for what, _ in lines] == ITEMS
    return "".join(sha[:PIN_HEX] for _, sha in lines)


def brief(name, lines):
    """one line per configuration: a SHA-256 over its per-array lines"""
    text = "".join(f"{name} {what} {sha}\n" for what, sha in lines)
    return name + " " + hashlib.sha256(text.encode()).hexdigest()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--write", action="store_true")
    ap.add_argument("--brief", action="store_true")
    ap.add_argument("--list", action="store_true")
    ap.add_argument("names", nargs="*")
    a = ap.parse_args()
    if a.list:
        for name, *_rest, small in configurations():
            print(name, "" if small else "(large)")
        return
    result = {}
    for name, lines in run(a.small or a.write, set(a.names)):
        result[name] = pinned(lines)
        if a.brief:
            print(brief(name, lines), flush=True)
            continue
        for what, sha in lines:
            print(f"{name} {what} {sha}", flush=True)
    if a.write:
        with open(GOLDEN, "w") as f:
            json.dump(result, f, indent=0, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
