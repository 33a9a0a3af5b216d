"""Primal rounding of a batch, one launch per perturbation round (bddmma_perturb_primal_costs_batch,
bddmma_incremental_mm_agreement_rounding_batch: kernels/batchround.hpp; ComputePrimalSolution on a batch) on the MI355X.

The reference of every comparison is a twin of each member driven alone through the per-member calls.  Every comparison is bit for bit:
minima are exact in any order, the per-variable sums keep the order of var_layers, the quotient and the sum of the cost update are formed
in double and rounded once as the per-member kernels form them, and the iterations between two rounds are the device function the member
alone runs — which leaves no room for a tolerance.  The member sets are those of tests/test_gpu_batch_costs.py::names_of: one pack
(assign3, mostly padding lanes; assign9 with more than 64 layers on one wave), set covers of 2, 4, 7 and 10 packs (10 packs: 16 waves of
which 6 are idle, float only) and mixed3x9.  Every test asserts nr_packs() and fused_small() first (fused()).

`rounds[i]` is the INDEX of the round in which member i's agreement was seen, so the per-member loop finds it with num_rounds =
rounds[i] + 1 and does not with num_rounds = rounds[i]: that is the boundary test 3 checks on a twin."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from bdd_amd import capi  # noqa: E402
from bdd_amd.solver import bdd_hip_batch, bdd_hip_lbfgs, bdd_hip_parallel_mma  # noqa: E402
from test_gpu_batch_bounds import set_both  # noqa: E402
from test_gpu_batch_costs import VIEWS, fused, member_set, names_of, offsets, random_costs, refused, state, views  # noqa: E402
from test_gpu_small_learned import AUTOGRAD_MEMBERS  # noqa: E402

LOOP = dict(init_delta=0.1, delta_growth_rate=1.2, num_itr_lb=5)
AGREEING = ("assign3", "cover40x60", "assign8", "cover67x100")


def assert_views(names, members, twins, what):
    for n, s, q in zip(names, members, twins):
        for x, y, nm in zip(views(s), views(q), VIEWS):
            np.testing.assert_array_equal(x, y, err_msg=f"{what}, {n}: {nm}")


def agreed(r, s):
    return r["counts"][0] + r["counts"][1] == s.nr_variables()


def assert_round(names, got, want, what):
    """the per-member dicts of a batch round against the twins' own: counts, both cost differences, and sol (zeros where the member did
    not agree, in both)"""
    assert len(got) == len(want) == len(names)
    for n, g, w in zip(names, got, want):
        assert g["counts"] == w["counts"], (what, n, g["counts"], w["counts"])
        for k in ("sol", "cost_delta_0", "cost_delta_1"):
            assert g[k].dtype == w[k].dtype and g[k].shape == w[k].shape, (what, n, k)
            np.testing.assert_array_equal(g[k], w[k], err_msg=f"{what}, {n}: {k}")


def twin_loop(q, num_rounds, seed):
    return q.primal_rounding_incremental(LOOP["init_delta"], LOOP["delta_growth_rate"], LOOP["num_itr_lb"], False, num_rounds, seed)


# ---------------------------------------------------------------- 1. one round
@pytest.mark.parametrize("precision", ["float", "double"])
def test_one_batch_round_equals_each_members_own(precision):
    """behind a batch set of random costs with non-zero deferred differences, behind 3 iterations, with stale sweep states on two members
    only, behind 20 more iterations, and behind sets of costs from {0, 1} and of zero costs; two (round_index, seed) pairs"""
    names = names_of(precision)
    members, twins = member_set(names, precision), member_set(names, precision)
    batch = bdd_hip_batch(members)
    rng = np.random.default_rng(81)
    total = np.zeros(4, np.int64)
    hashed = 0

    def both_iterate(k):
        batch.iterations(k)
        for q in twins:
            q.iterations(k)

    def stale_two():
        for i in (1, len(members) - 1):
            v = members[i].nr_variables()
            d0, d1 = rng.uniform(-0.5, 0.5, v), rng.uniform(-0.5, 0.5, v)
            members[i].update_costs(d0, d1)
            twins[i].update_costs(d0, d1)

    def set_integer(hi_max):
        """lo and hi from {0, .., hi_max}, no deferred differences: ties between the two min-marginals of a layer; with hi_max = 0 every
        path of every BDD costs 0, so every variable is of the `equal` type and draws from the hash"""
        n, dt = int(offsets(members)[-1]), members[0].value_type
        set_both(batch, twins, (rng.integers(0, hi_max + 1, n).astype(dt), rng.integers(0, hi_max + 1, n).astype(dt), np.zeros(n, dt)))

    # (random costs and iterations alone never gave the `equal` type on this set, in neither precision: the last two states add it)
    states = [("behind a batch set", lambda: set_both(batch, twins, random_costs(members, rng))), ("behind 3 iterations", lambda: both_iterate(3)),
              ("behind update_costs on two members", stale_two), ("behind 20 more iterations", lambda: both_iterate(20)),
              ("behind a set of costs from {0, 1}", lambda: set_integer(1)), ("behind a set of zero costs", lambda: set_integer(0))]
    for round_index, seed in ((0, 0), (3, 17)):
        for what, prepare in states:
            prepare()
            delta = 0.1 * (1 + round_index)
            got = batch.perturb_primal_costs(delta, round_index, seed)
            want = [q.perturb_primal_costs(delta, round_index, seed) for q in twins]
            print(precision, what, (round_index, seed), [w["counts"] for w in want])
            assert_round(names, got, want, f"{precision}, {what}, {(round_index, seed)}")
            assert_views(names, members, twins, f"{precision}, {what}, {(round_index, seed)}")
            for w in want:
                total += np.asarray(w["counts"], np.int64)
                hashed += w["counts"][2] + w["counts"][3] > 0
                assert np.any(w["cost_delta_0"] != 0) or np.any(w["cost_delta_1"] != 0)
    assert np.all(total > 0), total     # all four types occur over the set
    assert hashed > 0                   # the hash of (variable, round, seed) is exercised
    batch.close()


# ---------------------------------------------------------------- 2. agreement and perturbation in one launch
@pytest.mark.parametrize("precision", ["float", "double"])
def test_an_agreeing_member_keeps_its_costs_beside_members_that_are_perturbed(precision):
    names = AGREEING
    members, twins = member_set(names, precision), member_set(names, precision)
    batch = bdd_hip_batch(members)
    batch.iterations(300)
    batch.distribute_delta()   # the deferred differences go into lo / hi here, so that the round's own distribute_delta adds zeros
    for q in twins:
        q.iterations(300)
        q.distribute_delta()
    before = [s.get_solver_costs() for s in members]
    want = [q.perturb_primal_costs(0.1, 0, 5) for q in twins]
    done = [agreed(w, q) for w, q in zip(want, twins)]
    print(precision, [w["counts"] for w in want], done)
    assert any(done) and not all(done), done   # on the twins: a member whose min-marginals agree beside members whose do not
    got = batch.perturb_primal_costs(0.1, 0, 5)
    assert_round(names, got, want, precision)
    for n, s, bf, d, g in zip(names, members, before, done, got):
        after = s.get_solver_costs()
        if d:   # lo, hi and the (cleared) deferred differences bit-equal to before the call
            for k in (0, 1, 2):
                np.testing.assert_array_equal(after[k], bf[k], err_msg=f"{precision}, {n}: {VIEWS[k]} of an agreeing member changed")
            assert set(np.unique(g["sol"])) <= {0, 1} and g["sol"].sum() == g["counts"][0]
        else:
            assert np.any(after[0] != bf[0]) or np.any(after[1] != bf[1]), n
    assert_views(names, members, twins, f"{precision}, first round")
    # a second round: the agreeing member agrees again and stays as it is
    want2 = [q.perturb_primal_costs(0.12, 1, 5) for q in twins]
    got2 = batch.perturb_primal_costs(0.12, 1, 5)
    assert_round(names, got2, want2, f"{precision}, second round")
    for n, s, bf, d in zip(names, members, before, done):
        if d:
            after = s.get_solver_costs()
            for k in (0, 1, 2):
                np.testing.assert_array_equal(after[k], bf[k], err_msg=f"{precision}, {n}: {VIEWS[k]} changed in the second round")
    assert_views(names, members, twins, f"{precision}, second round")
    batch.close()


# ---------------------------------------------------------------- 3. the loop
@pytest.mark.parametrize("precision", ["float", "double"])
def test_the_batch_loop_equals_each_members_own_loop(precision):
    names = names_of(precision)
    rng = np.random.default_rng(83)
    seen = {}
    for num_rounds in (2, 40):
        members, twins = member_set(names, precision), member_set(names, precision)
        batch = bdd_hip_batch(members)
        got, rounds = batch.primal_rounding_incremental(num_rounds=num_rounds, seed=9, return_rounds=True, **LOOP)
        want = [twin_loop(q, num_rounds, 9) for q in twins]
        print(precision, num_rounds, rounds, [bool(w) for w in want])
        assert len(got) == len(want) == len(names)
        for n, g, w, r, q in zip(names, got, want, rounds, twins):
            assert g == w, (precision, num_rounds, n)
            assert (r < num_rounds) == bool(w) and 0 <= r <= num_rounds, (n, r)
            assert not w or (len(w) == q.nr_variables() and set(w) <= {0.0, 1.0})
        assert_views(names, members, twins, f"{precision}, {num_rounds} rounds")
        # what the last distribute_delta of each member's loop applied
        for n, s, q in zip(names, members, twins):
            g_lo, g_hi = rng.normal(0, 1, s.nr_layers()).astype(s.value_type), rng.normal(0, 1, s.nr_layers()).astype(s.value_type)
            np.testing.assert_array_equal(s.grad_distribute_delta(g_lo, g_hi), q.grad_distribute_delta(g_lo, g_hi), err_msg=f"{precision}, {num_rounds} rounds, {n}")
        seen[num_rounds] = (rounds, [bool(w) for w in want])
        batch.close()
    # on the twins: with 2 rounds some member is not found; with 40 some member is found in a round >= 1 (iterations between rounds,
    # members dropping out at different rounds, the mask)
    assert not all(seen[2][1]), seen[2]
    late = [i for i, (r, f) in enumerate(zip(*seen[40])) if f and r >= 1]
    assert late, seen[40]
    assert len(set(seen[40][0])) >= 2, seen[40]   # they leave at different rounds (or never)
    # the round index of one such member, on fresh twins: found with rounds + 1 rounds, not found with `rounds`
    i = late[0]
    r = seen[40][0][i]
    assert twin_loop(fused(names[i], precision), r + 1, 9), (names[i], r)
    assert twin_loop(fused(names[i], precision), r, 9) == [], (names[i], r)


# ---------------------------------------------------------------- 4. ordering without host synchronisation
@pytest.mark.parametrize("precision", ["float", "double"])
def test_member_iterations_and_the_batch_loop_order_themselves(precision):
    names = names_of(precision)
    members, twins = member_set(names, precision), member_set(names, precision)
    batch = bdd_hip_batch(members)
    for s in members:
        s.iterations(50)
    got = batch.primal_rounding_incremental(num_rounds=6, seed=2, **LOOP)
    for s in members:
        s.iterations(3)
    want = []
    for q in twins:
        q.iterations(50)
        q.synchronize()
        want.append(twin_loop(q, 6, 2))
        q.iterations(3)
        q.synchronize()
    assert got == want
    assert_views(names, members, twins, precision)
    batch.close()


# ---------------------------------------------------------------- 5. refusals
def test_refusals_are_decided_before_any_member_or_output_is_touched():
    names = ("assign8", "cover40x60", "cover67x100", "assign3")
    members = member_set(names, "float")
    batch = bdd_hip_batch(members)
    L, h = batch._L, batch._h
    dt = members[0].value_type
    nv = int(sum(s.nr_variables() for s in members))
    rng = np.random.default_rng(85)
    batch.set_solver_costs(*random_costs(members, rng))
    batch.iterations(2)
    before = [state(s) for s in members]

    def unchanged(what):
        for nme, s, bf in zip(names, members, before):
            for x, y, nm in zip(state(s), bf, VIEWS):
                np.testing.assert_array_equal(x, y, err_msg=f"{what}, {nme}: {nm}")

    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    counts = np.full(4 * len(members), 77, np.uint32)
    sol = np.full(nv, 7, np.int8)
    c0, c1 = np.full(nv, -7.0, dt), np.full(nv, -7.0, dt)
    found = (C.c_int * len(members))(*([7] * len(members)))
    rounds = (C.c_uint64 * len(members))(*([7] * len(members)))
    cp = counts.ctypes.data_as(C.POINTER(C.c_uint32))

    def untouched(what):
        assert np.all(counts == 77) and np.all(sol == 7) and np.all(c0 == -7.0) and np.all(c1 == -7.0), what
        assert list(found) == [7] * len(members) and list(rounds) == [7] * len(members), what
        unchanged(what)

    inv = capi.ERR_INVALID_ARGUMENT
    # a required null array
    for args in ((None, ptr(sol), ptr(c0), ptr(c1)), (cp, None, ptr(c0), ptr(c1))):
        assert L.bddmma_perturb_primal_costs_batch(h, 0.1, 0, 0, *args) == inv
        assert b"null" in L.bddmma_batch_last_error(h)
    for args in ((None, found, rounds), (ptr(sol), None, rounds)):
        assert L.bddmma_incremental_mm_agreement_rounding_batch(h, 0.1, 1.2, 5, 3, 0, *args) == inv
        assert b"null" in L.bddmma_batch_last_error(h)
    untouched("null arrays")
    # init_delta <= 0, delta_growth_rate <= 0
    for init_delta, growth in ((0.0, 1.2), (-0.1, 1.2), (0.1, 0.0), (0.1, -1.0), (float("nan"), 1.2)):
        assert L.bddmma_incremental_mm_agreement_rounding_batch(h, init_delta, growth, 5, 3, 0, ptr(sol), found, rounds) == inv
        assert b"positive" in L.bddmma_batch_last_error(h)
    untouched("init_delta / delta_growth_rate")
    # a member with an L-BFGS wrapper attached
    wrapper = bdd_hip_lbfgs(members[2])
    calls = (lambda: batch._check(L.bddmma_perturb_primal_costs_batch(h, 0.1, 0, 0, cp, ptr(sol), ptr(c0), ptr(c1)), h),
             lambda: batch._check(L.bddmma_incremental_mm_agreement_rounding_batch(h, 0.1, 1.2, 5, 3, 0, ptr(sol), found, rounds), h),
             lambda: batch.perturb_primal_costs(0.1), lambda: batch.primal_rounding_incremental(**LOOP))
    for call in calls:
        msg = refused(capi.ERR_STATE, call)
        assert "member 2" in msg and "L-BFGS" in msg, msg
    untouched("an L-BFGS wrapper")
    wrapper.close()
    batch.close()
    # accepted again on a fresh set
    fresh = member_set(names, "float")
    batch = bdd_hip_batch(fresh)
    assert len(batch.perturb_primal_costs(0.1)) == len(names)
    assert len(batch.primal_rounding_incremental(num_rounds=2, **LOOP)) == len(names)
    batch.close()


# ---------------------------------------------------------------- 6. autograd
COUNTED = [(cls, name) for cls in (bdd_hip_batch, bdd_hip_parallel_mma) for name in ("set_solver_costs", "primal_rounding_incremental", "perturb_primal_costs")]


def counters(monkeypatch):
    calls = {}
    for cls, name in COUNTED:
        f, key = getattr(cls, name), f"{'batch' if cls is bdd_hip_batch else 'member'}.{name}"
        calls[key] = 0

        def wrapper(*a, _f=f, _key=key, **kw):
            calls[_key] += 1
            return _f(*a, **kw)
        monkeypatch.setattr(cls, name, wrapper)
    return calls


def run_primal(solvers, arrays, tdt):
    import torch
    from bdd_amd.autograd import ComputePrimalSolution
    t = [torch.tensor(v, dtype=tdt, device="cuda") for v in arrays]
    out = ComputePrimalSolution(solvers, *t, LOOP["init_delta"], LOOP["delta_growth_rate"], LOOP["num_itr_lb"])
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("precision", ["float", "double"])
def test_compute_primal_solution_of_a_batch_makes_batch_calls_only(precision, monkeypatch):
    """On a batch: one batch set and one batch loop, no call on a member; on a list n of each member call; with a member that has had an
    L-BFGS wrapper the batch's first call refuses with BDDMMA_ERR_STATE, touching nothing, and the list form runs.  The results are the
    list form's in all three."""
    import torch
    tdt = torch.float64 if precision == "double" else torch.float32
    a, b, c, d = ([fused(n, precision) for n in AUTOGRAD_MEMBERS] for _ in range(4))
    n = len(a)
    batch, batch_c = bdd_hip_batch(a), bdd_hip_batch(c)
    arrays = random_costs(a, np.random.default_rng(86))
    calls = counters(monkeypatch)
    zero = {k: 0 for k in calls}
    got = run_primal(batch, arrays, tdt)
    assert calls == {**zero, "batch.set_solver_costs": 1, "batch.primal_rounding_incremental": 1}, calls
    calls.update(zero)
    want = run_primal(list(b), arrays, tdt)
    assert calls == {**zero, "member.set_solver_costs": n, "member.primal_rounding_incremental": n}, calls
    assert got == want and len(got) == n
    assert any(got) and all(len(x) in (0, s.nr_variables()) for x, s in zip(got, a))
    for s, q in zip(a, b):
        for x, y, nm in zip(state(s), state(q), VIEWS):
            np.testing.assert_array_equal(x, y, err_msg=f"{precision}: {nm}")
    for s in (c[1], d[1]):
        wrapper = bdd_hip_lbfgs(s)
        wrapper.iteration()
        wrapper.close()
    calls.update(zero)
    got_c = run_primal(batch_c, arrays, tdt)
    assert calls["batch.primal_rounding_incremental"] == 0 and calls["member.primal_rounding_incremental"] == n and calls["member.set_solver_costs"] == n, calls
    assert got_c == run_primal(list(d), arrays, tdt)
    assert [bool(x) for x in got_c] == [bool(x) for x in want]
    batch.close(), batch_c.close()
