"""CPU tests of the NumPy restatement of the learned iterations (tests/learned_mma_restatement.py), pinned against the oracle-made
fixtures under tests/golden/: with isotropic weights it reproduces the bound trajectory of iteration() (iter_lb_*), and with weight 1
on every layer — the un-normalised sums added back as they are — the per-pass delta trace of the forward_mm / backward_mm protocol
(delta_trace_*, lb_trace_*).  The GPU tests compare the solver with this restatement."""
import numpy as np
import pytest

from learned_mma_restatement import History, LearnedMma, ema
from util import GOLDEN, load_golden, suffix

TOL = {"double": 1e-12, "float": 1e-5}


def _close(a, b, precision, scale=1.0):
    return abs(a - b) <= TOL[precision] * max(abs(b), scale)


def _restatement(name, precision):
    _, z = load_golden(name)
    m = LearnedMma(z["instr"], z["delims"], precision)
    m.update_costs_hi(np.asarray(z["costs"], np.float64))
    return m, z


@pytest.mark.parametrize("name", GOLDEN)
@pytest.mark.parametrize("precision", ["double", "float"])
def test_isotropic_weights_reproduce_iteration_trajectory(name, precision):
    m, z = _restatement(name, precision)
    sfx = suffix(precision)
    assert m.lower_bound() == float(z[f"lb_init_{sfx}"])
    lbs = []
    ran = m.iterations(m.isotropic_alpha(), 20, 0.5, improvement_slope=0.0, lb_trajectory=lbs)
    assert ran == 20
    ref = z[f"iter_lb_{sfx}"]
    scale = max(1.0, float(np.abs(ref).max()))
    for it in range(20):
        assert _close(lbs[it], float(ref[it]), precision, scale), (it, lbs[it], float(ref[it]))


@pytest.mark.parametrize("name", GOLDEN)
@pytest.mark.parametrize("precision", ["double", "float"])
def test_unit_weights_reproduce_delta_trace(name, precision):
    """weight 1 everywhere adds the sums S back un-divided: the reference's forward_mm(0.5, d); backward_mm(0.5, d) protocol"""
    m, z = _restatement(name, precision)
    sfx = suffix(precision)
    ones = np.ones(m.n_layers, m.dt)
    trace, lb_trace = z[f"delta_trace_{sfx}"], z[f"lb_trace_{sfx}"]
    V = trace.shape[2] // 2
    m.backward_run()
    scale = max(1.0, float(np.abs(trace).max()))
    for it in range(10):
        m.forward_pass(0.5, *m.weighted_delta(ones))
        np.testing.assert_allclose(m.sums()[:V].ravel(), trace[it, 0], rtol=TOL[precision], atol=TOL[precision] * scale)
        m.backward_pass(0.5, *m.weighted_delta(ones))
        np.testing.assert_allclose(m.sums()[:V].ravel(), trace[it, 1], rtol=TOL[precision], atol=TOL[precision] * scale)
        assert _close(m.lower_bound(), float(lb_trace[it]), precision, scale)
    # and the isotropic weights turn those sums into S / n, what normalize_delta makes of them
    S = m.sums()
    dlo, dhi = m.weighted_delta(m.isotropic_alpha())
    nb = m.nbdds[m.layer_var].astype(m.dt)
    np.testing.assert_allclose(dlo, S[m.layer_var, 0] / nb, rtol=TOL[precision], atol=0)
    np.testing.assert_allclose(dhi, S[m.layer_var, 1] / nb, rtol=TOL[precision], atol=0)


def test_matching_first_row_dyadic_trajectory():
    m, _ = _restatement("matching_3x3_first_row", "double")
    lbs = []
    m.iterations(m.isotropic_alpha(), 2, 0.5, improvement_slope=0.0, lb_trajectory=lbs)
    assert lbs == [-4.78125, -4.3671875]


def test_history_rules_by_hand():
    """four tracked iterations with beta = 0.5 on made-up per-BDD bounds and solutions, the averages worked out by hand"""
    beta = np.float64(0.5)
    h = History(beta)
    sol_avg, lb1, lb2 = np.full(2, 7.0), np.full(2, 7.0), np.full(2, 7.0)
    sols = [np.array([1.0, 0.0]), np.array([1.0, 1.0]), np.array([0.0, 1.0]), np.array([0.0, 0.0])]
    lbs = [np.array([1.0, 10.0]), np.array([2.0, 14.0]), np.array([4.0, 16.0]), np.array([5.0, 16.0])]
    h.step(sols[0], lbs[0], sol_avg, lb1, lb2)                  # the first solution is copied; nothing else is touched
    assert sol_avg.tolist() == [1.0, 0.0] and lb1.tolist() == [7.0, 7.0] and lb2.tolist() == [7.0, 7.0]
    h.step(sols[1], lbs[1], sol_avg, lb1, lb2)                  # changes (1, 4) copied
    assert sol_avg.tolist() == [1.0, 0.5] and lb1.tolist() == [1.0, 4.0] and lb2.tolist() == [7.0, 7.0]
    h.step(sols[2], lbs[2], sol_avg, lb1, lb2)                  # changes (2, 2): EMA (1.5, 3); second differences (1, -2) copied
    assert sol_avg.tolist() == [0.5, 0.75] and lb1.tolist() == [1.5, 3.0] and lb2.tolist() == [1.0, -2.0]
    h.step(sols[3], lbs[3], sol_avg, lb1, lb2)                  # changes (1, 0): EMA (1.25, 1.5); second diff (-1, -2): EMA (0, -2)
    assert sol_avg.tolist() == [0.25, 0.375] and lb1.tolist() == [1.25, 1.5] and lb2.tolist() == [0.0, -2.0]
    assert h.tracked == 4


def test_ema_rounding_of_float():
    """beta * avg in float, (1 - beta) * cur and the sum in double, one rounding to float"""
    avg = np.array([0.1], np.float32)
    cur = np.array([0.3], np.float32)
    b = np.float32(0.9)
    want = np.float32(np.float64(b * avg[0]) + (1.0 - np.float64(b)) * np.float64(cur[0]))
    assert ema(avg, cur, b)[0] == want and ema(avg, cur, b).dtype == np.float32


def test_stopping_rule_and_history_count():
    """improvement_slope > 0 stops once the bound moves less than slope * the first iteration's change and the history is complete;
    the count returned is the number of iterations run, and initial_lb_change is set once per solver"""
    m, _ = _restatement("matching_3x3_first_row", "double")
    a = m.isotropic_alpha()
    lbs = []
    ran = m.iterations(a, 200, 0.5, improvement_slope=1e-3, lb_trajectory=lbs)
    assert 1 < ran < 200
    first = m.initial_lb_change
    assert first == abs(-5.0 - lbs[0])
    assert abs(lbs[-1] - lbs[-2]) < 1e-3 * first and all(abs(lbs[i] - lbs[i - 1]) >= 1e-3 * first for i in range(1, ran - 1))
    sol, l1, l2 = np.zeros(m.n_layers), np.zeros(m.n_bdds), np.zeros(m.n_bdds)
    ran2 = m.iterations(a, 200, 0.5, improvement_slope=1e-3, sol_avg=sol, lb_first_diff_avg=l1, lb_second_diff_avg=l2,
                        compute_history_for_itr=3)
    assert m.initial_lb_change == first
    assert 3 <= ran2 < 200
