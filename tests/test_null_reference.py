"""CPU pins of tests/null_reference.py: its dynamic programme against the brute-force enumeration of all 4^M windows, for
M = 1, 2, 3, 6 (1..3 lie below order + 1 for some order), orders 0..3 and both starts.  At 200 thresholds across the
score range the bounds taken from the quantised distribution enclose the exact tail and are no looser than twice the
quantisation error allows (check_tails: inequalities, no calibrated tolerance); the pmf sums to 1; the stationary
distribution is one."""
import numpy as np
import pytest

from tests import null_reference as R


def test_contexts_and_next_context():
    assert [R.contexts(o) for o in range(4)] == [1, 5, 21, 85]
    assert R.context_of([], 3) == 0 and R.context_of([2], 3) == 3 and R.context_of([1, 2], 3) == 5 + 6
    assert R.context_of([3, 1, 2, 0], 3) == 21 + 16 + 8 and R.context_of([3, 1, 2, 0], 1) == 1 and R.context_of([3], 0) == 0
    for order in range(4):
        for s in range(R.contexts(order)):
            assert R.context_of(R.letters_of(s), order) == s
            for a in range(4):
                assert R.letters_of(R.next_context(order, s, a)) == (R.letters_of(s) + [a])[-order:] if order else True
    assert R.next_context(0, 0, 3) == 0


@pytest.mark.parametrize("order", [0, 1, 2, 3])
def test_stationary_is_stationary(order):
    P = R.dirichlet_probabilities(order, 7 + order)
    pi = R.stationary(P, order)
    base = (4 ** order - 1) // 3
    assert abs(pi.sum() - 1.0) < 1e-14 and np.all(pi[:base] == 0) and np.all(pi[base:] > 0)
    out = np.zeros_like(pi)
    for s in range(R.contexts(order)):
        for a in range(4):
            out[R.next_context(order, s, a)] += pi[s] * P[s, a]
    assert np.abs(out - pi).max() < 1e-14


@pytest.mark.parametrize("kind", ["stationary", "run"])
@pytest.mark.parametrize("order", [0, 1, 2, 3])
@pytest.mark.parametrize("M", [1, 2, 3, 6])
def test_dp_against_enumeration(M, order, kind):
    rng = np.random.default_rng(100 * M + 10 * order + (kind == "run"))
    P = R.dirichlet_probabilities(order, 31 + order)
    init = R.start(P, order, kind)
    w, c = rng.standard_normal((M, 4)) * 1.5, float(rng.standard_normal())
    x, p = R.enumerate_windows(w, c, P, init, order)
    assert abs(p.sum() - 1.0) < 1e-12
    for step in (2.0 ** -4, 0.37):
        q, offset, err, G = R.quantise(w, c, step)
        assert q.min() == 0 and np.all(q.min(axis=1) == 0) and err <= M * step / 2 + 1e-15
        pmf = R.dp(q, P, init, order)
        assert pmf.shape == (G,) and abs(pmf.sum() - 1.0) < 1e-12 and pmf.min() >= 0
        t = np.linspace(x.min() - 2.0 * err - 0.1, x.max() + 2.0 * err + 0.1, 200)      # both ends beyond every bound's reach
        lower, upper = R.grid_tail(pmf, offset, step, t + err), R.grid_tail(pmf, offset, step, t - err)
        R.check_tails(lower, upper, x, p, t, err)
        assert lower[0] == pytest.approx(1.0, abs=1e-12) and upper[-1] == 0.0


def test_exact_weights_give_the_exact_distribution():
    """weights that are multiples of the step: err = 0, and the grid distribution is the enumeration's"""
    rng = np.random.default_rng(5)
    P = R.dirichlet_probabilities(2, 3)
    init = R.start(P, 2, "stationary")
    w = rng.integers(-8, 9, size=(4, 4)) / 4.0
    q, offset, err, G = R.quantise(w, 0.5, 0.25)
    assert err == 0.0
    pmf = R.dp(q, P, init, 2)
    x, p = R.enumerate_windows(w, 0.5, P, init, 2)
    want = np.bincount(np.rint((x - offset) / 0.25).astype(np.int64), weights=p, minlength=G)
    assert np.abs(pmf - want).max() < 1e-14
