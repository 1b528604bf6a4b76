"""CPU-only pins of tests/background_reference.py, the reference every other background test compares with: the
sampler against direct thresholding, gaps, the statistics of a long sample against its table, and the round trip
fit -> thresholds -> sample -> fit through crbm_amd.background.MarkovBackground."""
import numpy as np

from tests import background_reference as R

SIGMAS = 5.0
MIN_VISITS = 1000         # contexts visited less often are not held to the bound


def test_context_index_and_counts_by_hand():
    assert [R.context_index(c) for c in ((), (0,), (3,), (0, 0), (1, 2), (3, 3), (0, 0, 0), (3, 3, 3))] == [0, 1, 4, 5, 11, 20, 21, 84]
    assert [R.contexts(o) for o in range(4)] == [1, 5, 21, 85]
    s = np.array([0, 1, 4, 1, 1, 2, 4, 4, 3], np.uint8)          # AC.CCG..T
    c = R.kmer_counts(s, 2)
    assert c.size == 84 and c[:4].tolist() == [1, 3, 1, 1]
    two = c[4:20].reshape(4, 4)
    assert two[0, 1] == 1 and two[1, 1] == 1 and two[1, 2] == 1 and two.sum() == 3
    three = c[20:].reshape(4, 4, 4)
    assert three[1, 1, 2] == 1 and three.sum() == 1
    brute = np.zeros(84, np.uint64)                              # explicit windows, one at a time
    t = R.gapped_stream(500, seed=3, gap_share=0.1)
    for j, off in ((1, 0), (2, 4), (3, 20)):
        for p in range(t.size - j + 1):
            w = t[p:p + j]
            if (w < 4).all():
                brute[off + int("".join(map(str, w)), 4)] += 1
    assert np.array_equal(R.kmer_counts(t, 2), brute)


def test_order_0_is_direct_thresholding():
    table = R.dirichlet_table(0, 1)
    for pos0 in (0, 5, 2 ** 34 - 6):
        u = R.draws(42, pos0, 1000)
        want = (u[:, None] >= table[0][None, :]).sum(axis=1).astype(np.uint8)
        assert np.array_equal(R.sample(table, 0, 1000, 42, pos0=pos0), want)
    assert np.array_equal(R.draws(42, 3, 50), R.draws(42, 0, 53)[3:])     # a draw belongs to its position


def test_gaps_survive_and_reset_the_context():
    M = R.M32
    table = np.array([[0, 0, 0]] + [[M, M, M]] * 4, np.uint32)   # the empty context draws T, every other one A
    tmpl = np.zeros(40, np.uint8)
    tmpl[[0, 9, 10, 25, 39]] = 4
    got = R.sample(table, 1, tmpl, seed=1)
    assert np.array_equal(got == 4, tmpl == 4)
    first = np.flatnonzero((tmpl != 4) & np.concatenate([[True], tmpl[:-1] == 4]))
    assert np.all(got[first] == 3)
    rest = (tmpl != 4)
    rest[first] = False
    assert np.all(got[rest] == 0)


def transition_counts(sample, order):
    """(contexts, 4) visits by letter drawn; a context as the sampler sees it (shorter behind the start or a gap)"""
    n = np.zeros((R.contexts(order), 4), np.int64)
    ctx = []
    for a in sample:
        if a == 4:
            ctx = []
            continue
        n[R.context_index(ctx), a] += 1
        ctx = (ctx + [int(a)])[-order:] if order else []
    return n


def within_bound(n, P):
    visits = n.sum(axis=1)
    held = visits >= MIN_VISITS
    sigma = np.sqrt(visits[:, None] * P * (1 - P))
    return held, np.abs(n - visits[:, None] * P)[held] <= SIGMAS * sigma[held] + 1e-9


def test_sample_statistics_match_the_table():
    """2 10^5 letters of a fixed order-2 table whose rows keep every letter at 0.1 or more: each of the 16 full contexts
    is visited about 12 500 times, far above the cap of 1000 visits; the shorter contexts are visited once."""
    rng = np.random.default_rng(2024)
    P = 0.1 + 0.6 * rng.dirichlet(np.ones(4), size=R.contexts(2))
    table = R.thresholds_from_probabilities(P)
    exact = R.probabilities_of(table)
    assert np.abs(exact - P).max() < 1e-9
    n = transition_counts(R.sample(table, 2, 200000, seed=7), 2)
    held, ok = within_bound(n, exact)
    assert held.sum() == 16 and held[5:].all() and ok.all()


def test_fit_sample_fit_round_trip():
    from crbm_amd.background import MarkovBackground
    rng = np.random.default_rng(5)
    P = 0.1 + 0.6 * rng.dirichlet(np.ones(4), size=R.contexts(2))
    first = R.sample(R.thresholds_from_probabilities(P), 2, 200000, seed=11)
    bg = MarkovBackground(2, R.kmer_counts(first, 2))
    table = bg.thresholds(pseudocount=1.0)
    again = R.sample(table, 2, 200000, seed=12)
    n = transition_counts(again, 2)
    held, ok = within_bound(n, R.probabilities_of(table))
    assert held.sum() == 16 and ok.all()
    refit = MarkovBackground(2, R.kmer_counts(again, 2))         # and the refitted table is the table, within the same bound
    q = refit.probabilities(pseudocount=0.0)[5:]
    visits = n.sum(axis=1)[5:, None]
    want = R.probabilities_of(table)[5:]
    assert np.all(np.abs(q - want) * visits <= SIGMAS * np.sqrt(visits * want * (1 - want)) + 1e-6)
