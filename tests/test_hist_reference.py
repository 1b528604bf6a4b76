"""The yardstick of the score histogram (tests/hist_reference.py) on the CPU, before any kernel is held to it: the
log-odds and the exact counts against a brute-force loop on a tiny model, check_histogram accepting the exact counts and
refusing a moved score, a lost window and a double count, and the input condition (at most 1 % of the scores inside the
bands) for models of the four shapes of tests/test_gpu_hist.py."""
import numpy as np
import pytest

from tests.emu import harness
from tests import hist_reference as H
from tests.scan_reference import stream_scores


def _stream(T, seed, gaps=(0, 9, 10, 31)):
    s = np.random.default_rng(seed).integers(0, 4, size=T, dtype=np.uint8)
    s[list(gaps)] = 4
    return s


@pytest.mark.parametrize("ds", [True, False])
def test_logodds_and_counts_against_a_brute_force_loop(ds):
    K, M, T, lo, hi, nbins = 3, 4, 40, -6.0, 2.0, 8
    o = harness.random_model(K, M, ds, 5)
    stream = _stream(T, 1)
    X, valid = H.stream_logodds(o, stream)
    S = 2 if ds else 1
    want = np.zeros((K, S, nbins), np.int64)
    n = 0
    for s0 in range(T - M + 1):
        win = stream[s0:s0 + M]
        assert valid[s0] == bool((win < 4).all())
        if not valid[s0]:
            assert np.isnan(X[:, :, s0]).all()
            continue
        n += 1
        for k in range(K):
            fwd = sum(o.W[k, 0, win[j], j] for j in range(M)) + o.b[0, k]
            rev = sum(o.W[k, 0, 3 - win[j], M - 1 - j] for j in range(M)) + o.b[0, k]
            for s, x in enumerate([fwd, rev] if ds else [fwd + rev]):
                assert abs(X[s, k, s0] - x) < 1e-12
                t = (x - lo) * nbins / (hi - lo)
                want[k, s, 0 if t < 0 else nbins - 1 if t >= nbins else int(t)] += 1
    assert n == valid.sum() and 0 < n < valid.size
    got = H.reference_counts(X, valid, lo, hi, nbins)
    assert np.array_equal(got, want)
    assert want[:, :, 0].sum() > 0                                  # the clamp below lo is exercised
    # sigmoid of the log-odds is the probability the scan's yardstick reports
    P, v2 = stream_scores(o, stream)
    assert np.array_equal(valid, v2)
    np.testing.assert_allclose(1.0 / (1.0 + np.exp(-X[:, :, valid])), P[:, :, valid], rtol=1e-12)


def test_check_histogram_accepts_the_exact_counts_and_refuses_wrong_ones():
    o = harness.random_model(6, 7, True, 8)
    stream = _stream(700, 2, gaps=(0, 63, 64, 300, 699))
    lo, hi, nbins = -8.0, 8.0, 64
    X, valid = H.stream_logodds(o, stream)
    counts = H.reference_counts(X, valid, lo, hi, nbins)
    n = int(valid.sum())
    assert H.check_histogram(counts, n, X, valid, lo, hi, nbins) <= 0.01
    k, s = 2, 1
    j = int(np.argmax(counts[k, s, 1:-1])) + 1
    moved = counts.copy()                                           # a score two bins away from where it belongs
    moved[k, s, j] -= 1
    moved[k, s, min(j + 2, nbins - 1)] += 1
    with pytest.raises(AssertionError, match="tail outside"):
        H.check_histogram(moved, n, X, valid, lo, hi, nbins)
    lost = counts.copy()
    lost[k, s, j] -= 1
    with pytest.raises(AssertionError, match="row totals"):
        H.check_histogram(lost, n, X, valid, lo, hi, nbins)
    twice = counts.copy()
    twice[k] *= 2                                                   # a motif two slabs both counted
    with pytest.raises(AssertionError, match="row totals"):
        H.check_histogram(twice, n, X, valid, lo, hi, nbins)
    with pytest.raises(AssertionError):
        H.check_histogram(counts, n + 1, X, valid, lo, hi, nbins)
    with pytest.raises(AssertionError, match="inside the bands"):    # bands that swallow the data are an input error
        H.check_histogram(counts, n, X, valid, lo, hi, nbins, rtol=0.05)


@pytest.mark.parametrize("K,M,ds", [(10, 15, True), (20, 15, True), (300, 10, False), (257, 1, False)])
def test_the_shapes_of_the_gpu_cases_meet_the_input_condition(K, M, ds):
    """reference alone, harness.random_model of each shape over a 5003-letter stream with gaps, lo = -8, hi = 8, 64 bins:
    at most 1 % of the scores inside the bands, scores below lo (the clamp is exercised)"""
    o = harness.random_model(K, M, ds, K + M)
    rng = np.random.default_rng(2031)
    stream = rng.integers(0, 4, size=5003, dtype=np.uint8)
    for a in rng.integers(0, 5003 - 25, size=2):
        stream[a:a + 25] = 4
    X, valid = H.stream_logodds(o, stream)
    counts = H.reference_counts(X, valid, -8.0, 8.0, 64)
    share = H.check_histogram(counts, int(valid.sum()), X, valid, -8.0, 8.0, 64)
    print("%d x %d: %.2f %% of the scores inside the bands, %d below lo, %d at or above hi"
          % (K, M, 100 * share, counts[:, :, 0].sum(), (X[:, :, valid] >= 8.0).sum()))
    assert share <= 0.01
