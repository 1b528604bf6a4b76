"""Pins tests/compare_reference.py, the yardstick of the motif comparison: the tails against a brute-force enumeration
of all C^l tuples of pool columns as exact fractions; every pmf sums to 1 within l (B + 1) 2^-53 (a cell of length l is a
sum of at most B products per convolution, the whole a sum of sums: the bound counts one rounding per product and add
along the longest chain, generously); the quantisation and bin rules at their edges; and the three cases a user checks
first: a query cut out of a target, a reverse-complemented target, a palindrome."""
from fractions import Fraction

import numpy as np
import pytest

from tests import compare_reference as R


def motifs_of(widths, seed):
    rng = np.random.default_rng(seed)
    return [R.quantise(R.dirichlet_motif(rng, w)) for w in widths]


def test_quantise_and_bins_at_the_edges():
    p = np.array([[1.0, 0.0, 0.25, 0.5 / 4096], [0.0, 1.0, 0.25, 1.49 / 4096], [0.0, 0.0, 0.25, 0.0], [0.0, 0.0, 0.25, 1.0]])
    q = R.quantise(p)
    assert q.dtype == np.uint16 and q.shape == (4, 4)
    assert q[0].tolist() == [4096, 0, 0, 0] and q[2].tolist() == [1024] * 4 and q[3].tolist() == [1, 1, 0, 4096]
    assert R.reverse_complement(q)[0].tolist() == [4096, 0, 1, 1] and R.reverse_complement(q)[3].tolist() == [0, 0, 0, 4096]
    for B in (2, 100, 256):
        b = R.bins_of(q[:2], q[:2], B)
        assert b[0, 0] == b[1, 1] == B - 1 and b[0, 1] == b[1, 0] == 0         # D = 0 and D = 2^25, the two ends
        every = R.bins_of(q, np.array([[4096, 4096, 4096, 4096], [0, 0, 0, 0]], np.uint16), B)   # D up to 2^26: clipped
        assert every.min() >= 0 and every.max() < B
    # the rounding of the bin rule: sim (B - 1) / 2^25 rounded half up
    a, b = np.array([[2048, 2048, 0, 0]], np.uint16), np.array([[2048, 0, 2048, 0]], np.uint16)       # D = 2^23
    assert R.bins_of(a, b, 100)[0, 0] == int(np.floor((2 ** 25 - 2 ** 23) * 99 / 2 ** 25 + 0.5))


@pytest.mark.parametrize("C,both", [(6, False), (3, True), (5, False)])
def test_tails_against_brute_force(C, both):
    """m = 3, B = 7: every (i, l) against the enumeration of all C^l tuples, within 1e-13 relative"""
    B = 7
    query = motifs_of([3], 10 + C)[0]
    targets = motifs_of([C // 2, C - C // 2], 20 + C)
    pool = R.pool_of(targets, both)
    assert len(pool) == C * (2 if both else 1) <= 6
    counts = R.counts_of(query, pool, B)
    assert np.all(counts.sum(axis=1) == len(pool))
    tails = R.tails_of(counts, 1.0 / len(pool))
    assert sorted(tails) == [(0, 1), (0, 2), (0, 3), (1, 1), (1, 2), (2, 1)]
    for (i, l), tail in tails.items():
        want = R.brute_force_tails(query, pool, B, i, l)
        assert len(tail) == len(want) == l * (B - 1) + 2 and tail[-1] == 0.0
        for got, w in zip(tail, want):
            assert abs(Fraction(float(got)) - w) <= Fraction(1, 10 ** 13) * w, (i, l)
            assert (got == 0.0) == (w == 0)


def test_every_pmf_sums_to_one():
    for B, m, seed in ((100, 12, 1), (256, 6, 2), (2, 20, 3)):
        query = motifs_of([m], seed)[0]
        pool = R.pool_of(motifs_of((8, 13, 20, 9, 15, 6), seed + 50), True)
        pmfs = R.pmfs_of(R.counts_of(query, pool, B), 1.0 / len(pool))
        for (i, l), pmf in pmfs.items():
            assert pmf.size == l * (B - 1) + 1 and pmf.min() >= 0.0
            assert abs(float(sum(Fraction(float(v)) for v in pmf) - 1)) <= l * (B + 1) * 2.0 ** -53, (B, i, l)


@pytest.fixture(scope="module")
def library():
    return motifs_of(np.random.default_rng(0).integers(6, 21, size=40), 99)


def test_a_cut_out_query_finds_its_target(library):
    k = next(i for i, t in enumerate(library) if i > 10 and len(t) >= 10)
    target = library[k]
    query = target[2:8]
    out = R.compare([query], library, bins=100, both=True)
    order = np.argsort(out["p_min"][0])
    assert order[0] == k and out["offset"][0, k] == -2 and out["strand"][0, k] == 1 and out["overlap"][0, k] == 6
    assert out["p_min"][0, k] < 1e-9 and out["p_min"][0, order[1]] > 1e3 * out["p_min"][0, k]
    assert out["n_off"][0, k] == 2 * (6 + len(target) - 1)
    pvalue, evalue, qvalue = R.derive(out["p_min"], out["n_off"])
    assert np.all(pvalue >= out["p_min"] * (1 - 1e-12)) and np.all(pvalue <= out["p_min"] * out["n_off"] * (1 + 1e-12))
    assert np.allclose(evalue, pvalue * 40) and np.all(qvalue >= pvalue * (1 - 1e-15)) and np.all(qvalue <= 1.0)
    assert np.argmin(qvalue[0]) == k


def test_a_reverse_complemented_target_is_found_on_strand_minus(library):
    k = 5
    query = R.reverse_complement(library[k])
    out = R.compare([query], library, bins=100, both=True)
    assert np.argmin(out["p_min"][0]) == k and out["strand"][0, k] == -1 and out["offset"][0, k] == 0 and out["overlap"][0, k] == len(query)
    given = R.compare([query], library, bins=100, both=False)
    assert np.all(given["strand"] == 1) and given["p_min"][0, k] > 1e6 * out["p_min"][0, k]
    assert np.array_equal(given["n_off"] * 2, out["n_off"])


def test_a_palindrome_goes_to_strand_plus(library):
    half = library[3][:5]
    pal = np.concatenate([half, R.reverse_complement(half)])
    assert np.array_equal(R.reverse_complement(pal), pal)
    out = R.compare([pal], library[:10] + [pal], bins=100, both=True)
    assert np.argmin(out["p_min"][0]) == 10 and out["strand"][0, 10] == 1 and out["offset"][0, 10] == 0


def test_min_overlap_and_p_of_one():
    queries, targets = motifs_of((4, 9), 7), motifs_of((3, 12, 9), 8)
    for need in (1, 5, 100):
        out = R.compare(queries, targets, bins=20, both=True, min_overlap=need)
        for k, m in enumerate((4, 9)):
            for t, n in enumerate((3, 12, 9)):
                lim = min(need, m, n)
                assert out["n_off"][k, t] == 2 * (m + n - 1 - 2 * (lim - 1)) and out["overlap"][k, t] >= lim
    pvalue, _, _ = R.derive(np.array([[1.0, 0.5, 0.0]]), np.array([[3, 2, 7]]))
    assert pvalue[0, 0] == 1.0 and abs(pvalue[0, 1] - 0.75) < 1e-15 and pvalue[0, 2] == 0.0


def test_benjamini_hochberg_by_hand():
    p = np.array([0.01, 0.04, 0.03, 0.5])
    # ranked: 0.01 (1), 0.03 (2), 0.04 (3), 0.5 (4) -> 0.04, 0.06, 0.0533.., 0.5 -> monotone from the right
    want = [0.04, 0.04 * 4 / 3, 0.04 * 4 / 3, 0.5]
    assert np.allclose(R.benjamini_hochberg(p), want, rtol=1e-15)
