"""Pins the yardstick of the record summaries (tests/record_reference.py) on the CPU: on equal-length N-free records
fe == L * oracle.freeEnergy and per_motif is the oracle's per-motif term with the visible bias taken out; the best site
is the argmax of scan_reference.reference_sites at threshold 0; rows of A ++ [4] ++ B are the rows of A followed by the
rows of B; and the input condition of the best-site rule -- at most 1 % ambiguous cells -- holds for
harness.random_model at the shapes the emulation and GPU tests use, with exact ties present where motifs are short."""
import numpy as np
import pytest

from oracle.crbm_oracle import onehot_of
from tests.emu import harness
from tests import record_reference as rr
from tests.scan_reference import reference_sites

SHAPES = [(10, 15, True, 25), (20, 15, True, 35), (10, 5, False, 15), (36, 6, False, 42), (6, 1, True, 7)]


@pytest.mark.parametrize("K,M,ds,seed", SHAPES[:3])
def test_equal_length_records_against_the_oracle(K, M, ds, seed):
    o = harness.random_model(K, M, ds, seed, draw_c=True)
    codes = np.random.default_rng(3).integers(0, 4, size=(12, 50), dtype=np.uint8)
    stream, offsets = rr.make_stream(list(codes))
    ref = rr.record_summary(o, stream, offsets)
    D = onehot_of(codes)
    np.testing.assert_allclose(ref["fe"], 50 * o.freeEnergy(D), rtol=1e-12)
    bias = (D * o.c.reshape(1, 1, -1, 1)).sum(axis=(1, 2, 3))
    np.testing.assert_allclose(ref["per_motif"], o.freeEnergy(D, permotif=True) + bias[:, None], rtol=1e-12)
    assert np.all(ref["windows"] == 50 - M + 1) and np.all(ref["letters"].sum(axis=1) == 50)
    for r in range(12):
        assert ref["letters"][r].tolist() == np.bincount(codes[r], minlength=4).tolist()


@pytest.mark.parametrize("K,M,ds,seed", SHAPES)
def test_best_site_is_the_argmax_of_the_scan_reference(K, M, ds, seed):
    o = harness.random_model(K, M, ds, seed)
    stream, offsets = rr.record_stream(2031, M)
    ref = rr.record_summary(o, stream, offsets)
    assert ref["windows"].sum() == ref["valid"].sum()
    sites = reference_sites(o, stream, 0.0)
    seq = np.searchsorted(offsets, sites["start"], side="right") - 1
    rel = sites["start"] - offsets[seq]
    for r in range(offsets.size - 1):
        mine = seq == r
        assert mine.sum() == ref["windows"][r] * K * (2 if ds else 1)
        for k in range(K):
            cell = mine & (sites["motif"] == k)
            if not cell.any():
                assert ref["start"][r, k] == -1 and ref["prob"][r, k] == 0.0 and ref["strand"][r, k] == 0
                continue
            p = sites["prob"][cell]
            i = np.flatnonzero(p == p.max())[0]              # sorted by (start, strand), + before -: the first maximum
            assert (ref["start"][r, k], ref["strand"][r, k], ref["prob"][r, k]) == (rel[cell][i], sites["strand"][cell][i], p[i])


def test_rows_of_a_concatenation():
    o = harness.random_model(10, 15, True, 25, draw_c=True)
    stream, offsets = rr.record_stream(2031, 15)
    recs = rr.split_records(stream, offsets)
    assert len(recs) == 50 and [len(r) for r in recs[:9]] == [0, 0, 1, 14, 15, 16, 63, 64, 65] and len(recs[-1]) == 1500
    assert 9000 < stream.size < 13000
    gapped = [r for r in recs if len(r) > 60 and (r > 3).any()]
    assert 10 <= len(gapped) <= 30 and all(1 <= (r > 3).sum() <= 4 for r in gapped)
    whole = rr.record_summary(o, stream, offsets)
    a, b = rr.record_summary(o, *rr.make_stream(recs[:20])), rr.record_summary(o, *rr.make_stream(recs[20:]))
    for k in ("windows", "letters", "per_motif", "fe", "start", "strand", "prob"):
        assert np.array_equal(whole[k], np.concatenate([a[k], b[k]])), k


@pytest.mark.parametrize("K,M,ds,seed", SHAPES)
def test_input_condition_of_the_best_site_rule(K, M, ds, seed):
    """the reference's own answer passes check_best at the GPU tests' RTOL with at most 1 % ambiguous cells, no
    saturated probability, and the tie rule is exercised by the short motifs"""
    o = harness.random_model(K, M, ds, seed)
    stream, offsets = rr.record_stream(2031, M)
    ref = rr.record_summary(o, stream, offsets)
    amb, cells, ties, mirror = rr.check_best(ref, ref, 2e-5, "%dx%d" % (K, M))
    print("%d x %d: %d of %d cells ambiguous, %d exact ties, %d mirror ties" % (K, M, amb, cells, ties, mirror))
    assert cells == (ref["windows"] > 0).sum() * K and amb <= 0.01 * cells
    assert ref["prob"][ref["windows"] > 0].max() < 1.0
    if M <= 5:
        assert ties > 20
    unit = 2.0 ** -20
    rr.check_fe(ref, ref, 2e-5, unit)
    off = dict(ref, per_motif=ref["per_motif"] + (ref["windows"][:, None] > 0) * 3e-4 * np.abs(ref["per_motif"]).max())
    with pytest.raises(AssertionError):                      # and the bound is no formality
        rr.check_fe(off, ref, 2e-5, unit)
