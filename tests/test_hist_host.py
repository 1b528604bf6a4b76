"""CPU-only tests of the calibration surface: the declaration of crbm_scan_histogram_codes and its refusal of a null
handle, CRBM.scoreHistogram's argument checks (all before the C side), calibrate.ScoreHistogram on hand-made counts
(tail, thresholds with an unresolved motif, p-values with prob 0 and 1 and the strand mapping, +, save / load) and
sequences.shuffleStream."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_abi_declares_the_histogram_entry_point():
    import crbm_amd
    from crbm_amd import _lib
    header = open(os.path.join(ROOT, "include", "crbm_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    decl = re.search(r"\bint crbm_scan_histogram_codes\((.*?)\);", code, flags=re.S)
    assert decl, "crbm_scan_histogram_codes is not declared"
    assert [a.strip() for a in decl.group(1).split(",")] == [
        "crbm_handle* h", "const uint8_t* codes", "int64_t T", "float lo", "float hi", "int32_t nbins", "uint64_t* counts",
        "int64_t* windows"]
    doc = header[header.index("score histogram"):header.index("int crbm_scan_histogram_codes(")]
    for word in ("log-odds", "bin rule", "first bin", "last", "== *windows exactly", "CRBM_ERR_INVALID", "1024"):
        assert word in doc, word
    lib = _lib.load()
    assert lib.crbm_scan_histogram_codes.argtypes == _lib.SIGNATURES["crbm_scan_histogram_codes"][1]
    codes = np.zeros(8, np.uint8)
    counts = np.zeros(64, np.uint64)
    windows = ctypes.c_int64(-1)
    assert lib.crbm_scan_histogram_codes(None, codes.ctypes.data_as(_lib._U8P), 8, -1.0, 1.0, 4,
                                         counts.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), ctypes.byref(windows)) == _lib.ERR_INVALID
    for name in ("ScoreHistogram", "shuffleStream"):
        assert hasattr(crbm_amd, name)
    assert hasattr(crbm_amd.CRBM, "scoreHistogram")


def _model(monkeypatch):
    """the stub of tests/test_scan_host.py: no GPU here, the checks must fire before any call"""
    from crbm_amd import CRBM
    m = CRBM(3, 4, batchsize=8, fantasy_hidden_len=10, seed=1)
    monkeypatch.setattr(m, "_h", lambda: None)
    monkeypatch.setattr(m, "_call", lambda *a: (_ for _ in ()).throw(AssertionError("reached the library")))
    return m


def test_score_histogram_refuses_bad_arguments_before_the_c_side(monkeypatch):
    m = _model(monkeypatch)
    good = np.array([0, 1, 2, 3, 4, 0, 1, 2, 3], np.uint8)
    with pytest.raises(ValueError, match="uint8"):
        m.scoreHistogram(good.astype(np.int32))
    with pytest.raises(ValueError, match="one-dimensional"):
        m.scoreHistogram(good.reshape(3, 3))
    with pytest.raises(ValueError, match="0..4"):
        m.scoreHistogram(np.array([0, 1, 5, 2], np.uint8))
    with pytest.raises(ValueError, match="start at 0 and ascend"):
        m.scoreHistogram(good, offsets=[1, 5, 10])
    with pytest.raises(ValueError, match="separated by a code 4"):
        m.scoreHistogram(good, offsets=[0, 4, 10])
    for bins in (0, 1025, -3, 2.5, "64", True, None):
        with pytest.raises(ValueError, match="bins must be"):
            m.scoreHistogram(good, bins=bins)
    for lo, hi in ((1.0, 1.0), (2.0, -2.0), (float("nan"), 1.0), (-1.0, float("inf")), (-1e39, 1.0), (0.0, 1e-50)):
        with pytest.raises(ValueError, match="finite with lo < hi"):
            m.scoreHistogram(good, lo=lo, hi=hi)
    with pytest.raises(ValueError, match="must be numbers"):
        m.scoreHistogram(good, lo="low")
    with pytest.raises(AssertionError, match="reached the library"):      # and a good call gets that far
        m.scoreHistogram(good, bins=1024, lo=-3, hi=3, offsets=[0, 5, 10])
    with pytest.raises(AssertionError, match="reached the library"):
        m.scoreHistogram(good)


def test_score_histogram_cuts_long_streams_and_sums_the_pieces(monkeypatch):
    from crbm_amd import CRBM, seqsToStream
    m = CRBM(3, 4, batchsize=8, fantasy_hidden_len=10, seed=1)
    stream, offsets, _ = seqsToStream(["ACGTA", "CCCCC", "GG", "TTTTTTTT", "ACGTACGTACG"])
    monkeypatch.setattr(CRBM, "_SCAN_MAX", 12)
    sizes = []

    def fake(piece, lo, hi, bins):                         # every letter a "window" in bin 1
        assert (lo, hi, bins) == (-2.0, 2.0, 4)
        sizes.append(piece.size)
        c = np.zeros((3, 2, 4), np.uint64)
        c[:, :, 1] = int((piece < 4).sum())
        return c, int((piece < 4).sum())
    monkeypatch.setattr(m, "_hist_call", fake)
    h = m.scoreHistogram(stream, bins=4, lo=-2, hi=2, offsets=offsets)
    assert sizes == [11, 11, 11]
    assert h.windows == int((stream < 4).sum()) and np.all(h.counts[:, :, 1] == h.windows) and h.counts.dtype == np.int64
    assert h.edges.tolist() == [-2.0, -1.0, 0.0, 1.0, 2.0] and h.doublestranded is True
    with pytest.raises(ValueError, match="needs offsets"):
        m.scoreHistogram(stream, bins=4)


def _hist():
    from crbm_amd import ScoreHistogram
    counts = np.zeros((3, 2, 8), np.int64)                  # bins of width 1 over [-4, 4): 1000 windows
    counts[0, 0] = [900, 50, 30, 10, 5, 3, 1, 1]
    counts[0, 1] = [0, 0, 0, 0, 0, 0, 0, 1000]              # everything at or above 3: never resolved
    counts[1, 0] = [1000, 0, 0, 0, 0, 0, 0, 0]
    counts[1, 1] = [990, 0, 0, 0, 0, 0, 10, 0]
    counts[2, 0] = [0, 0, 0, 0, 980, 10, 0, 10]
    counts[2, 1] = [100, 100, 100, 100, 200, 200, 100, 100]
    return ScoreHistogram(counts, np.linspace(-4, 4, 9), 1000, True)


def test_tail_thresholds_and_the_unresolved_motif():
    h = _hist()
    tail = h.tail()
    assert tail.shape == (3, 2, 8) and np.all(tail[:, :, 0] == 1000)
    assert tail[0, 0].tolist() == [1000, 100, 50, 20, 10, 5, 2, 1]
    thr, resolved = h.thresholds(0.01)
    assert thr.dtype == np.float32 and thr.shape == (3, 2) and resolved.dtype == bool
    sig = lambda x: 1.0 / (1.0 + np.exp(-x))
    up = lambda e: np.nextafter(np.float32(sig(e)), np.float32(1))
    assert resolved.tolist() == [[True, False], [True, True], [True, False]]
    assert thr[0, 0] == up(0.0)                              # tail[4] = 10 <= 10: edge 0
    assert thr[0, 1] == 1.0 and thr[2, 1] == 1.0             # even the last bin holds more than 10
    assert thr[1, 0] == up(-3.0)                             # nothing above the first bin: its upper edge
    assert thr[1, 1] == up(-3.0)                             # tail[1] = 10
    assert thr[2, 0] == up(2.0)                              # tail[6] = 10
    assert np.float32(sig(2.0)) <= thr[2, 0] < 1.0
    thr1, res1 = h.thresholds(1.0)                           # everything passes: the first bin is open below
    assert res1.all() and np.all(thr1 == 0.0)
    thr0, res0 = h.thresholds(0.0)
    assert res0.tolist() == [[False, False], [True, True], [False, False]] and thr0[1, 0] == up(-3.0) and thr0[1, 1] == up(3.0)
    for bad in (-0.1, 1.1, float("nan"), "x"):
        with pytest.raises(ValueError, match="fpr"):
            h.thresholds(bad)


def test_pvalues_prob_0_and_1_and_the_strand_mapping():
    from crbm_amd import CRBM
    h = _hist()
    sig = lambda x: 1.0 / (1.0 + np.exp(-x))
    sites = np.zeros(7, CRBM.SITE_DTYPE)
    sites["motif"] = [0, 0, 0, 0, 2, 2, 0]
    sites["strand"] = [1, 1, 1, -1, 1, -1, 0]
    sites["prob"] = [0.0, 1.0, sig(0.5), sig(0.5), sig(-0.5), sig(-2.5), sig(2.5)]
    p = h.pvalues(sites)
    assert p.dtype == np.float64
    want = [1001, 2, 11, 1001, 1001, 901, 3]                 # tail + 1; strand -1 reads s = 1, +1 and 0 read s = 0
    np.testing.assert_allclose(p, np.array(want) / 1001.0, rtol=1e-15)
    assert h.bin_of([-np.inf, np.inf, -4.0, 3.999, 4.0, -4.0001, 0.0]).tolist() == [0, 7, 0, 7, 7, 0, 4]
    from crbm_amd import ScoreHistogram
    ss = ScoreHistogram(h.counts[:, :1], h.edges, 1000, False)
    with pytest.raises(ValueError, match="double-stranded"):
        ss.pvalues(sites)
    assert ss.pvalues(sites[[0, 6]]).tolist() == [1.0, 3 / 1001.0]


def test_add_save_load_and_the_constructor_checks(tmp_path):
    from crbm_amd import ScoreHistogram
    h = _hist()
    two = h + h
    assert two.windows == 2000 and np.array_equal(two.counts, 2 * h.counts) and np.array_equal(two.edges, h.edges)
    assert np.array_equal(h.counts, _hist().counts)          # + leaves its operands alone
    with pytest.raises(ValueError, match="different binning"):
        h + ScoreHistogram(h.counts, np.linspace(-4, 5, 9), 1000, True)
    with pytest.raises(ValueError, match="different binning"):
        h + ScoreHistogram(h.counts[:2], h.edges, 1000, True)
    with pytest.raises(ValueError, match="different binning"):
        ScoreHistogram(h.counts[:, :1], h.edges, 1000, False) + ScoreHistogram(h.counts[:, :1, :4].copy() * 0 + 250, h.edges[:5], 1000, False)
    path = str(tmp_path / "background.npz")
    h.save(path)
    back = ScoreHistogram.load(path)
    assert np.array_equal(back.counts, h.counts) and back.counts.dtype == np.int64
    assert np.array_equal(back.edges, h.edges) and back.windows == 1000 and back.doublestranded is True
    with pytest.raises(ValueError, match="sum to windows"):
        ScoreHistogram(h.counts, h.edges, 999, True)
    with pytest.raises(ValueError, match="S = 2"):
        ScoreHistogram(h.counts, h.edges, 1000, False)
    with pytest.raises(ValueError, match="edges"):
        ScoreHistogram(h.counts, h.edges[:-1], 1000, True)
    empty = ScoreHistogram(np.zeros((2, 1, 4), np.int64), np.linspace(0, 1, 5), 0, False)
    with pytest.raises(ValueError, match="empty"):
        empty.thresholds(0.01)


def test_shuffle_stream():
    from crbm_amd import shuffleStream, seqsToStream
    rng = np.random.default_rng(3)
    stream = rng.integers(0, 4, size=5000, dtype=np.uint8)
    for a in (0, 17, 18, 19, 700, 4999):
        stream[a] = 4
    stream[2000:2100] = 4
    before = stream.copy()
    out = shuffleStream(stream, 7)
    assert np.array_equal(stream, before)                              # the input is left alone
    assert out.dtype == np.uint8 and out.shape == stream.shape
    assert np.array_equal(out == 4, stream == 4)                       # codes 4 stay where they are
    edges = np.flatnonzero(np.diff(np.concatenate(([True], stream == 4, [True])).astype(np.int8)))
    runs = list(zip(edges[::2], edges[1::2]))
    assert len(runs) == 4 and sum(b - a for a, b in runs) == int((stream < 4).sum())
    for a, b in runs:                                                  # every maximal run keeps its composition
        assert np.array_equal(np.bincount(out[a:b], minlength=4), np.bincount(stream[a:b], minlength=4))
    assert not np.array_equal(out, stream)
    assert np.array_equal(out, shuffleStream(stream, 7))               # deterministic per seed
    assert not np.array_equal(out, shuffleStream(stream, 8))           # and different across seeds
    s2, offsets, _ = seqsToStream(["ACGTNACGT", "", "GGGGC", "T"])
    o2 = shuffleStream(s2, 1)
    assert np.array_equal(o2 == 4, s2 == 4) and o2[-1] == 3            # record boundaries kept; a run of one letter
    assert shuffleStream(np.zeros(0, np.uint8), 1).size == 0
    assert np.array_equal(shuffleStream(np.full(9, 4, np.uint8), 1), np.full(9, 4, np.uint8))
    with pytest.raises(ValueError, match="uint8"):
        shuffleStream([0, 1, 2], 1)
