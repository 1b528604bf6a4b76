"""The score histogram (CRBM.scoreHistogram, crbm_scan_histogram_codes) on the GPU: against the float64 reference of
tests/hist_reference.py (exact row totals, tails inside the RTOL bands of the edges) on specialised and slabbed model
classes of test_gpu_sweeps; the same bits for every CRBM_SLAB_BYTES and run; additivity over a gap and the windows a
gap removes; a second binning; the use case (thresholds for a false-positive rate against scanSites' records, p-values);
the refusals, a bad code in the first and in the last of several segments among them (scanSites too: the stream
sweep's shared epilogue); and 2^22 letters on config #2's double-stranded model."""
import ctypes

import numpy as np
import pytest

from tests.test_gpu_parity import make_pair, RTOL
from tests.test_gpu_sweeps import CLASSES, ids, _model
from tests.test_gpu_scan import gapped_stream, per_start, _c_scan, _threshold, _same as _same_sites
from tests.scan_reference import window_valid
from tests.hist_reference import stream_logodds, check_histogram

pytestmark = pytest.mark.gpu

SERVED = [CLASSES[0], CLASSES[1], CLASSES[2], CLASSES[3]]   # 10 x 15 ds, 20 x 15 ds, 300 x 10 (five slabs), 257 x 1 (last slab moved back)
T_A, SEED = 5003, 2031
LO, HI, BINS = -8.0, 8.0, 64


def _same(a, b):
    assert a.windows == b.windows and a.doublestranded == b.doublestranded
    assert np.array_equal(a.edges, b.edges) and np.array_equal(a.counts, b.counts)


@pytest.mark.parametrize("cls", SERVED, ids=ids(SERVED))
def test_histogram_against_reference_and_the_same_bits_for_every_segmenting(cls, monkeypatch):
    """(a) check_histogram: every row sums to the valid windows exactly (a motif two slabs both counted would break
    it: 257 x 1 runs as slabs of 60 whose last is moved back over its neighbour); every tail lies between the
    reference's tails at the edge +- RTOL max(1, |edge|); at most 1 % of the reference's scores lie inside the bands.
    Stream gapped_stream(5003, 2031), lo = -8, hi = 8, 64 bins.  Shares inside the bands, reference alone on the CPU,
    for this test's own models: 0.32 %, 0.30 %, 0.19 %, 0.20 % (harness.random_model models of these shapes,
    tests/test_hist_reference.py: 0.29 %, 0.32 %, 0.16 %, 0.20 %); 26 511, 42 390, 843 841 and 0 scores fall below lo
    (the clamp is exercised), 0, 0, 3 and 0 at or above hi.  The run prints its own figures.
    (b) the same bits for the default CRBM_SLAB_BYTES (one segment), one that gives 7 segments, one whose segment
    edge falls inside a window, and a second run."""
    name, K, M, ds, A, pool, Lf, L, env, spec = cls
    m, o = _model(cls, monkeypatch)
    stream = gapped_stream(T_A, SEED)
    X, valid = stream_logodds(o, stream)
    monkeypatch.delenv("CRBM_SLAB_BYTES", raising=False)
    h = m.scoreHistogram(stream, bins=BINS, lo=LO, hi=HI)
    assert h.counts.shape == (K, 2 if ds else 1, BINS) and h.doublestranded == ds
    share = check_histogram(h.counts, h.windows, X, valid, LO, HI, BINS, rtol=RTOL)
    print("%s: %.2f %% of the reference's scores inside the bands, %d below lo, %d at or above hi"
          % (name, 100 * share, h.counts[:, :, 0].sum(), (X[:, :, valid] >= HI).sum()))
    _same(h, m.scoreHistogram(stream, bins=BINS, lo=LO, hi=HI))
    starts = T_A - M + 1
    monkeypatch.setenv("CRBM_SLAB_BYTES", str(per_start(cls) * (starts // 7 + 1)))
    _same(h, m.scoreHistogram(stream, bins=BINS, lo=LO, hi=HI))
    edge = 2500 + max(1, M // 2)
    monkeypatch.setenv("CRBM_SLAB_BYTES", str(per_start(cls) * edge))
    _same(h, m.scoreHistogram(stream, bins=BINS, lo=LO, hi=HI))


@pytest.mark.parametrize("cls", [CLASSES[0], CLASSES[2]], ids=ids([CLASSES[0], CLASSES[2]]))
def test_histogram_additivity_gaps_and_a_second_binning(cls, monkeypatch):
    """(c) hist(A ++ [4] ++ B) == hist(A) + hist(B) bit for bit; a code 4 at one position lowers every row's total by
    exactly the number of valid windows that covered it; 1024 bins over [-16, 16) have exact row totals, and their
    16-to-1 re-binning to 64 bins passes check_histogram (held to the reference, not to equality with a 64-bin run: a
    score within rounding of an edge may part ways)"""
    name, K, M, ds, A, pool, Lf, L, env, spec = cls
    m, o = _model(cls, monkeypatch)
    monkeypatch.delenv("CRBM_SLAB_BYTES", raising=False)
    a, b = gapped_stream(1777, 11), gapped_stream(2100, 12)
    a[0] = a[-1] = b[0] = b[-1] = 1                              # letters at the joint: only the separator parts them
    joined = np.concatenate([a, np.array([4], np.uint8), b])
    hj = m.scoreHistogram(joined, bins=BINS, lo=LO, hi=HI)
    _same(hj, m.scoreHistogram(a, bins=BINS, lo=LO, hi=HI) + m.scoreHistogram(b, bins=BINS, lo=LO, hi=HI))
    valid = window_valid(joined, M)
    p = int(np.flatnonzero(valid)[valid.sum() // 2]) + M // 3
    covered = int(valid[max(0, p - M + 1):p + 1].sum())
    assert covered > 0
    gap = joined.copy()
    gap[p] = 4
    hg = m.scoreHistogram(gap, bins=BINS, lo=LO, hi=HI)
    assert hg.windows == hj.windows - covered and np.all(hg.counts.sum(axis=2) == hj.windows - covered)
    X, valid = stream_logodds(o, joined)
    fine = m.scoreHistogram(joined, bins=1024, lo=-16.0, hi=16.0)
    assert fine.windows == int(valid.sum()) and np.all(fine.counts.sum(axis=2) == fine.windows)
    # bins of 1/32 are only some 25 bands wide where the scores lie: about 4 % of the reference's scores sit inside a band
    # (reference alone, on the CPU), so the input condition of the 1 % cap cannot hold here and the tails are checked without it
    check_histogram(fine.counts, fine.windows, X, valid, -16.0, 16.0, 1024, rtol=RTOL, band_share=1.0)
    S = 2 if ds else 1
    check_histogram(fine.counts.reshape(K, S, 64, 16).sum(axis=3), fine.windows, X, valid, -16.0, 16.0, 64, rtol=RTOL)


@pytest.mark.parametrize("cls", [CLASSES[0], CLASSES[2]], ids=ids([CLASSES[0], CLASSES[2]]))
def test_thresholds_for_a_false_positive_rate_against_scan_sites(cls, monkeypatch):
    """(d) fpr = 0.01: for every resolved (motif, strand) with threshold bin j, the scanSites records of that motif and
    strand at or above thr[motif, strand] number between tail[j + 1] and tail[j - 1] (one bin of slack covers fp32
    rounding at the edge), and their p-values are all at most (tail[j - 1] + 1) / (windows + 1).  The records come
    from one scanSites call at the smallest threshold, filtered on the host as the README shows."""
    name, K, M, ds, A, pool, Lf, L, env, spec = cls
    m, o = _model(cls, monkeypatch)
    monkeypatch.delenv("CRBM_SLAB_BYTES", raising=False)
    stream = gapped_stream(T_A, SEED)
    h = m.scoreHistogram(stream, bins=BINS, lo=LO, hi=HI)
    thr, resolved = h.thresholds(0.01)
    assert resolved.any()
    j, _ = h._tail_bin(0.01)
    tail = np.concatenate([np.full(h.counts.shape[:2] + (1,), h.windows), h.tail(), np.zeros(h.counts.shape[:2] + (1,), np.int64)], axis=2)
    sites = m.scanSites(stream, float(thr[resolved].min()))
    s = np.where(sites["strand"] == -1, 1, 0)
    sites, s = sites[sites["prob"] >= thr[sites["motif"], s]], s[sites["prob"] >= thr[sites["motif"], s]]
    n = np.zeros(h.counts.shape[:2], np.int64)
    np.add.at(n, (sites["motif"], s), 1)
    hi_tail = np.take_along_axis(tail, j[:, :, None], axis=2)[:, :, 0]          # tail[j - 1] (the padded array is shifted by one)
    lo_tail = np.take_along_axis(tail, j[:, :, None] + 2, axis=2)[:, :, 0]      # tail[j + 1]
    ok = (lo_tail <= n) & (n <= hi_tail)
    assert np.all(ok[resolved]), (np.argwhere(~ok & resolved)[:5].tolist(), n[~ok & resolved][:5], j[~ok & resolved][:5])
    assert np.all(thr[~resolved] == 1.0)
    assert sites.size > 0
    assert np.all(h.pvalues(sites) <= (hi_tail[sites["motif"], s] + 1.0) / (h.windows + 1.0))


def test_histogram_refusals_leave_the_handle_usable(monkeypatch):
    """(e) through the raw C entry point: CRBM_ERR_INVALID for pooled, 20-letter and 8 x 100 models, 0 and 1025 bins,
    lo >= hi, a NaN hi, a code 5, a null counts array; the same handle then returns the histogram it returned before;
    T < M gives zeros and windows == 0"""
    from crbm_amd import _lib
    u64 = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))
    ptr = lambda a: a.ctypes.data_as(_lib._U8P)
    stream = gapped_stream(400, 3)
    windows = ctypes.c_int64(-1)
    for cls in (CLASSES[4], CLASSES[7], CLASSES[6]):
        name, K, M, ds, A, pool, Lf, L, env, spec = cls
        m, o = _model(cls, monkeypatch)
        counts = np.zeros((K, 2 if ds else 1, BINS), np.uint64)
        assert m._lib.crbm_scan_histogram_codes(m._h(), ptr(stream), stream.size, LO, HI, BINS, u64(counts), ctypes.byref(windows)) == _lib.ERR_INVALID, name
        with pytest.raises(Exception, match="pooling|alphabet|generic"):
            m.scoreHistogram(stream, bins=BINS, lo=LO, hi=HI)
    m, o = _model(CLASSES[0], monkeypatch)
    good = m.scoreHistogram(stream, bins=BINS, lo=LO, hi=HI)
    lib, h = m._lib, m._h()
    counts = np.full((10, 2, 1025), 77, np.uint64)
    call = lambda st, T, lo, hi, nb, c=counts: lib.crbm_scan_histogram_codes(h, ptr(st), T, lo, hi, nb, u64(c) if c is not None else None, ctypes.byref(windows))
    bad = stream.copy()
    bad[77] = 5
    assert call(stream, stream.size, LO, HI, 0) == _lib.ERR_INVALID
    assert call(stream, stream.size, LO, HI, 1025) == _lib.ERR_INVALID
    assert call(stream, stream.size, 1.0, 1.0, BINS) == _lib.ERR_INVALID
    assert call(stream, stream.size, 2.0, -2.0, BINS) == _lib.ERR_INVALID
    assert call(stream, stream.size, LO, float("nan"), BINS) == _lib.ERR_INVALID
    assert call(stream, stream.size, float("-inf"), HI, BINS) == _lib.ERR_INVALID
    assert call(bad, bad.size, LO, HI, BINS) == _lib.ERR_INVALID
    assert call(stream, -1, LO, HI, BINS) == _lib.ERR_INVALID
    assert call(stream, 2 ** 31, LO, HI, BINS) == _lib.ERR_INVALID
    assert call(stream, stream.size, LO, HI, BINS, None) == _lib.ERR_INVALID
    assert np.all(counts == 77)                                   # a refusal writes nothing
    _same(good, m.scoreHistogram(stream, bins=BINS, lo=LO, hi=HI))
    assert call(stream, 14, LO, HI, BINS) == 0                    # T < M
    assert windows.value == 0 and not counts.ravel()[:10 * 2 * BINS].any() and np.all(counts.ravel()[10 * 2 * BINS:] == 77)
    none = m.scoreHistogram(np.full(200, 4, np.uint8), bins=BINS, lo=LO, hi=HI)
    assert none.windows == 0 and not none.counts.any()


@pytest.mark.parametrize("cls", [CLASSES[0], CLASSES[2]], ids=ids([CLASSES[0], CLASSES[2]]))
def test_a_bad_code_in_any_segment_is_refused_and_the_handle_stays_usable(cls, monkeypatch):
    """(g) the epilogue both stream features share, over 7 segments on two streams (gapped_stream(5003, 2031)): a code
    5 in the last segment, then in the first, makes crbm_scan_sites_codes and crbm_scan_histogram_codes (the C entry
    points: the Python side would refuse first) fail with the "0..4" message, and after every refusal the same handle
    returns, for the clean stream, records and counts equal bit for bit to those from before"""
    from crbm_amd import _lib
    name, K, M, ds, A, pool, Lf, L, env, spec = cls
    m, o = _model(cls, monkeypatch)
    stream = gapped_stream(T_A, SEED)
    _, _, thr = _threshold(o, stream)
    starts = T_A - M + 1
    seg = starts // 7 + 1
    assert -(-starts // seg) == 7
    monkeypatch.setenv("CRBM_SLAB_BYTES", str(per_start(cls) * seg))
    sites = m.scanSites(stream, thr)
    hist = m.scoreHistogram(stream, bins=BINS, lo=LO, hi=HI)
    assert sites.size > 0 and hist.windows > 0
    counts = np.zeros((K, 2 if ds else 1, BINS), np.uint64)
    windows = ctypes.c_int64(-1)
    for p in (T_A - 2, 1):                       # read by the last segment alone; by the first alone
        assert p >= 6 * seg + M - 1 or p < seg
        bad = stream.copy()
        bad[p] = 5
        with pytest.raises(Exception, match=r"0\.\.4"):
            _c_scan(m, bad, thr, sites.size)
        _same_sites(sites, m.scanSites(stream, thr))
        with pytest.raises(Exception, match=r"0\.\.4"):
            m._call("crbm_scan_histogram_codes", bad.ctypes.data_as(_lib._U8P), bad.size, LO, HI, BINS,
                    counts.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), ctypes.byref(windows))
        _same(hist, m.scoreHistogram(stream, bins=BINS, lo=LO, hi=HI))
        _same_sites(sites, m.scanSites(stream, thr))


def test_histogram_scale_cfg2_two_to_the_22():
    """(f) config #2's double-stranded model over 2^22 random letters with gap runs: every row sums to the number of
    valid windows, and the histogram equals the sum of the histograms of its two halves, split at an inserted code 4"""
    K, M = 10, 15
    T = 1 << 22
    m, o = make_pair(K, M, ds=True, Lf=186, bshift=3.0, wscale=0.7)
    stream = gapped_stream(T, 99, share=0.01, run=500)
    half = T // 2
    stream[half - 1] = stream[half + 1] = 2
    stream[half] = 4
    h = m.scoreHistogram(stream, bins=512)
    n = int(window_valid(stream, M).sum())
    assert h.windows == n and np.all(h.counts.sum(axis=2) == n) and h.counts.shape == (K, 2, 512)
    assert (h.counts > 0).sum() > 1000
    _same(h, m.scoreHistogram(stream[:half], bins=512) + m.scoreHistogram(stream[half + 1:], bins=512))
