"""The stream scan (CRBM.scanSites, crbm_scan_sites_codes) on the GPU: against the float64 window scorer of
tests/scan_reference.py (tie-aware, RTOL) on specialised and slabbed model classes of test_gpu_sweeps; bit for bit
against motifSites on the same letters; the same bits for every CRBM_SLAB_BYTES and run; a gap removes exactly the
windows it touches; the overflow path; the refusals; and 2^24 letters on config #2's double-stranded model."""
import ctypes
import time

import numpy as np
import pytest

from tests.test_gpu_parity import make_pair, RTOL
from tests.test_gpu_sweeps import CLASSES, ids, _model, _codes
from tests.scan_reference import stream_scores, check_records

pytestmark = pytest.mark.gpu

SERVED = [CLASSES[0], CLASSES[1], CLASSES[2]]          # 10 x 15 ds, 20 x 15 ds, 300 x 10 as five slabs of 60 motifs
SPEC = [CLASSES[0], CLASSES[1]]
SEED, QUANTILE, T_A = 2031, 0.97, 5003                 # the stream and threshold of test (a); see its docstring


def gapped_stream(T, seed, share=0.01, run=25):
    """random letters, about `share` of them inside runs of `run` gaps, gaps at both ends"""
    rng = np.random.default_rng(seed)
    s = rng.integers(0, 4, size=T, dtype=np.uint8)
    for a in rng.integers(0, T - run, size=max(1, int(T * share / run))):
        s[a:a + run] = 4
    s[0] = s[T - 1] = 4
    return s


def per_start(cls):
    """bytes the driver counts per window start (crbm_sweep.h, stream_plan): 4 + 4 per slab"""
    name, K, M, ds, A, pool, Lf, L, env, spec = cls
    return 4 + 4 * (1 if spec else -(-K // 60))


def _c_scan(m, stream, thr, capacity):
    """crbm_scan_sites_codes: (records, count), guard records behind the capacity checked"""
    from crbm_amd import _lib
    from crbm_amd.crbm import _RAW_SITE
    raw = np.zeros(capacity + 8, _RAW_SITE)
    raw["seq"] = -7
    count = ctypes.c_int64(-1)
    m._call("crbm_scan_sites_codes", stream.ctypes.data_as(_lib._U8P), stream.size, thr, capacity,
            raw.ctypes.data_as(ctypes.POINTER(_lib.CrbmSite)), ctypes.byref(count))
    assert np.all(raw["seq"][capacity:] == -7), "a record landed past the capacity"
    return raw[:min(capacity, count.value)], count.value


def _same(a, b):
    assert a.size == b.size
    for f in ("seq", "motif", "start", "strand"):
        assert np.array_equal(a[f], b[f].astype(a[f].dtype)), f
    assert np.array_equal(a["prob"].view(np.uint32), b["prob"].view(np.uint32))


def _threshold(o, stream):
    P, valid = stream_scores(o, stream)
    return P, valid, float(np.quantile(P[:, :, valid], QUANTILE))


@pytest.mark.parametrize("cls", SERVED, ids=ids(SERVED))
def test_scan_against_reference_slabs_runs_and_gaps(cls, monkeypatch):
    """(a) the records against the float64 reference with the rules of test_gpu_sites.check_records: every record a
    reference site with matching probability, none below thr (1 - RTOL), every reference window at or above
    thr (1 + RTOL) present, sorted, no duplicates, nothing in an invalid window; windows inside the +-RTOL band are
    exempt from the presence check and may be at most 1 % of the reference's sites.  Stream: gapped_stream(5003,
    SEED); threshold: the 0.97 quantile of the reference's valid scores.  Observed on the CPU, reference alone:
    10 x 15 ds 2 946 sites, 0 in the band; 20 x 15 ds 5 891 sites, 2 in the band; 300 x 10 ss 44 316 sites, 9 in
    the band -- all far below 1 %.
    (c) the same bits for three CRBM_SLAB_BYTES -- the default (one segment), one that gives at least 6 segments, one
    whose segment edge falls inside a window that holds a site -- and for a second run.
    (d) a gap at one position removes exactly the records of the windows that cover it."""
    name, K, M, ds, A, pool, Lf, L, env, spec = cls
    m, o = _model(cls, monkeypatch)
    stream = gapped_stream(T_A, SEED)
    P, valid, thr = _threshold(o, stream)
    monkeypatch.delenv("CRBM_SLAB_BYTES", raising=False)
    sites = m.scanSites(stream, thr)
    n_ref, band = check_records(sites, P, thr, ds, RTOL)
    print("%s: %d records, reference %d sites, %d in the band" % (name, sites.size, n_ref, band))
    assert sites.size > 0
    _same(sites, m.scanSites(stream, thr))                                 # a second run
    starts = T_A - M + 1
    monkeypatch.setenv("CRBM_SLAB_BYTES", str(per_start(cls) * (starts // 7 + 1)))      # 7 segments, the last one short
    _same(sites, m.scanSites(stream, thr))
    s0 = int(sites["start"][sites.size // 2])                              # an edge inside the window of this site
    edge = s0 + max(1, M // 2)
    assert s0 < edge < s0 + M and edge < starts
    monkeypatch.setenv("CRBM_SLAB_BYTES", str(per_start(cls) * edge))
    _same(sites, m.scanSites(stream, thr))
    monkeypatch.delenv("CRBM_SLAB_BYTES", raising=False)
    # (d)
    p = s0 + M // 3
    gap = stream.copy()
    gap[p] = 4
    keep = ~((sites["start"] > p - M) & (sites["start"] <= p))
    assert not keep.all()
    _same(sites[keep], m.scanSites(gap, thr))


@pytest.mark.parametrize("cls", SPEC, ids=ids(SPEC))
def test_scan_equals_motif_sites_bit_for_bit(cls, monkeypatch):
    """(b) an (n, L) block of N-free rows as one stream with separators: scanSites with offsets, re-sorted to
    motifSites' order, equals motifSites(codes, thr) field by field, prob bit for bit"""
    name, K, M, ds, A, pool, Lf, L, env, spec = cls
    n = 37
    m, o = _model(cls, monkeypatch)
    codes = _codes(n, L, 4, seed=K + M + 3)
    stream = np.full((n, L + 1), 4, np.uint8)
    stream[:, :L] = codes
    stream = np.ascontiguousarray(stream.ravel()[:-1])
    offsets = np.arange(n + 1, dtype=np.int64) * (L + 1)
    _, _, thr = _threshold(o, stream[:4000])
    want = m.motifSites(codes, thr)
    got = m.scanSites(stream, thr, offsets=offsets)
    assert want.size > 0
    order = np.lexsort((np.where(got["strand"] == -1, 1, 0), got["motif"], got["start"], got["seq"]))
    assert np.array_equal(order, np.arange(got.size)), "records not sorted by (seq, start, motif, strand)"
    resort = np.lexsort((np.where(got["strand"] == -1, 1, 0), got["start"], got["motif"], got["seq"]))
    _same(want, got[resort])


@pytest.mark.parametrize("cls", [CLASSES[0], CLASSES[2]], ids=ids([CLASSES[0], CLASSES[2]]))
def test_scan_overflow(cls, monkeypatch):
    """(e) threshold 0 with a capacity of 10 over several segments: the count is the number of valid windows x K x S,
    exactly the first 10 records are written and nothing past them; capacity 0 without an array counts alone"""
    from crbm_amd import _lib
    name, K, M, ds, A, pool, Lf, L, env, spec = cls
    m, o = _model(cls, monkeypatch)
    stream = gapped_stream(1501, 5)
    P, valid = stream_scores(o, stream)
    S = 2 if ds else 1
    monkeypatch.setenv("CRBM_SLAB_BYTES", str(per_start(cls) * 300))
    full = m.scanSites(stream, 0.0)
    assert full.size == int(valid.sum()) * K * S
    check_records(full, P, 0.0, ds, RTOL)
    r, c = _c_scan(m, stream, 0.0, 10)
    assert c == full.size and r.size == 10
    _same(full[:10], r)
    count = ctypes.c_int64(-1)
    m._call("crbm_scan_sites_codes", stream.ctypes.data_as(_lib._U8P), stream.size, 0.0, 0, None, ctypes.byref(count))
    assert count.value == full.size
    # nothing to find: a stream shorter than the motif, and one without a valid window
    assert m.scanSites(stream[1:M], 0.0).size == 0
    assert m.scanSites(np.full(200, 4, np.uint8), 0.0).size == 0
    assert m.scanSites(np.zeros(0, np.uint8), 0.0).size == 0


def test_scan_refusals_leave_the_handle_usable(monkeypatch):
    """(f) pooling, other alphabets and motifs beyond 64 letters are refused with their word; a bad code, a bad
    threshold and a negative length are refused by the C side too; the handle works afterwards"""
    from crbm_amd import _lib
    for cls, word in ((CLASSES[4], "pooling"), (CLASSES[8], "alphabet"), (CLASSES[7], "alphabet"), (CLASSES[6], "generic")):
        name, K, M, ds, A, pool, Lf, L, env, spec = cls
        m, o = _model(cls, monkeypatch)
        stream = gapped_stream(400, 3)
        with pytest.raises(Exception, match=word):
            m.scanSites(stream, 0.5)
        codes = _codes(6, L, A, seed=1)
        np.testing.assert_allclose(m.freeEnergy(codes), o.freeEnergy(np.ascontiguousarray(
            np.eye(A, dtype=np.float32)[codes].transpose(0, 2, 1)[:, None])), rtol=RTOL, atol=1e-6)
    m, o = _model(CLASSES[0], monkeypatch)
    stream = gapped_stream(400, 3)
    good = m.scanSites(stream, 0.5)
    count = ctypes.c_int64(-1)
    ptr = lambda a: a.ctypes.data_as(_lib._U8P)
    lib, h = m._lib, m._h()
    bad = stream.copy()
    bad[77] = 5
    assert lib.crbm_scan_sites_codes(h, ptr(bad), bad.size, 0.5, 0, None, ctypes.byref(count)) == _lib.ERR_INVALID
    assert lib.crbm_scan_sites_codes(h, ptr(stream), stream.size, 1.5, 0, None, ctypes.byref(count)) == _lib.ERR_INVALID
    assert lib.crbm_scan_sites_codes(h, ptr(stream), -1, 0.5, 0, None, ctypes.byref(count)) == _lib.ERR_INVALID
    assert lib.crbm_scan_sites_codes(h, ptr(stream), stream.size, 0.5, -1, None, ctypes.byref(count)) == _lib.ERR_INVALID
    assert lib.crbm_scan_sites_codes(h, ptr(stream), 2 ** 31, 0.5, 0, None, ctypes.byref(count)) == _lib.ERR_INVALID
    _same(good, m.scanSites(stream, 0.5))


def test_scan_scale_cfg2_two_to_the_24():
    """(g) config #2's double-stranded model over 2^24 + 1000 letters, about 1 % of them in gap runs: the records of
    every sampled N-free stretch of 200 letters (a sampled 1 % of the stream) are, in number and bit for bit, those
    of motifSites over the same stretches as rows; the time of the scan is printed"""
    K, M, L = 10, 15, 200
    T = (1 << 24) + 1000
    m, o = make_pair(K, M, ds=True, Lf=186, bshift=3.0, wscale=0.7)
    stream = gapped_stream(T, 99, share=0.01, run=500)
    Pq, vq = stream_scores(o, stream[:20000])
    thr = float(np.quantile(Pq[:, :, vq], 1.0 - 1.0 / 400))
    m.scanSites(stream[:100000], thr)                                       # warm-up: kernels loaded, buffers there
    t0 = time.perf_counter()
    sites = m.scanSites(stream, thr)
    dt = time.perf_counter() - t0
    print("scanSites over %d letters: %d records in %.1f ms" % (T, sites.size, dt * 1e3))
    assert np.all(np.diff(sites["start"].astype(np.int64)) >= 0)
    rng = np.random.default_rng(7)
    a = np.sort(rng.choice(T - L, size=T // (100 * L), replace=False))
    rows = stream[a[:, None] + np.arange(L)[None, :]]
    free = (rows < 4).all(axis=1)
    a, rows = a[free], np.ascontiguousarray(rows[free])
    assert a.size > 500
    want = m.motifSites(rows, thr)
    lo = np.searchsorted(sites["start"], a, side="left")
    hi = np.searchsorted(sites["start"], a + L - M, side="right")
    assert int((hi - lo).sum()) == want.size and want.size > 1000
    got = np.concatenate([sites[l:h] for l, h in zip(lo, hi)])
    seq = np.repeat(np.arange(a.size), hi - lo)
    rel = got["start"] - a[seq]
    order = np.lexsort((np.where(got["strand"] == -1, 1, 0), rel, got["motif"], seq))
    assert np.array_equal(seq[order], want["seq"]) and np.array_equal(rel[order], want["start"])
    assert np.array_equal(got["motif"][order], want["motif"]) and np.array_equal(got["strand"][order], want["strand"])
    assert np.array_equal(got["prob"][order].view(np.uint32), want["prob"].view(np.uint32))
