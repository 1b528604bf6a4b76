"""Motif sites (CRBM.motifSites / motifBestSites, crbm_motif_sites*) on every model class of test_gpu_sweeps against
the float64 oracle (tie-aware, RTOL), against the GPU's own dense outputs (motifHitProbs and the flipped-filter
probabilities), bit for bit across input forms, slab sizes and runs; the overflow path (threshold 0, a capacity of 10);
and config #2's double-stranded model over 65 536 resident sequences."""
import ctypes

import numpy as np
import pytest

from tests.test_gpu_parity import make_pair, RTOL
from tests.test_gpu_sweeps import CLASSES, ids, _model, _codes, _onehot, _budget, _in_bytes

pytestmark = pytest.mark.gpu


def oracle_scores(o, D):
    """(S, n, K, Lh) float64: the + (or single) strand, then the reverse-complemented filter"""
    if o.doublestranded:
        P = [o._bottomUpProbability(o._bottomUpActivity(D)), o._bottomUpProbability(o._bottomUpActivity(D, True))]
    else:
        P = [o.motifHitProbs(D)]
    return np.stack([p[:, :, 0, :] for p in P])


def check_records(recs, P, thr, ds, complete=True, seq0=0):
    """recs of rows seq0.. against scores P of those rows: every record an oracle site, none below thr (1 - RTOL), no
    duplicates, sorted; complete: every position with p >= thr (1 + RTOL) present"""
    st = np.where(recs["strand"] == -1, 1, 0)
    assert np.all(np.isin(recs["strand"], (1, -1) if ds else (0,)))
    seq = recs["seq"] - seq0
    np.testing.assert_allclose(recs["prob"], P[st, seq, recs["motif"], recs["start"]], rtol=RTOL, atol=1e-7)
    assert np.all(recs["prob"] >= np.float32(thr * (1 - RTOL)))
    order = np.lexsort((st, recs["start"], recs["motif"], recs["seq"]))
    assert np.array_equal(order, np.arange(recs.size)), "records not sorted by (seq, motif, start, strand)"
    key = ((seq.astype(np.int64) * P.shape[2] + recs["motif"]) * P.shape[3] + recs["start"]) * 2 + st
    assert np.unique(key).size == recs.size
    if complete:
        want = np.argwhere(P >= thr * (1 + RTOL))                       # (strand, seq, motif, start)
        wkey = ((want[:, 1].astype(np.int64) * P.shape[2] + want[:, 2]) * P.shape[3] + want[:, 3]) * 2 + want[:, 0]
        assert np.isin(wkey, key).all(), "an oracle site is missing"


def check_best(best, P, ds):
    top = P.max(axis=(0, 3))
    np.testing.assert_allclose(best["prob"], top, rtol=RTOL, atol=1e-7)
    assert np.all(np.isin(best["strand"], (1, -1) if ds else (0,)))
    n, K = top.shape
    at = P[np.where(best["strand"] == -1, 1, 0), np.arange(n)[:, None], np.arange(K)[None, :], best["start"]]
    np.testing.assert_allclose(at, top, rtol=RTOL, atol=1e-7)


def _c_sites(m, lo, hi, thr, capacity, best=True):
    """crbm_motif_sites_resident on rows [lo, hi): (records, count, best dict or None)"""
    from crbm_amd import _lib
    from crbm_amd.crbm import _RAW_SITE
    n, K = hi - lo, m.num_motifs
    raw = np.zeros(capacity + 8, _RAW_SITE)
    raw["seq"] = -7
    count = ctypes.c_int64(-1)
    i32 = ctypes.POINTER(ctypes.c_int32)
    b = {"start": np.empty((n, K), np.int32), "strand": np.empty((n, K), np.int32), "prob": np.empty((n, K), np.float32)}
    m._call("crbm_motif_sites_resident", lo, hi, thr, capacity, raw.ctypes.data_as(ctypes.POINTER(_lib.CrbmSite)),
            ctypes.byref(count), b["start"].ctypes.data_as(i32) if best else None,
            b["strand"].ctypes.data_as(i32) if best else None, _lib.fptr(b["prob"]) if best else None)
    assert np.all(raw["seq"][capacity:] == -7), "a record landed past the capacity"
    if best:
        b["strand"] = b["strand"].astype(np.int8)
    return raw[:min(capacity, count.value)], count.value, (b if best else None)


def _same(a, b):
    assert a.size == b.size
    for f in ("seq", "motif", "start", "strand"):
        assert np.array_equal(a[f], b[f].astype(a[f].dtype))
    assert np.array_equal(a["prob"].view(np.uint32), b["prob"].view(np.uint32))


def _same_best(a, b):
    assert np.array_equal(a["start"], b["start"]) and np.array_equal(a["strand"], b["strand"])
    assert np.array_equal(a["prob"].view(np.uint32), b["prob"].view(np.uint32))


@pytest.mark.parametrize("cls", CLASSES, ids=ids(CLASSES))
def test_sites_against_oracle_sources_slabs_runs(cls, monkeypatch):
    name, K, M, ds, A, pool, Lf, L, env, spec = cls
    n, lo = 60, 5
    m, o = _model(cls, monkeypatch)
    allc = _codes(n + 11, L, A, seed=K + M + 1)
    m._upload(allc, 0)
    codes = allc[lo:lo + n]
    data = _onehot(codes, A)
    P = oracle_scores(o, data)
    S, Lh = P.shape[0], P.shape[3]
    thr = float(np.quantile(P, 0.97))
    _budget(monkeypatch, 0, None)
    sites = m.motifSites(codes, thr)
    best = m.motifBestSites(codes)
    check_records(sites, P, thr, ds)
    check_best(best, P, ds)
    assert sites.size > 0
    # the GPU's own dense outputs, thresholded: + (or .) records are motifHitProbs, - records the flipped filter
    hp = m.motifHitProbs(codes)[:, :, 0, :]
    plus = sites[sites["strand"] >= 0]
    np.testing.assert_allclose(plus["prob"], hp[plus["seq"], plus["motif"], plus["start"]], rtol=RTOL, atol=1e-7)
    assert np.isin(np.flatnonzero(hp >= thr * (1 + RTOL)),
                   np.ravel_multi_index((plus["seq"], plus["motif"], plus["start"]), hp.shape)).all()
    if ds:
        hm = m._bottomUpProbabilityOfData(data, flip_motif=True)[:, :, 0, :]
        minus = sites[sites["strand"] == -1]
        np.testing.assert_allclose(minus["prob"], hm[minus["seq"], minus["motif"], minus["start"]], rtol=RTOL, atol=1e-7)
        assert np.isin(np.flatnonzero(hm >= thr * (1 + RTOL)),
                       np.ravel_multi_index((minus["seq"], minus["motif"], minus["start"]), hm.shape)).all()
    # the same bits from one-hot input, the resident rows, a second run, and many slabs on both streams
    _same(sites, m.motifSites(data, thr))
    _same_best(best, m.motifBestSites(data))
    r, c, rb = _c_sites(m, lo, lo + n, thr, sites.size + 3)
    assert c == sites.size
    _same(sites, r)
    _same_best(best, rb)
    _same(sites, m.motifSites(codes, thr))
    dense = S * K * Lh * 4 if not spec else 0
    for src, x in (("codes", codes), ("onehot", data)):
        _budget(monkeypatch, _in_bytes(src, A, L) + K * 8 + dense, 9)    # 7 slabs, the last one short
        _same(sites, m.motifSites(x, thr))
        _same_best(best, m.motifBestSites(x))
    _budget(monkeypatch, K * 8 + dense, 9)
    r, c, rb = _c_sites(m, lo, lo + n, thr, sites.size)
    _same(sites, r)
    _same_best(best, rb)


@pytest.mark.parametrize("cls", [CLASSES[0], CLASSES[2], CLASSES[4]], ids=ids([CLASSES[0], CLASSES[2], CLASSES[4]]))
def test_sites_overflow(cls, monkeypatch):
    """threshold 0 over a multi-slab sweep: every position is a site, count exact, records complete and sorted; a
    capacity of 10 gets the exact count and exactly the first 10 records"""
    name, K, M, ds, A, pool, Lf, L, env, spec = cls
    n = 23
    m, o = _model(cls, monkeypatch)
    codes = _codes(n, L, A, seed=3)
    m._upload(codes, 0)
    P = oracle_scores(o, _onehot(codes, A))
    S, Lh = P.shape[0], P.shape[3]
    dense = S * K * Lh * 4 if not spec else 0
    _budget(monkeypatch, L + K * 8 + dense, 4)                           # 6 slabs over both streams
    sites = m.motifSites(codes, 0.0)
    assert sites.size == n * K * S * Lh
    check_records(sites, P, 0.0, ds)
    r, c, _ = _c_sites(m, 0, n, 0.0, 10, best=False)
    assert c == n * K * S * Lh and r.size == 10
    _same(sites[:10], r)


def test_sites_scale_cfg2_resident():
    """config #2's model (10 x 15, double-stranded) over 65 536 x 200 bp resident, about one site per (sequence,
    motif): the count against the oracle over all rows (tie-aware bounds), the first and last 1000 records against the
    oracle on their rows"""
    from oracle.crbm_oracle import onehot_of
    K, M, n, L = 10, 15, 65536, 200
    m, o = make_pair(K, M, ds=True, Lf=186, bshift=3.0, wscale=0.7)
    codes = _codes(n, L, 4, seed=77)
    m._upload(codes, 0)
    P0 = oracle_scores(o, onehot_of(codes[:2000]))
    thr = float(np.quantile(P0, 1.0 - 1.0 / (2 * (L - M + 1))))
    lo_n = hi_n = 0
    for a in range(0, n, 4096):
        P = oracle_scores(o, onehot_of(codes[a:a + 4096]))
        lo_n += int((P >= thr * (1 + RTOL)).sum())
        hi_n += int((P >= thr * (1 - RTOL)).sum())
    raw, count, _ = _c_sites(m, 0, n, thr, hi_n + 16, best=False)
    assert lo_n <= count <= hi_n and raw.size == count
    assert 0.3 * n * K < count < 3 * n * K
    for part in (raw[:1000], raw[-1000:]):
        s0, s1 = int(part["seq"][0]), int(part["seq"][-1])
        P = oracle_scores(o, onehot_of(codes[s0:s1 + 1]))
        check_records(part, P, thr, True, complete=False, seq0=s0)
        inner = raw[(raw["seq"] > s0) & (raw["seq"] < s1)]                # rows whose records all lie in the part
        if inner.size:
            Pi = oracle_scores(o, onehot_of(codes[s0 + 1:s1]))
            check_records(inner, Pi, thr, True, complete=True, seq0=s0 + 1)
