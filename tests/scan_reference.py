"""The yardstick of the stream scan (CRBM.scanSites, crbm_scan_sites_codes): a float64 NumPy window scorer on the
oracle.  A stream is a 1-D uint8 array of codes, 0..3 = A,C,G,T and 4 = no letter.  Window s covers codes
[s, s + M); it is valid when all of them are letters.  A valid window has the scores the oracle gives the same M
letters in a row -- sigma(x + x'), strand 0, for single-stranded models; sigma(x) (+1) and sigma(x') of the
reverse-complemented filter (-1) for double-stranded ones -- which depend on those M letters alone, so the invalid
positions may hold any letter while the scores are formed and are masked afterwards."""
import numpy as np

from oracle.crbm_oracle import onehot_of

REC = np.dtype([("seq", "<i4"), ("motif", "<i4"), ("start", "<i4"), ("strand", "<i4"), ("prob", "<f8")])


def window_valid(stream, M):
    """(T - M + 1,) bool: all M codes from s on are letters (empty for T < M)"""
    stream = np.asarray(stream)
    T = stream.size
    if T < M:
        return np.zeros(0, bool)
    bad = np.concatenate(([0], np.cumsum(stream > 3)))
    return (bad[M:] - bad[:T - M + 1]) == 0


def stream_scores(o, stream):
    """(P, valid): P (S, K, T - M + 1) float64, the + (or single) strand first, then the reverse-complemented filter;
    entries of invalid windows are -1"""
    stream = np.asarray(stream, np.uint8)
    M, K = o.motif_length, o.num_motifs
    S = 2 if o.doublestranded else 1
    valid = window_valid(stream, M)
    if valid.size == 0:
        return np.zeros((S, K, 0)), valid
    D = onehot_of(np.where(stream > 3, 0, stream)[None, :])
    if o.doublestranded:
        P = [o._bottomUpProbability(o._bottomUpActivity(D)), o._bottomUpProbability(o._bottomUpActivity(D, True))]
    else:
        P = [o.motifHitProbs(D)]
    P = np.stack([p[0, :, 0, :] for p in P]).astype(np.float64)
    P[:, :, ~valid] = -1.0
    return P, valid


def reference_sites(o, stream, thr):
    """the sites with prob >= thr, sorted by (start, motif, strand), + before -"""
    P, _ = stream_scores(o, stream)
    st, k, s = np.nonzero(P >= thr)
    order = np.lexsort((st, k, s))
    out = np.zeros(order.size, REC)
    out["motif"], out["start"] = k[order], s[order]
    out["strand"] = np.where(st[order] == 1, -1, 1) if o.doublestranded else 0
    out["prob"] = P[st[order], k[order], s[order]]
    return out


def check_records(recs, P, thr, ds, rtol, complete=True, band_share=0.01):
    """The rules of tests/test_gpu_sites.check_records for stream records against stream_scores' P: every record a
    reference site with matching probability (none in an invalid window: P is -1 there), none below thr (1 - rtol),
    sorted by (start, motif, strand) without duplicates; complete: every reference window at or above thr (1 + rtol)
    present.  Windows inside the +-rtol band are exempt from the presence check; at most `band_share` of the
    reference's sites may lie there.  Returns (reference sites, windows in the band)."""
    st = np.where(recs["strand"] == -1, 1, 0)
    assert np.all(np.isin(recs["strand"], (1, -1) if ds else (0,)))
    assert np.all(recs["seq"] == 0)
    p_ref = P[st, recs["motif"], recs["start"]]
    assert np.all(p_ref >= 0), "a record in an invalid window"
    np.testing.assert_allclose(recs["prob"], p_ref, rtol=rtol, atol=1e-7)
    assert np.all(recs["prob"] >= np.float32(thr * (1 - rtol)))
    order = np.lexsort((st, recs["motif"], recs["start"]))
    assert np.array_equal(order, np.arange(recs.size)), "records not sorted by (start, motif, strand)"
    key = (recs["start"].astype(np.int64) * P.shape[1] + recs["motif"]) * 2 + st
    assert np.unique(key).size == recs.size
    n_ref = int((P >= thr).sum())
    band = int(((P >= thr * (1 - rtol)) & (P < thr * (1 + rtol))).sum())
    if complete:
        w_st, w_k, w_s = np.nonzero(P >= thr * (1 + rtol))
        wkey = (w_s.astype(np.int64) * P.shape[1] + w_k) * 2 + w_st
        assert np.isin(wkey, key).all(), "a reference site is missing"
        assert band <= band_share * max(n_ref, 1), (band, n_ref)
    return n_ref, band
