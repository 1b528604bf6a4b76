"""The yardstick of the score histogram (CRBM.scoreHistogram, crbm_scan_histogram_codes): float64 log-odds of every
window straight from the oracle's activations (no sigmoid in between, so nothing saturates), exact counts under the bin
rule of include/crbm_amd.h, and check_histogram, which holds counts formed in fp32 to them.

A count cannot be compared bin by bin: a score within rounding of an edge may fall on either side.  So every interior
edge e_j gets a band of half-width delta_j = RTOL * max(1, |e_j|) -- the project's fp32 tolerance (tests/test_gpu_parity.py)
applied to the activation -- and the histogram's tail at bin j must lie between the reference's tails at e_j + delta_j
and e_j - delta_j.  Row totals are exact."""
import numpy as np

from oracle.crbm_oracle import onehot_of
from tests.scan_reference import window_valid

RTOL = 1e-4


def stream_logodds(o, stream):
    """(X, valid): X (S, K, T - M + 1) float64, the log-odds of stream_scores' P -- x (+) and x' of the
    reverse-complemented filter (-) for double-stranded models, x + x' for single-stranded ones; entries of invalid
    windows are NaN"""
    stream = np.asarray(stream, np.uint8)
    K = o.num_motifs
    S = 2 if o.doublestranded else 1
    valid = window_valid(stream, o.motif_length)
    if valid.size == 0:
        return np.zeros((S, K, 0)), valid
    D = onehot_of(np.where(stream > 3, 0, stream)[None, :])
    fwd, rev = o._bottomUpActivity(D)[0, :, 0, :], o._bottomUpActivity(D, True)[0, :, 0, :]
    X = np.stack([fwd, rev] if o.doublestranded else [fwd + rev]).astype(np.float64)
    X[:, :, ~valid] = np.nan
    return X, valid


def edges_of(lo, hi, nbins):
    return lo + (hi - lo) * np.arange(nbins + 1) / nbins


def reference_counts(x_ref, valid, lo, hi, nbins):
    """(K, S, nbins) int64: the exact counts of the float64 scores under the bin rule"""
    S, K, _ = x_ref.shape
    out = np.zeros((K, S, nbins), np.int64)
    for s in range(S):
        for k in range(K):
            t = (x_ref[s, k, valid] - lo) * (nbins / (hi - lo))
            b = np.where(t < 0, 0, np.where(t >= nbins, nbins - 1, np.minimum(np.maximum(t, 0), nbins - 1).astype(np.int64)))
            out[k, s] = np.bincount(b, minlength=nbins)
    return out


def check_histogram(counts, windows, x_ref, valid, lo, hi, nbins, rtol=RTOL, band_share=0.01):
    """counts (K, S, nbins) and windows against the reference scores x_ref (S, K, starts) of the `valid` windows:
      1. every (k, s) row sums to the number of valid windows, exactly, and so does `windows`;
      2. for every interior edge j: tail_ref(e_j + delta_j) <= tail[k, s, j] <= tail_ref(e_j - delta_j);
      3. the reference scores inside any band are at most `band_share` of all scores -- a condition on the inputs, so
         that 2. cannot pass by bands that swallow the data.
    Returns the share of 3."""
    counts = np.asarray(counts)
    S, K, _ = x_ref.shape
    n = int(valid.sum())
    assert counts.shape == (K, S, nbins), counts.shape
    assert int(windows) == n, (int(windows), n)
    totals = counts.sum(axis=2)
    assert np.all(totals == n), ("row totals", np.argwhere(totals != n)[:5].tolist(), n)
    e = edges_of(lo, hi, nbins)[1:nbins]
    d = rtol * np.maximum(1.0, np.abs(e))
    tail = np.cumsum(counts[:, :, ::-1].astype(np.int64), axis=2)[:, :, ::-1]
    in_band = 0
    for s in range(S):
        for k in range(K):
            xs = np.sort(x_ref[s, k, valid])
            below_hi = np.searchsorted(xs, e + d, side="left")           # scores < e + d
            below_lo = np.searchsorted(xs, e - d, side="left")           # scores < e - d
            t = tail[k, s, 1:]
            bad = (t < n - below_hi) | (t > n - below_lo)
            assert not bad.any(), ("tail outside its bounds", k, s, (1 + np.flatnonzero(bad))[:5].tolist(),
                                   t[bad][:5].tolist(), (n - below_hi)[bad][:5].tolist(), (n - below_lo)[bad][:5].tolist())
            in_band += int((below_hi - below_lo).sum())
    share = in_band / max(1, n * K * S)
    assert share <= band_share, ("scores inside the bands", share)
    return share
