"""Calibration of site scores: what CRBM.scoreHistogram returns.  A ScoreHistogram holds, per motif and strand, the
counts of the scan's scores over a background stream, binned in the log-odds x (prob = sigmoid(x)) by the rule of
crbm_scan_histogram_codes (include/crbm_amd.h): bin 0 holds everything below lo, the last bin everything at or above
hi.  It turns them into per-motif thresholds for a target false-positive rate and into p-values of scanSites records.
Host code only: NumPy on a few thousand integers."""
import numpy as np


def _sigmoid(x):
    return 1.0 / (1.0 + np.exp(-np.asarray(x, np.float64)))


class ScoreHistogram(object):
    """counts (K, S, bins) int64; edges (bins + 1,) float64, edges[0] = lo and edges[-1] = hi; windows: the valid
    windows scored, the sum of every (motif, strand) row; doublestranded: S = 2, strand +1 at s = 0 and -1 at s = 1
    (S = 1: the single strand 0)."""

    def __init__(self, counts, edges, windows, doublestranded):
        counts = np.ascontiguousarray(counts, dtype=np.int64)
        edges = np.ascontiguousarray(edges, dtype=np.float64)
        doublestranded = bool(doublestranded)
        if counts.ndim != 3 or counts.shape[1] != (2 if doublestranded else 1):
            raise ValueError("counts must be (K, S, bins) with S = 2 for double-stranded models, 1 otherwise")
        if edges.shape != (counts.shape[2] + 1,) or not np.all(np.isfinite(edges)) or np.any(np.diff(edges) <= 0):
            raise ValueError("edges must be bins + 1 finite ascending values")
        if counts.min(initial=0) < 0 or np.any(counts.sum(axis=2) != int(windows)):
            raise ValueError("every (motif, strand) row of counts must sum to windows")
        self.counts, self.edges, self.windows, self.doublestranded = counts, edges, int(windows), doublestranded

    @property
    def bins(self):
        return self.counts.shape[2]

    def __add__(self, other):
        if not isinstance(other, ScoreHistogram):
            return NotImplemented
        if (self.counts.shape != other.counts.shape or self.doublestranded != other.doublestranded
                or not np.array_equal(self.edges, other.edges)):
            raise ValueError("histograms of different binning or model shape cannot be added")
        return ScoreHistogram(self.counts + other.counts, self.edges, self.windows + other.windows, self.doublestranded)

    def tail(self):
        """(K, S, bins) int64: the scores in bin j or above"""
        return np.cumsum(self.counts[:, :, ::-1], axis=2)[:, :, ::-1]

    def _tail_bin(self, fpr):
        """(j, resolved): per (motif, strand) the smallest bin whose tail is at most fpr * windows"""
        if not (isinstance(fpr, (int, float, np.floating)) and 0.0 <= float(fpr) <= 1.0):
            raise ValueError("fpr must lie in [0, 1]")
        if self.windows < 1:
            raise ValueError("an empty histogram calibrates nothing")
        ok = self.tail() <= float(fpr) * self.windows                 # (the tail descends: once true, true above)
        return np.where(ok.any(axis=2), ok.argmax(axis=2), self.bins - 1), ok.any(axis=2)

    def thresholds(self, fpr):
        """(thr, resolved): thr (K, S) float32, the scanSites threshold of every motif and strand for at most a share
        `fpr` of background windows -- sigmoid(edges[j]) of the smallest bin j whose tail is at most fpr * windows,
        rounded towards 1 by one float32 step (0 for j = 0: the first bin is open below).  Where even the last bin
        holds more, resolved is False and thr is 1.0: widen the range or use more bins."""
        j, resolved = self._tail_bin(fpr)
        thr = np.nextafter(_sigmoid(self.edges[j]).astype(np.float32), np.float32(1.0))
        thr = np.where(j == 0, np.float32(0.0), thr)
        return np.where(resolved, thr, np.float32(1.0)).astype(np.float32), resolved

    def bin_of(self, x):
        """the bin of log-odds x (float64; -inf and +inf allowed) under the bin rule"""
        lo, hi = self.edges[0], self.edges[-1]
        with np.errstate(invalid="ignore", over="ignore"):
            t = (np.asarray(x, np.float64) - lo) * (self.bins / (hi - lo))
        t = np.where(t >= 0, t, 0.0)                                   # (t < 0 and NaN: the first bin)
        return np.minimum(t, self.bins - 1).astype(np.int64)

    def pvalues(self, sites):
        """p-values of SITE_DTYPE records (scanSites, motifSites): with j the bin of logit(prob),
        p = (tail[motif, s, j] + 1) / (windows + 1), s = 1 for strand -1 and 0 otherwise.  Conservative: the whole
        bin of the site counts as at least as extreme."""
        prob = np.asarray(sites["prob"], np.float64)
        with np.errstate(divide="ignore"):
            x = np.log(prob) - np.log1p(-prob)
        s = np.where(np.asarray(sites["strand"]) == -1, 1, 0)
        if s.size and s.max() >= self.counts.shape[1]:
            raise ValueError("records of strand -1 need the histogram of a double-stranded model")
        return (self.tail()[np.asarray(sites["motif"]), s, self.bin_of(x)] + 1.0) / (self.windows + 1.0)

    def save(self, path):
        """as .npz (numpy appends the extension when it is missing)"""
        np.savez(path, counts=self.counts, edges=self.edges, windows=np.int64(self.windows),
                 doublestranded=np.bool_(self.doublestranded))

    @classmethod
    def load(cls, path):
        with np.load(path) as z:
            return cls(z["counts"], z["edges"], int(z["windows"]), bool(z["doublestranded"]))
