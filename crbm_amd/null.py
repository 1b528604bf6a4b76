"""The analytic null: the exact distribution of a motif's window score under a Markov background.

The log-odds x that scanSites reports for a motif and strand is additive over the window: x = c + sum_j w[j][a_j], a
position weight matrix.  scoreDistribution rounds the weights to multiples of `step`, and the device
(crbm_score_distribution, crbm_null.h) runs the dynamic programme over (context, integer score) of a MarkovBackground of
order 0..3.  The result is exact to any tail depth -- no sampling noise, no floor of 1 / (windows + 1) -- up to the
rounding of the weights, which every ScoreDistribution carries as the rigorous bound `err`: |x - (offset + step Q)| <= err
for every window.  tail_bounds, thresholds and pvalues account for it.

Limits.  The null describes one window: far from any gap (start="stationary") or right behind one (start="run", the chain
of sampleBackground at the start of a run).  Single-stranded scores sum both orientations, as scanSites does.  Tail
probabilities below about 1e-300 underflow to 0.  DNA models with pooling == 1 only."""
import ctypes

import numpy as np

from . import _lib
from .background import MarkovBackground, contexts, MAX_ORDER

_DP = ctypes.POINTER(ctypes.c_double)
MAX_G = 2 ** 24
STARTS = ("stationary", "run")


def next_context(order, s, a):
    """the context behind context s once letter a has been appended (crbm_background.h)"""
    j = 0
    while j < order and s >= (4 ** (j + 1) - 1) // 3:
        j += 1
    v = (s - (4 ** j - 1) // 3) * 4 + a
    if j < order:
        return (4 ** (j + 1) - 1) // 3 + v
    return (4 ** order - 1) // 3 + v % 4 ** order


def window_pwm(model):
    """(w, c): w (R, M, 4) and c (R,) float64 of the rows r = k * S + s, so that the log-odds of scanSites for motif k,
    strand s and the window a_0 .. a_{M-1} is c[r] + sum_j w[r][j][a_j]"""
    W = np.asarray(model.motifs.get_value(), np.float64)[:, 0]           # (K, 4, M)
    b = np.asarray(model.bias.get_value(), np.float64).reshape(-1)
    fwd = W.transpose(0, 2, 1)                                           # (K, M, 4)
    rev = W[:, ::-1, ::-1].transpose(0, 2, 1)                            # the reverse-complemented filter
    if model.doublestranded:
        w = np.stack([fwd, rev], axis=1).reshape(-1, fwd.shape[1], 4)
        c = np.repeat(b, 2)
    else:
        w, c = fwd + rev, 2.0 * b
    return np.ascontiguousarray(w), np.ascontiguousarray(c)


def quantise(w, c, step):
    """(q, offset, err, G): q (R, M, 4) int32 >= 0 with min_a q = 0, offset (R,) the log-odds of Q = 0, err (R,) with
    |x - (offset + step Q)| <= err for every window, G (R,) int64 the number of integer scores of a row"""
    w = np.asarray(w, np.float64)
    q0 = np.rint(w / step)
    if not np.all(np.abs(q0) < 2.0 ** 30):
        raise ValueError("step %g is too small for these weights: use a larger step" % step)
    err = np.abs(w - step * q0).max(axis=2).sum(axis=1)
    low = q0.min(axis=2, keepdims=True)
    q = (q0 - low).astype(np.int32)
    offset = np.asarray(c, np.float64) + step * low[:, :, 0].sum(axis=1)
    G = q.max(axis=2).astype(np.int64).sum(axis=1) + 1
    return np.ascontiguousarray(q), offset, err, G


def stationary(P, order):
    """(contexts,) float64: the stationary distribution of the full-length contexts under P (contexts, 4), zero on the
    partial ones.  ValueError when it is not unique."""
    P = np.asarray(P, np.float64)
    base, F = (4 ** order - 1) // 3, 4 ** order
    T = np.zeros((F, F))
    for s in range(F):
        for a in range(4):
            T[s, next_context(order, base + s, a) - base] += P[base + s, a]
    _, sv, vh = np.linalg.svd(T.T - np.eye(F))
    if np.sum(sv < 1e-10) != 1:
        raise ValueError('the chain is reducible at this pseudocount and has no unique stationary distribution: '
                         'use a pseudocount above 0, or start="run"')
    pi = vh[-1] / vh[-1].sum()
    for _ in range(3):                                                   # polish: pi T = pi to rounding
        pi = np.maximum(pi @ T, 0.0)
        pi /= pi.sum()
    out = np.zeros(contexts(order))
    out[base:] = pi
    return out


def start_distribution(P, order, start):
    if start == "stationary":
        return stationary(P, order)
    if start == "run":
        init = np.zeros(contexts(order))
        init[0] = 1.0
        return init
    raise ValueError('start must be "stationary" or "run"')


def last_device_ms(model):
    """device time (HIP events around the kernels of every group of rows, summed) of the model's last scoreDistribution"""
    ms = ctypes.c_float(0.0)
    model._call("crbm_null_ms", ctypes.byref(ms))
    return float(ms.value)


def _sigmoid(x):
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-np.asarray(x, np.float64)))


_BELOW_ONE = np.nextafter(np.float32(1.0), np.float32(0.0))


class ScoreDistribution(object):
    """pmf (K, S, G) float64: the probability of every integer score Q of motif k and strand s (S = 2 for double-stranded
    models, strand +1 at s = 0 and -1 at s = 1; S = 1 otherwise), zero beyond a row's own range; offset (K, S): the
    log-odds of Q = 0; err (K, S): the true log-odds x of any window and its integer score Q obey
    |x - (offset + step Q)| <= err; step; doublestranded; order and start: what it was computed for."""

    def __init__(self, pmf, offset, err, step, doublestranded, order, start):
        pmf = np.ascontiguousarray(pmf, dtype=np.float64)
        doublestranded = bool(doublestranded)
        if pmf.ndim != 3 or pmf.shape[1] != (2 if doublestranded else 1) or pmf.shape[2] < 1:
            raise ValueError("pmf must be (K, S, G) with S = 2 for double-stranded models, 1 otherwise")
        offset, err = np.ascontiguousarray(offset, dtype=np.float64), np.ascontiguousarray(err, dtype=np.float64)
        if offset.shape != pmf.shape[:2] or err.shape != pmf.shape[:2] or np.any(err < 0) or not (np.all(np.isfinite(offset)) and np.all(np.isfinite(err))):
            raise ValueError("offset and err must be finite (K, S) arrays, err not negative")
        if not (np.isfinite(step) and step > 0):
            raise ValueError("step must be positive")
        if pmf.min() < 0 or not np.all(np.isfinite(pmf)):
            raise ValueError("pmf must be finite and not negative")
        if start not in STARTS:
            raise ValueError('start must be "stationary" or "run"')
        self.pmf, self.offset, self.err, self.step = pmf, offset, err, float(step)
        self.doublestranded, self.order, self.start = doublestranded, int(order), str(start)

    @property
    def G(self):
        return self.pmf.shape[2]

    def tail(self):
        """(K, S, G + 1) float64: P(Q >= n), n = 0 .. G (the last entry is 0)"""
        t = np.cumsum(self.pmf[:, :, ::-1], axis=2)[:, :, ::-1]
        return np.concatenate([t, np.zeros(t.shape[:2] + (1,))], axis=2)

    def _first(self, x):
        """the smallest integer score Q with offset + step Q >= x, clipped to [0, G]; x broadcasts against (K, S)"""
        with np.errstate(invalid="ignore", over="ignore"):
            n = np.ceil((np.asarray(x, np.float64) - self.offset) / self.step)
        return np.clip(np.nan_to_num(n, nan=0.0, posinf=self.G, neginf=0.0), 0, self.G).astype(np.int64)

    def tail_bounds(self, x):
        """(lower, upper), each (K, S): rigorous bounds of P(X >= x) for the true log-odds X of a background window --
        upper = P(offset + step Q >= x - err), lower = P(offset + step Q >= x + err)"""
        t = self.tail()
        k, s = np.indices(self.offset.shape)
        return t[k, s, self._first(x + self.err)], t[k, s, self._first(x - self.err)]

    def thresholds(self, fpr):
        """(thr, resolved): thr (K, S) float32, the scanSites threshold of every motif and strand for at most a share
        `fpr` of background windows.  With n the smallest integer score whose tail P(Q >= n) is at most fpr, every window
        with a log-odds above x = offset + err + step (n - 1) has Q >= n; thr is sigmoid(x), rounded towards 1 by one
        float32 step (0 for n = 0: every window may pass).  Where that is 1.0 the float32 probability of a site cannot
        resolve the threshold, and resolved is False."""
        if not (isinstance(fpr, (int, float, np.floating)) and 0.0 <= float(fpr) <= 1.0):
            raise ValueError("fpr must lie in [0, 1]")
        ok = self.tail() <= float(fpr)                                   # (the tail descends, and its last entry is 0)
        n = ok.argmax(axis=2)
        x = self.offset + self.err + self.step * (n - 1.0)
        thr = np.nextafter(_sigmoid(x).astype(np.float32), np.float32(1.0))
        thr = np.where(n == 0, np.float32(0.0), thr).astype(np.float32)
        return thr, thr < np.float32(1.0)

    def pvalues(self, sites):
        """the upper tail bound at logit(prob) of SITE_DTYPE records (scanSites, motifSites), by their motif and strand.
        prob is clipped to the largest float32 below 1: a saturated site gets the tail at that score, not 0.  No + 1
        smoothing: nothing was sampled."""
        prob = np.minimum(np.asarray(sites["prob"], np.float64), np.float64(_BELOW_ONE))
        with np.errstate(divide="ignore"):
            x = np.log(prob) - np.log1p(-prob)
        k = np.asarray(sites["motif"], np.int64)
        s = np.where(np.asarray(sites["strand"]) == -1, 1, 0)
        if s.size and s.max() >= self.pmf.shape[1]:
            raise ValueError("records of strand -1 need the distribution of a double-stranded model")
        with np.errstate(invalid="ignore", over="ignore"):
            n = np.ceil((x - self.err[k, s] - self.offset[k, s]) / self.step)
        n = np.clip(np.nan_to_num(n, nan=0.0, posinf=self.G, neginf=0.0), 0, self.G).astype(np.int64)
        return self.tail()[k, s, n]

    def binned(self, bins, lo, hi):
        """(K, S, bins) float64: the probability of every bin of a ScoreHistogram of `bins` bins over [lo, hi) -- the bin
        rule of crbm_scan_histogram_codes applied to the grid scores offset + step Q -- for comparison with an empirical
        histogram's counts / windows"""
        bins = int(bins)
        if bins < 1 or not (np.isfinite(lo) and np.isfinite(hi) and lo < hi):
            raise ValueError("bins must be positive and lo < hi finite")
        out = np.zeros(self.pmf.shape[:2] + (bins,))
        Q = np.arange(self.G, dtype=np.float64)
        for k in range(self.pmf.shape[0]):
            for s in range(self.pmf.shape[1]):
                t = (self.offset[k, s] + self.step * Q - lo) * (bins / (hi - lo))
                b = np.minimum(np.where(t >= 0, t, 0.0), bins - 1).astype(np.int64)
                out[k, s] = np.bincount(b, weights=self.pmf[k, s], minlength=bins)
        return out

    def save(self, path):
        """as .npz (numpy appends the extension when it is missing)"""
        np.savez(path, pmf=self.pmf, offset=self.offset, err=self.err, step=np.float64(self.step),
                 doublestranded=np.bool_(self.doublestranded), order=np.int64(self.order), start=np.str_(self.start))

    @classmethod
    def load(cls, path):
        with np.load(path) as z:
            return cls(z["pmf"], z["offset"], z["err"], float(z["step"]), bool(z["doublestranded"]), int(z["order"]), str(z["start"]))


def scoreDistribution(model, background, step=2 ** -10, pseudocount=1.0, start="stationary"):
    """The ScoreDistribution of every motif and strand of `model` under `background` (a MarkovBackground; its
    probabilities(pseudocount)), the weights rounded to multiples of `step`.  start: "stationary" -- a window far from
    any gap, the context in front of it drawn from the chain's stationary distribution -- or "run" -- the first window
    behind a gap.  Serves every DNA model (input_dims == 4) with pooling == 1, whatever kernels it trains on."""
    if not isinstance(background, MarkovBackground):
        raise ValueError("background must be a MarkovBackground (fitBackground)")
    if getattr(model, "input_dims", None) != 4 or getattr(model, "pooling", None) != 1:
        raise ValueError("scoreDistribution serves DNA models (input_dims == 4) with pooling == 1")
    if isinstance(step, bool) or not isinstance(step, (int, float, np.floating, np.integer)) or not (np.isfinite(step) and step > 0):
        raise ValueError("step must be a positive number")
    if start not in STARTS:
        raise ValueError('start must be "stationary" or "run"')
    step = float(step)
    order = background.order
    assert 0 <= order <= MAX_ORDER
    P = np.ascontiguousarray(background.probabilities(pseudocount))
    init = np.ascontiguousarray(start_distribution(P, order, start))
    w, c = window_pwm(model)
    q, offset, err, Gr = quantise(w, c, step)
    G = int(Gr.max())
    if G > MAX_G:
        raise ValueError("step %g gives %d integer scores, more than 2^24: use a larger step" % (step, G))
    R, M = q.shape[:2]
    pmf = np.zeros((R, G), np.float64)
    model._call("crbm_score_distribution", q.ctypes.data_as(_lib._I32P), R, M, order, P.ctypes.data_as(_DP), init.ctypes.data_as(_DP),
                G, pmf.ctypes.data_as(_DP))
    S = 2 if model.doublestranded else 1
    return ScoreDistribution(pmf.reshape(-1, S, G), offset.reshape(-1, S), err.reshape(-1, S), step, model.doublestranded, order, start)
