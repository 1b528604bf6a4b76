"""Markov backgrounds: the null of a motif scan that keeps the short-range dependence of real sequence (CpG depletion,
poly-A), which sequences.shuffleStream destroys.

fitBackground counts the j-mers of a stream on the device (crbm_stream_kmer_counts) and returns a MarkovBackground
of order 0..3; sampleBackground draws a stream of any length from it on the device (crbm_background_sample), gaps and
record structure taken from a template stream.  The result goes wherever shuffleStream's does: scoreHistogram,
scanSites, recordSummary.  Both device operations are model-independent; the model lends its device.  MarkovBackground
itself is host code: NumPy on a few hundred integers.

Contexts: the last j <= order letters l_1 .. l_j, oldest first, have the index (4^j - 1) / 3 + sum_i l_i 4^(j - i); the
empty context is 0 (include/crbm_amd.h)."""
import ctypes

import numpy as np

from . import _lib

MAX_ORDER = 3
_MAX_T = 2 ** 31 - 1          # letters of one C call; longer streams are cut behind gaps
_U32P = ctypes.POINTER(ctypes.c_uint32)
_U64P = ctypes.POINTER(ctypes.c_uint64)


def _check_order(order):
    if isinstance(order, bool) or not isinstance(order, (int, np.integer)) or not 0 <= order <= MAX_ORDER:
        raise ValueError("order must be an integer in [0, %d]" % MAX_ORDER)
    return int(order)


def contexts(order):
    """the number of contexts of an order: 1, 5, 21, 85"""
    return (4 ** (order + 1) - 1) // 3


def kmer_offset(j):
    """where the j-mers (j >= 1) start in a counts array: 0, 4, 20, 84"""
    return (4 ** j - 4) // 3


def kmer_slots(order):
    """the length of a counts array: 4, 20, 84, 340"""
    return kmer_offset(order + 2)


def context_index(letters):
    """the index of the context l_1 .. l_j (codes 0..3, oldest first); () is the empty context 0"""
    v = 0
    for a in letters:
        if not 0 <= int(a) <= 3:
            raise ValueError("a context holds letters 0..3")
        v = 4 * v + int(a)
    return (4 ** len(letters) - 1) // 3 + v


def check_table(table):
    """(table, order) of a raw threshold table: (contexts, 3) uint32, every row ascending"""
    table = np.asarray(table)
    if table.dtype != np.uint32 or table.ndim != 2 or table.shape[1] != 3 or table.shape[0] not in (1, 5, 21, 85):
        raise ValueError("a threshold table is (contexts, 3) uint32 with 1, 5, 21 or 85 contexts (order 0..3)")
    if np.any(table[:, 1:] < table[:, :-1]):
        raise ValueError("a row of the threshold table does not ascend")
    return np.ascontiguousarray(table), (1, 5, 21, 85).index(table.shape[0])


class MarkovBackground(object):
    """A Markov chain of order 0..3 over A, C, G, T as the counts it was fitted from: `counts` (uint64) holds, for every
    j = 1 .. order + 1, the occurrences of every j-mer -- the 1-mers, then the 2-mers, ..., each block indexed with the
    oldest letter most significant (kmer_offset(j) + index).  a + b pools the counts of two backgrounds of equal
    order."""

    def __init__(self, order, counts):
        self.order = _check_order(order)
        counts = np.asarray(counts)
        if counts.shape != (kmer_slots(self.order),) or counts.dtype.kind not in "ui" or (counts.dtype.kind == "i" and counts.min(initial=0) < 0):
            raise ValueError("counts must be %d non-negative integers (order %d)" % (kmer_slots(self.order), self.order))
        self.counts = np.ascontiguousarray(counts, dtype=np.uint64)

    def kmers(self, j):
        """the counts of the j-mers, (4,) * j"""
        if not 1 <= j <= self.order + 1:
            raise ValueError("j must lie in [1, order + 1]")
        return self.counts[kmer_offset(j):kmer_offset(j + 1)].reshape((4,) * j)

    def probabilities(self, pseudocount=1.0):
        """(contexts, 4) float64: P(a | ctx) = (n[ctx . a] + pseudocount) / (sum_a n[ctx . a] + 4 pseudocount).  A context
        of j < order letters (the first letters of a run) uses the (j + 1)-mer counts.  Where the denominator is 0
        (pseudocount 0 and a context never seen) the row is uniform."""
        alpha = float(pseudocount)
        if not (np.isfinite(alpha) and alpha >= 0.0):
            raise ValueError("pseudocount must be finite and not negative")
        rows = []
        for j in range(self.order + 1):
            n = self.kmers(j + 1).reshape(-1, 4).astype(np.float64)
            den = n.sum(axis=1, keepdims=True) + 4.0 * alpha
            with np.errstate(invalid="ignore", divide="ignore"):
                rows.append(np.where(den > 0, (n + alpha) / den, 0.25))
        return np.concatenate(rows, axis=0)

    def thresholds(self, pseudocount=1.0):
        """(contexts, 3) uint32: thr[ctx][i] = min(2^32 - 1, floor(2^32 sum_{a <= i} P(a | ctx))), in float64 -- what
        crbm_background_sample compares its draws with."""
        cum = np.cumsum(self.probabilities(pseudocount)[:, :3], axis=1)
        return np.minimum(np.floor(cum * 4294967296.0), 4294967295.0).astype(np.uint32)

    def __add__(self, other):
        if not isinstance(other, MarkovBackground):
            return NotImplemented
        if other.order != self.order:
            raise ValueError("backgrounds of different order cannot be added")
        return MarkovBackground(self.order, self.counts + other.counts)

    def save(self, path):
        """as .npz (numpy appends the extension when it is missing)"""
        np.savez(path, order=np.int64(self.order), counts=self.counts)

    @classmethod
    def load(cls, path):
        with np.load(path) as z:
            return cls(int(z["order"]), z["counts"])


def _check_stream(stream):
    if not isinstance(stream, np.ndarray) or stream.dtype != np.uint8 or stream.ndim != 1:
        raise ValueError("stream must be a one-dimensional uint8 array of codes 0..4 (sequences.seqsToStream)")
    stream = np.ascontiguousarray(stream)
    if stream.size and int(stream.max()) > 4:
        raise ValueError("stream codes must lie in 0..4 (0..3 = A,C,G,T; 4 = no letter)")
    return stream


def _gap_cuts(stream, limit):
    """[lo, hi) of the pieces of at most `limit` codes a stream goes to the device in: a piece ends behind a gap, so the
    next one starts from the empty context and no j-mer spans two pieces"""
    lo, T = 0, stream.size
    while T - lo > limit:
        window = stream[lo:lo + limit]
        back = int(np.argmax(window[::-1] == 4))
        if window[limit - 1 - back] != 4:
            raise ValueError("a stream of more than %d codes is cut behind gaps, and %d codes from %d on hold none" % (limit, limit, lo))
        yield lo, lo + limit - back
        lo += limit - back
    yield lo, T


def fitBackground(model, stream, order=3, _cut=None):
    """The MarkovBackground of `order` (0..3) of a stream: its j-mer counts, j = 1 .. order + 1, counted on the device.
    `stream` as in CRBM.scanSites (uint8 codes, 4 = no letter); gaps and record separators end a j-mer, so `offsets`
    play no role.  `model` is any CRBM: it lends its device."""
    order = _check_order(order)
    stream = _check_stream(stream)
    counts = np.zeros(kmer_slots(order), np.uint64)
    for lo, hi in _gap_cuts(stream, _MAX_T if _cut is None else int(_cut)):
        piece = stream[lo:hi]
        got = np.zeros(kmer_slots(order), np.uint64)
        model._call("crbm_stream_kmer_counts", piece.ctypes.data_as(_lib._U8P), piece.size, order, got.ctypes.data_as(_U64P))
        counts += got
    return MarkovBackground(order, counts)


def last_device_ms(model):
    """device time (HIP events around the kernels of every segment, summed) of the model's last fitBackground or
    sampleBackground call -- of its last piece, when the stream was cut"""
    ms = ctypes.c_float(0.0)
    model._call("crbm_background_ms", ctypes.byref(ms))
    return float(ms.value)


def sampleBackground(model, template, background, seed, pseudocount=1.0, _cut=None):
    """A stream drawn from a Markov background on the device, usable wherever sequences.shuffleStream's result is.
    `template`: a stream whose gaps (codes 4: N, record separators) are kept where they are -- the chain starts from the
    empty context behind each -- or an integer length (all letters).  `background`: a MarkovBackground (its
    thresholds(pseudocount)) or a raw (contexts, 3) uint32 threshold table.  `seed`: an integer; the same seed gives the
    same stream, letter p being a function of (seed, p, the context) alone (include/crbm_amd.h,
    crbm_background_sample).  Exact: no chunk of the stream is restarted from a marginal.  A template of more than
    2^31 - 1 codes is cut behind gaps."""
    if isinstance(background, MarkovBackground):
        table, order = check_table(background.thresholds(pseudocount))
    else:
        table, order = check_table(background)
    if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)):
        raise ValueError("seed must be an integer")
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    limit = _MAX_T if _cut is None else int(_cut)
    if isinstance(template, (int, np.integer)) and not isinstance(template, bool):
        T = int(template)
        if T < 0:
            raise ValueError("the length must not be negative")
        if T > limit:
            raise ValueError("a length above %d needs a template stream with gaps to cut behind" % limit)
        cuts, stream = [(0, T)], None
    else:
        stream = _check_stream(template)
        cuts = list(_gap_cuts(stream, limit))
        T = stream.size
    out = np.empty(T, np.uint8)
    for lo, hi in cuts:
        piece = None if stream is None else stream[lo:hi]
        model._call("crbm_background_sample", table.ctypes.data_as(_U32P), order, hi - lo, lo, seed,
                    None if piece is None else piece.ctypes.data_as(_lib._U8P), out[lo:hi].ctypes.data_as(_lib._U8P))
    return out
