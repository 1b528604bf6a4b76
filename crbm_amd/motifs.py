"""Motif comparison: which known motif is this one, and which learned motifs are copies of each other?

readMotifs reads JASPAR, bare four-row pfm and MEME minimal text files into a MotifSet; compareMotifs scores every
placement of every query on every target, in both orientations, on the device (crbm_motif_compare, crbm_compare.h) and
returns a MotifComparison with p-, E- and q-values.

The statistic is an overlap-only comparison in the manner of Gupta et al. 2007 (Tomtom): the columns of a placement that
face each other are scored, the overhanging ones are not.  A column pair scores an integer bin of its squared Euclidean
distance; the p-value of a placement is the exact tail of the sum of that many bins when the target columns are drawn
independently from the pool of all target columns.  It makes no claim of bit compatibility with the MEME suite's program:
scores, null and E-values follow the same idea, not the same arithmetic.

Limits.  Overlap-only scores: a short overlap with a few perfect columns can beat a long, good one; raise min_overlap.
The score range is fixed (0 .. bins - 1 per column pair over the largest possible distance), not fitted to the data.
Widths up to 64, DNA only.  Every output is a (K, N) array: 45 bytes per pair on the host.  The null of an overlap of l
columns resolves probabilities down to (1 / C)^l for a pool of C columns; once that reaches the subnormal range (below
about 1e-308) the far tail loses precision and finally reads 0, and such p-values compare as equal."""
import ctypes
import os

import numpy as np

from . import _lib

SCALE = 4096
MAX_WIDTH = 64
MIN_BINS, MAX_BINS = 2, 256
TARGET_TILE = 32                 # targets per block of the placement kernel (crbm_compare.h: TILE_DEFAULT)
OUTPUT_BYTES = 1 << 28           # compareMotifs cuts its queries into calls of at most this many output bytes
STRANDS = ("both", "given")
MATCH_DTYPE = np.dtype([("query", np.int32), ("target", np.int32), ("offset", np.int32), ("strand", np.int8), ("overlap", np.int32),
                        ("p_min", np.float64), ("pvalue", np.float64), ("evalue", np.float64), ("qvalue", np.float64)])

_DP = ctypes.POINTER(ctypes.c_double)
_I8P = ctypes.POINTER(ctypes.c_int8)
_U32P = ctypes.POINTER(ctypes.c_uint32)


def _matrix(m, what="a motif"):
    m = np.array(m, dtype=np.float64)
    if m.ndim != 2 or m.shape[0] != 4 or m.shape[1] < 1:
        raise ValueError("%s must be a (4, w) matrix, rows A, C, G, T" % what)
    if m.shape[1] > MAX_WIDTH:
        raise ValueError("%s is %d columns wide: at most %d" % (what, m.shape[1], MAX_WIDTH))
    if not np.all(np.isfinite(m)) or m.min() < 0 or np.any(np.abs(m.sum(axis=0) - 1.0) > 1e-6):
        raise ValueError("%s must be stochastic: entries in [0, 1], every column summing to 1" % what)
    return np.ascontiguousarray(m)


class MotifSet(object):
    """names (list of str) and matrices (list of (4, w) float64, rows A, C, G, T, every column summing to 1 within 1e-6),
    widths 1 .. 64"""

    def __init__(self, names, matrices):
        names, matrices = list(names), list(matrices)
        if len(names) != len(matrices):
            raise ValueError("as many names as matrices")
        if not matrices:
            raise ValueError("a MotifSet holds at least one motif")
        self.names = [str(n) for n in names]
        self.matrices = [_matrix(m, "motif %s" % n) for n, m in zip(self.names, matrices)]

    @classmethod
    def from_model(cls, model, name="mot"):
        """the model's getPFMs(), named as saveMotifs names them (<name>1, <name>2, ...)"""
        pfms = model.getPFMs()
        return cls(["%s%d" % (name, i + 1) for i in range(len(pfms))], pfms)

    def __len__(self):
        return len(self.matrices)

    def __getitem__(self, i):
        if isinstance(i, slice):
            return MotifSet(self.names[i], self.matrices[i])
        if isinstance(i, (list, tuple, np.ndarray)):
            return MotifSet([self.names[int(e)] for e in i], [self.matrices[int(e)] for e in i])
        return self.names[i], self.matrices[i]

    @property
    def widths(self):
        return np.array([m.shape[1] for m in self.matrices], np.int32)

    def reverse_complement(self):
        """columns reversed, A <-> T and C <-> G"""
        return MotifSet(self.names, [m[::-1, ::-1] for m in self.matrices])

    def quantised(self):
        """(cols, start): cols (total columns, 4) uint16 = clip(floor(p * 4096 + 0.5), 0, 4096), motif k in the rows
        [start[k], start[k + 1]); start (len + 1,) int32"""
        cols = np.concatenate([m.T for m in self.matrices], axis=0)
        cols = np.clip(np.floor(cols * SCALE + 0.5), 0, SCALE)
        start = np.concatenate([[0], np.cumsum(self.widths, dtype=np.int64)])
        return np.ascontiguousarray(cols, np.uint16), np.ascontiguousarray(start, np.int32)


# ---- readers -----------------------------------------------------------------------------------------------------------
def _fail(path, line, why):
    raise ValueError("%s, line %d: %s" % (path, line, why))


def _numbers(tokens, path, line):
    try:
        return [float(t) for t in tokens]
    except ValueError:
        _fail(path, line, "not a number")


def _finish(rows, pseudocount, path, line):
    """rows: four lists (A, C, G, T) -> (4, w), every column (v + pseudocount / 4) / (sum v + pseudocount)"""
    if len(rows) != 4:
        _fail(path, line, "a record has %d rows, not four" % len(rows))
    if len(set(len(r) for r in rows)) != 1 or not rows[0]:
        _fail(path, line, "a ragged record: the rows differ in length")
    v = np.array(rows, np.float64)
    if v.min() < 0 or not np.all(np.isfinite(v)):
        _fail(path, line, "a negative or non-finite entry")
    total = v.sum(axis=0)
    if np.any(total <= 0):
        _fail(path, line, "a column sums to 0")
    if v.shape[1] > MAX_WIDTH:
        _fail(path, line, "a motif of %d columns: at most %d" % (v.shape[1], MAX_WIDTH))
    return (v + pseudocount / 4.0) / (total + pseudocount)


def _read_meme(lines, path, pseudocount):
    names, mats, i = [], [], 0
    while i < len(lines):
        tok = lines[i].split()
        if not tok or tok[0] != "MOTIF":
            i += 1
            continue
        if len(tok) < 2:
            _fail(path, i + 1, "MOTIF without an id")
        name, at = tok[1], i + 1
        i += 1
        while i < len(lines) and not lines[i].strip().startswith("letter-probability matrix"):
            if lines[i].split()[:1] == ["MOTIF"]:
                _fail(path, at, "MOTIF %s has no letter-probability matrix" % name)
            i += 1
        if i == len(lines):
            _fail(path, at, "MOTIF %s has no letter-probability matrix" % name)
        head = lines[i].replace("=", "= ").split()
        fields = {head[j].rstrip("="): head[j + 1] for j in range(len(head) - 1) if head[j].endswith("=")}
        if fields.get("alength", "4") != "4":
            _fail(path, i + 1, "alength must be 4 (DNA)")
        w = int(fields["w"]) if "w" in fields else None
        i += 1
        rows = []
        while i < len(lines) and (w is None or len(rows) < w):
            tok = lines[i].split()
            if not tok or tok[0] in ("MOTIF", "URL") or (w is None and not tok[0][0].isdigit() and tok[0][0] != "."):
                break
            vals = _numbers(tok, path, i + 1)
            if len(vals) != 4:
                _fail(path, i + 1, "a ragged record: a row of %d numbers, not four" % len(vals))
            rows.append(vals)
            i += 1
        if not rows or (w is not None and len(rows) != w):
            _fail(path, at, "MOTIF %s: %d rows, w= %s" % (name, len(rows), w))
        names.append(name)
        mats.append(_finish([list(r) for r in zip(*rows)], pseudocount, path, at))
    if not names:
        _fail(path, 1, "no MOTIF record")
    return names, mats


def _read_rows(lines, path, pseudocount):
    """JASPAR records ('>ID NAME', then 'A [ ... ]' rows) and the bare four-row pfm (named after the file)"""
    names, mats = [], []
    name, rows, at = None, [], 1

    def close(line):
        if name is None and not rows:
            return
        names.append(name if name is not None else os.path.splitext(os.path.basename(path))[0])
        mats.append(_finish(rows, pseudocount, path, line))

    for n, raw in enumerate(lines, 1):
        text = raw.strip()
        if not text or text.startswith("#"):
            continue
        if text.startswith(">"):
            close(at)
            tok = text[1:].split()
            if not tok:
                _fail(path, n, "a header without an id")
            name, rows, at = (tok[1] if len(tok) > 1 else tok[0]), [], n
            continue
        if not rows and name is None:
            at = n
        tok = text.replace("[", " ").replace("]", " ").replace("|", " ").split()
        if tok and tok[0] in ("A", "C", "G", "T"):
            if tok[0] != "ACGT"[len(rows) % 4] or len(rows) >= 4:
                _fail(path, n, "rows must come as A, C, G, T, four per record")
            tok = tok[1:]
        elif len(rows) >= 4:
            _fail(path, n, "a record has more than four rows")
        rows.append(_numbers(tok, path, n))
    close(at)
    if not names:
        _fail(path, 1, "no motif")
    return names, mats


def _read_file(path, pseudocount):
    with open(path) as f:
        lines = f.read().splitlines()
    if any(l.split()[:1] == ["MOTIF"] for l in lines):
        return _read_meme(lines, path, pseudocount)
    return _read_rows(lines, path, pseudocount)


def readMotifs(path, pseudocount=0.0):
    """A MotifSet from one file, a list of files or a directory (its files in sorted order).  Formats, told apart by
    content: JASPAR ('>ID NAME', then four 'A [ ... ]' rows of counts or frequencies; many records per file; the motif
    is named NAME, or ID where there is none), the bare four-row pfm that saveMotifs writes (named after the file) and
    the MEME minimal text format ('MOTIF id', 'letter-probability matrix: alength= 4 w= ...', w rows of four numbers).
    Every column is normalised as (v + pseudocount / 4) / (sum v + pseudocount).  A column that sums to 0, a ragged
    record or a record with anything other than four rows raises ValueError with the file and line."""
    if not (isinstance(pseudocount, (int, float, np.floating, np.integer)) and not isinstance(pseudocount, bool)
            and np.isfinite(pseudocount) and pseudocount >= 0):
        raise ValueError("pseudocount must be a number >= 0")
    if isinstance(path, (list, tuple)):
        files = [str(p) for p in path]
    elif os.path.isdir(path):
        files = sorted(os.path.join(path, f) for f in os.listdir(path) if os.path.isfile(os.path.join(path, f)))
    else:
        files = [str(path)]
    if not files:
        raise ValueError("no motif file")
    names, mats = [], []
    for f in files:
        n, m = _read_file(f, float(pseudocount))
        names += n
        mats += m
    return MotifSet(names, mats)


# ---- the comparison ----------------------------------------------------------------------------------------------------
def benjamini_hochberg(p):
    """q-values of the last axis: q_(r) = min_{s >= r} p_(s) n / s over the ascending p_(1) .. p_(n)"""
    p = np.asarray(p, np.float64)
    n = p.shape[-1]
    order = np.argsort(p, axis=-1, kind="stable")
    ranked = np.take_along_axis(p, order, axis=-1) * n / np.arange(1, n + 1)
    ranked = np.minimum(np.minimum.accumulate(ranked[..., ::-1], axis=-1)[..., ::-1], 1.0)
    q = np.empty_like(ranked)
    np.put_along_axis(q, order, ranked, axis=-1)
    return q


def derive(p_min, n_off):
    """(pvalue, evalue, qvalue) of (K, N) p_min and n_off: pvalue = -expm1(n_off log1p(-p_min)), 1 where p_min is 1;
    evalue = pvalue N; qvalue by Benjamini-Hochberg over the N targets of each query"""
    p_min = np.asarray(p_min, np.float64)
    one = p_min >= 1.0
    with np.errstate(divide="ignore", invalid="ignore"):
        pvalue = np.where(one, 1.0, -np.expm1(np.asarray(n_off, np.float64) * np.log1p(-np.where(one, 0.0, p_min))))
    return pvalue, pvalue * p_min.shape[1], benjamini_hochberg(pvalue)


class MotifComparison(object):
    """(K, N) arrays p_min, pvalue, evalue, qvalue (float64), offset, overlap, n_off (int32), strand (int8, +1 / -1) and
    the name lists queries (K) and targets (N).  Target column j lies under query column j + offset.  p_min and the
    integers are the device's; pvalue, evalue and qvalue are derived from them on the host (derive) when first read."""

    FIELDS = ("p_min", "pvalue", "evalue", "qvalue", "offset", "strand", "overlap", "n_off")

    def __init__(self, queries, targets, p_min, offset, strand, overlap, n_off, bins=100, strands="both", min_overlap=1):
        self.queries, self.targets = [str(n) for n in queries], [str(n) for n in targets]
        shape = (len(self.queries), len(self.targets))
        self.p_min = np.ascontiguousarray(p_min, np.float64)
        self.offset, self.overlap, self.n_off = (np.ascontiguousarray(a, np.int32) for a in (offset, overlap, n_off))
        self.strand = np.ascontiguousarray(strand, np.int8)
        for name in ("p_min", "offset", "strand", "overlap", "n_off"):
            if getattr(self, name).shape != shape:
                raise ValueError("%s must be (queries, targets) = %r" % (name, shape))
        if shape[0] < 1 or shape[1] < 1:
            raise ValueError("at least one query and one target")
        if strands not in STRANDS:
            raise ValueError('strands must be "both" or "given"')
        self._derived = None
        self.bins, self.strands, self.min_overlap = int(bins), str(strands), int(min_overlap)

    def _derive(self):
        if self._derived is None:
            self._derived = derive(self.p_min, self.n_off)
        return self._derived

    @property
    def pvalue(self):
        return self._derive()[0]

    @property
    def evalue(self):
        return self._derive()[1]

    @property
    def qvalue(self):
        return self._derive()[2]

    def matches(self, evalue=10.0):
        """the pairs with an E-value of at most `evalue`, a structured array (MATCH_DTYPE: query and target as indices
        into the name lists) sorted by query, then p-value, then target"""
        k, t = np.nonzero(self.evalue <= evalue)
        order = np.lexsort((t, self.pvalue[k, t], k))
        k, t = k[order], t[order]
        out = np.zeros(k.size, MATCH_DTYPE)
        out["query"], out["target"] = k, t
        for name in ("offset", "strand", "overlap", "p_min", "pvalue", "evalue", "qvalue"):
            out[name] = getattr(self, name)[k, t]
        return out

    def best(self, n=1):
        """the n best targets of every query, by p-value (ties: the smaller index): a structured array of
        K * min(n, N) records, query after query"""
        n = max(1, min(int(n), len(self.targets)))
        t = np.argsort(self.pvalue, axis=1, kind="stable")[:, :n].reshape(-1)
        k = np.repeat(np.arange(len(self.queries)), n)
        out = np.zeros(k.size, MATCH_DTYPE)
        out["query"], out["target"] = k, t
        for name in ("offset", "strand", "overlap", "p_min", "pvalue", "evalue", "qvalue"):
            out[name] = getattr(self, name)[k, t]
        return out

    def save(self, path):
        """as .npz (numpy appends the extension when it is missing)"""
        np.savez(path, queries=np.array(self.queries, dtype=np.str_), targets=np.array(self.targets, dtype=np.str_), p_min=self.p_min,
                 offset=self.offset, strand=self.strand, overlap=self.overlap, n_off=self.n_off, bins=np.int64(self.bins),
                 strands=np.str_(self.strands), min_overlap=np.int64(self.min_overlap))

    @classmethod
    def load(cls, path):
        with np.load(path) as z:
            return cls([str(s) for s in z["queries"]], [str(s) for s in z["targets"]], z["p_min"], z["offset"], z["strand"], z["overlap"],
                       z["n_off"], int(z["bins"]), str(z["strands"]), int(z["min_overlap"]))


def _as_set(x, what):
    if isinstance(x, MotifSet):
        return x
    raise ValueError("%s must be a MotifSet (readMotifs, MotifSet.from_model)" % what)


def _check(bins, strands, min_overlap):
    if isinstance(bins, bool) or not isinstance(bins, (int, np.integer)) or not MIN_BINS <= bins <= MAX_BINS:
        raise ValueError("bins must be an integer in [2, 256]")
    if strands not in STRANDS:
        raise ValueError('strands must be "both" or "given"')
    if isinstance(min_overlap, bool) or not isinstance(min_overlap, (int, np.integer)) or min_overlap < 1:
        raise ValueError("min_overlap must be an integer >= 1")


def last_device_ms(model):
    """(total, (counts, null, placements)): device time of the model's last comparison call, and of its three stages"""
    ms, stages = ctypes.c_float(0.0), (ctypes.c_float * 3)()
    model._call("crbm_compare_ms", ctypes.byref(ms), stages)
    return float(ms.value), tuple(float(s) for s in stages)


def compareNull(model, query, targets, bins=100, strands="both"):
    """(counts, tails) of one query (a (4, w) matrix) against the pool of `targets` (a MotifSet): counts (w, bins) uint32,
    and tails, a dict {(i, l): P(score of the columns i .. i + l - 1 >= x), x = 0 .. l (bins - 1) + 1}"""
    _check(bins, strands, 1)
    q = MotifSet(["query"], [query])
    tcols, tstart = _as_set(targets, "targets").quantised()
    qcols, _ = q.quantised()
    m, both = int(q.widths[0]), int(strands == "both")
    counts = np.zeros((m, bins), np.uint32)
    tail = np.zeros(sum((m - l + 1) * (l * (bins - 1) + 2) for l in range(1, m + 1)), np.float64)
    model._call("crbm_motif_compare_null", qcols.ctypes.data_as(_lib._U16P), m, tcols.ctypes.data_as(_lib._U16P),
                tstart.ctypes.data_as(_lib._I32P), len(targets), int(bins), both, 1.0 / (len(tcols) * (1 + both)),
                counts.ctypes.data_as(_U32P), tail.ctypes.data_as(_DP))
    tails, at = {}, 0
    for i in range(m):
        for l in range(1, m - i + 1):
            tails[(i, l)] = tail[at:at + l * (bins - 1) + 2]
            at += l * (bins - 1) + 2
    return counts, tails


def compareMotifs(model, queries=None, targets=None, bins=100, strands="both", min_overlap=1):
    """Compare every query motif with every target motif on the device and return a MotifComparison.

    model: any CRBM; it lends its device.  queries: a MotifSet, or None for the model's own motifs
    (MotifSet.from_model).  targets: a MotifSet, or None for the queries themselves -- which learned motifs are copies of
    each other? -- with the diagonal computed like any pair.  bins: the score bins per column pair, 2 .. 256.
    strands: "both" also places every target's reverse complement (and its columns join the null's pool), "given" does
    not.  min_overlap: a placement counts when at least min(min_overlap, both widths) columns face each other."""
    _check(bins, strands, min_overlap)
    queries = MotifSet.from_model(model) if queries is None else _as_set(queries, "queries")
    targets = queries if targets is None else _as_set(targets, "targets")
    qcols, qstart = queries.quantised()
    tcols, tstart = targets.quantised()
    K, N, both = len(queries), len(targets), int(strands == "both")
    invC = 1.0 / (len(tcols) * (1 + both))
    p_min, strand = np.zeros((K, N), np.float64), np.zeros((K, N), np.int8)
    offset, overlap, n_off = (np.zeros((K, N), np.int32) for _ in range(3))
    per_call = max(1, OUTPUT_BYTES // (N * 21))
    for k0 in range(0, K, per_call):
        k1 = min(K, k0 + per_call)
        cols = np.ascontiguousarray(qcols[qstart[k0]:qstart[k1]])
        start = np.ascontiguousarray(qstart[k0:k1 + 1] - qstart[k0], np.int32)
        model._call("crbm_motif_compare", cols.ctypes.data_as(_lib._U16P), start.ctypes.data_as(_lib._I32P), k1 - k0,
                    tcols.ctypes.data_as(_lib._U16P), tstart.ctypes.data_as(_lib._I32P), N, int(bins), both, int(min(min_overlap, MAX_WIDTH)), invC,
                    p_min[k0:k1].ctypes.data_as(_DP), offset[k0:k1].ctypes.data_as(_lib._I32P), strand[k0:k1].ctypes.data_as(_I8P),
                    overlap[k0:k1].ctypes.data_as(_lib._I32P), n_off[k0:k1].ctypes.data_as(_lib._I32P))
    return MotifComparison(queries.names, targets.names, p_min, offset, strand, overlap, n_off, bins, strands, min_overlap)
