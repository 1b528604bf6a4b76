"""NumPy restatement of the motif comparison of crbm_amd/csrc/crbm_compare.h, the yardstick of tests/test_gpu_compare.py,
tests/test_emu_compare.py and tools/bench_compare.py.  Everything is an integer up to the counts; from there one pinned
float64 order: col = count * invC, every cell of a convolution added in ascending y from 0.0, the tails by np.cumsum on
the reversed pmf (a sequential sum, x descending).  The device has to give the same bits.

A motif is a (4, w) float64 matrix, rows A, C, G, T, columns summing to 1; quantised it is (w, 4) uint16."""
import itertools
from fractions import Fraction

import numpy as np

SCALE = 4096
MAX_WIDTH = 64


def quantise(p):
    """(4, w) probabilities -> (w, 4) uint16: clip(floor(p * 4096 + 0.5), 0, 4096)"""
    x = np.floor(np.asarray(p, np.float64) * SCALE + 0.5)
    return np.ascontiguousarray(np.clip(x, 0, SCALE).T.astype(np.uint16))


def reverse_complement(q):
    """of a quantised (w, 4) motif: columns reversed, A <-> T and C <-> G"""
    return np.ascontiguousarray(q[::-1, ::-1])


def bins_of(a, b, B):
    """(len a, len b) int64: the bin of every column of a against every column of b"""
    d = a.astype(np.int64)[:, None, :] - b.astype(np.int64)[None, :, :]
    D = (d * d).sum(axis=2)
    sim = (1 << 25) - np.minimum(D, 1 << 25)
    return (sim * (B - 1) + (1 << 24)) >> 25


def pool_of(targets, both):
    """every column of every (quantised) target, and of every reverse complement with both"""
    cols = np.concatenate(list(targets), axis=0)
    return np.concatenate([cols, cols[:, ::-1]], axis=0) if both else cols


def counts_of(query, pool, B):
    """(m, B) uint32: the pool columns whose bin against query column i is y"""
    b = bins_of(query, pool, B)
    return np.stack([np.bincount(row, minlength=B) for row in b]).astype(np.uint32)


def tails_of(counts, invC):
    """{(i, l): tail_{i,l}, G_l + 1 float64} for 1 <= l <= m - i"""
    m, B = counts.shape
    col = counts.astype(np.float64) * np.float64(invC)
    out = {}
    for i in range(m):
        pmf = np.ones(1)
        for l in range(1, m - i + 1):
            nxt = np.zeros(l * (B - 1) + 1)
            for y in range(B):                                   # ascending y: every cell gains its terms in that order
                nxt[y:y + pmf.size] += pmf * col[i + l - 1, y]
            pmf = nxt
            out[(i, l)] = np.concatenate([np.cumsum(pmf[::-1])[::-1], [0.0]])
    return out


def pmfs_of(counts, invC):
    """{(i, l): pmf_{i,l}} -- the same programme, for the tests of the restatement itself"""
    m, B = counts.shape
    col = counts.astype(np.float64) * np.float64(invC)
    out = {}
    for i in range(m):
        pmf = np.ones(1)
        for l in range(1, m - i + 1):
            nxt = np.zeros(l * (B - 1) + 1)
            for y in range(B):
                nxt[y:y + pmf.size] += pmf * col[i + l - 1, y]
            pmf = nxt
            out[(i, l)] = pmf
    return out


def packed(tails, m):
    """the layout of crbm_motif_compare_null: start i ascending, then l ascending"""
    return np.concatenate([tails[(i, l)] for i in range(m) for l in range(1, m - i + 1)])


def pair(query, target, tails, B, both, min_overlap):
    """(p_min, offset, strand, overlap, n_off) of one (query, target)"""
    m, n = len(query), len(target)
    need = min(min_overlap, m, n)
    best, n_off = None, 0
    for strand, t in ((1, target), (-1, reverse_complement(target)))[:2 if both else 1]:
        b = bins_of(query, t, B)
        for o in range(-(n - 1), m):
            i0, j0 = max(0, o), max(0, -o)
            l = min(m - i0, n - j0)
            if l < need:
                continue
            n_off += 1
            S = int(sum(b[i0 + t_, j0 + t_] for t_ in range(l)))
            p = tails[(i0, l)][S]
            if best is None or p < best[0]:                      # strands and offsets come in the tie order: the first stays
                best = (p, o, strand, l)
    return best + (n_off,)


def compare(queries, targets, bins=100, both=True, min_overlap=1):
    """queries, targets: lists of quantised motifs.  Returns a dict of (K, N) arrays p_min, offset, strand, overlap, n_off
    and the lists `counts` and `tails` per query."""
    K, N = len(queries), len(targets)
    pool = pool_of(targets, both)
    invC = 1.0 / pool.shape[0]
    out = dict(p_min=np.zeros((K, N)), offset=np.zeros((K, N), np.int32), strand=np.zeros((K, N), np.int8),
               overlap=np.zeros((K, N), np.int32), n_off=np.zeros((K, N), np.int32), counts=[], tails=[], invC=invC)
    for k, q in enumerate(queries):
        counts = counts_of(q, pool, bins)
        tails = tails_of(counts, invC)
        out["counts"].append(counts)
        out["tails"].append(tails)
        for t, target in enumerate(targets):
            p, o, s, l, n_off = pair(q, target, tails, bins, both, min_overlap)
            out["p_min"][k, t], out["offset"][k, t], out["strand"][k, t], out["overlap"][k, t], out["n_off"][k, t] = p, o, s, l, n_off
    return out


def derive(p_min, n_off):
    """(pvalue, evalue, qvalue) of (K, N) p_min and n_off, as compareMotifs derives them on the host"""
    p_min = np.asarray(p_min, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        pvalue = np.where(p_min >= 1.0, 1.0, -np.expm1(n_off * np.log1p(-np.minimum(p_min, 1.0))))
    N = p_min.shape[1]
    return pvalue, pvalue * N, np.stack([benjamini_hochberg(row) for row in pvalue])


def benjamini_hochberg(p):
    p = np.asarray(p, np.float64)
    n = p.size
    order = np.argsort(p, kind="stable")
    q = np.empty(n)
    running = 1.0
    for rank in range(n, 0, -1):
        e = order[rank - 1]
        running = min(running, p[e] * n / rank)
        q[e] = running
    return q


def brute_force_tails(query, pool, B, i, l):
    """tail_{i,l} as exact fractions: every one of the C^l tuples of pool columns, each with probability C^-l"""
    b = bins_of(query, pool, B)
    C = pool.shape[0]
    hist = [0] * (l * (B - 1) + 1)
    for tup in itertools.product(range(C), repeat=l):
        hist[sum(int(b[i + t, c]) for t, c in enumerate(tup))] += 1
    tail, acc = [Fraction(0)] * (len(hist) + 1), Fraction(0)
    for x in range(len(hist) - 1, -1, -1):
        acc += Fraction(hist[x], C ** l)
        tail[x] = acc
    return tail


def dirichlet_motif(rng, w, alpha=0.3):
    """(4, w) float64 with Dirichlet(alpha) columns"""
    return np.ascontiguousarray(rng.dirichlet(np.full(4, alpha), size=w).T)
