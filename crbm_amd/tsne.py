"""t-SNE embedding of row features on the device: the TSNE().fit_transform of the reference's runTSNE
(secomo/utils.py:159-160) without scikit-learn.

Exact k nearest neighbours, the conditional affinities and the gradient descent (exact O(n^2) repulsion, no tree, no
angle parameter) are HIP kernels behind crbm_tsne_neighbors / crbm_tsne_affinities / crbm_tsne_descend
(include/crbm_amd.h, crbm_amd/csrc/crbm_tsne.h); the symmetrisation of the affinities is a one-off of 2nk entries on
the host.  No float atomics: the same inputs and seed give the same bits in every run."""
import ctypes
import math
import time

import numpy as np

from ._lib import fptr, _I32P, _I64P

MAX_K = 1024          # crbm_tsne.h, KNN_MAX_K: a wave's neighbour list in the LDS
MAX_D = 256           # crbm_tsne.h, KNN_MAX_D
_EXPLORATION = 250    # iterations at the early exaggeration (scikit-learn's _EXPLORATION_MAX_ITER)
_KL_EVERY = 50


def symmetrize(idx, p):
    """Joint affinities as CSR from the neighbour lists idx (n, k) and the conditional p (n, k):
    P_ij = (p_{j|i} + p_{i|j}) / (2n) over the union of both directions.  Returns indptr (n + 1) int64, indices int32
    (ascending inside each row) and values float32.  Host, NumPy, deterministic: a stable sort of i * n + j over both
    directions, then np.add.reduceat over the runs of equal keys (a pair both rows list is added in float64, its own
    direction first)."""
    idx = np.asarray(idx)
    p = np.asarray(p)
    if idx.ndim != 2 or idx.shape != p.shape or idx.shape[1] < 1:
        raise ValueError("idx and p must both be (n, k)")
    n, k = idx.shape
    if n < 2:
        raise ValueError("t-SNE needs at least two rows")
    j = idx.astype(np.int64).ravel()
    if j.min() < 0 or j.max() >= n:
        raise ValueError("a neighbour index outside [0, n)")
    i = np.repeat(np.arange(n, dtype=np.int64), k)
    if np.any(i == j):
        raise ValueError("a row lists itself as a neighbour")
    keys = np.concatenate([i * n + j, j * n + i])
    vals = np.concatenate([p.ravel().astype(np.float64)] * 2)
    order = np.argsort(keys, kind="stable")
    keys, vals = keys[order], vals[order]
    first = np.flatnonzero(np.concatenate([[True], keys[1:] != keys[:-1]]))
    values = (np.add.reduceat(vals, first) / (2.0 * n)).astype(np.float32)
    keys = keys[first]
    rows = keys // n
    indptr = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(rows, minlength=n), out=indptr[1:])
    return indptr, (keys - rows * n).astype(np.int32), values


def _check_csr(n, indptr, indices, values):
    if indptr.shape != (n + 1,) or indptr[0] != 0 or np.any(np.diff(indptr) < 0):
        raise ValueError("indptr must have n + 1 entries, start at 0 and ascend")
    if indptr[-1] != indices.size or indices.size != values.size:
        raise ValueError("indptr must end at the number of values")
    if indices.size and (indices.min() < 0 or indices.max() >= n):
        raise ValueError("an index outside [0, n)")


def neighbors(model, X, k):
    """idx (n, k) int32 and d2 (n, k) float32 of crbm_tsne_neighbors: the k nearest other rows of X (n, D) by
    d2 = sum_d (x_id - x_jd)^2 in float32, ordered by (d2, j)."""
    X = np.ascontiguousarray(X, dtype=np.float32)
    if X.ndim != 2:
        raise ValueError("X must be (n, D)")
    n, D = X.shape
    k = int(k)
    if n < 2:
        raise ValueError("t-SNE needs at least two rows")
    if D < 1 or D > MAX_D:
        raise ValueError("D must lie in [1, %d]" % MAX_D)
    if k < 1 or k > n - 1:
        raise ValueError("k must lie in [1, n - 1]")
    if k > MAX_K:
        raise ValueError("k above %d: a wave's neighbour list does not fit the LDS" % MAX_K)
    if not np.isfinite(X).all():
        raise ValueError("X is not finite")
    idx = np.empty((n, k), np.int32)
    d2 = np.empty((n, k), np.float32)
    model._call("crbm_tsne_neighbors", fptr(X), n, D, k, idx.ctypes.data_as(_I32P), fptr(d2))
    return idx, d2


def affinities(model, d2, perplexity):
    """p (n, k) and beta (n) float32 of crbm_tsne_affinities: per row the beta at which exp(-beta d2) / sum has entropy
    log(perplexity), by bisection."""
    d2 = np.ascontiguousarray(d2, dtype=np.float32)
    if d2.ndim != 2:
        raise ValueError("d2 must be (n, k)")
    n, k = d2.shape
    perplexity = float(perplexity)
    if n < 2:
        raise ValueError("t-SNE needs at least two rows")
    if k < 1 or k > n - 1 or k > MAX_K:
        raise ValueError("k must lie in [1, min(n - 1, %d)]" % MAX_K)
    if not (math.isfinite(perplexity) and 0.0 < perplexity < k + 1):
        raise ValueError("the perplexity must be finite, positive and below k + 1")
    if not (np.isfinite(d2).all() and (d2 >= 0).all()):
        raise ValueError("a distance is negative or not finite")
    p = np.empty((n, k), np.float32)
    beta = np.empty(n, np.float32)
    model._call("crbm_tsne_affinities", fptr(d2), n, k, perplexity, fptr(p), fptr(beta))
    return p, beta


def descend(model, P, y, velocity, gains, iterations, exaggeration, learning_rate, momentum, want_grad=False, want_kl=False):
    """`iterations` steps of crbm_tsne_descend on the CSR P = (indptr, indices, values); y, velocity and gains (n, 2)
    float32 are updated in place.  Returns a dict with 'grad' (of the last iteration, if asked for) and 'kl', 'z' (at the
    y the last iteration started from, if asked for).  iterations = 0 evaluates at y and moves nothing."""
    indptr = np.ascontiguousarray(P[0], dtype=np.int64)
    indices = np.ascontiguousarray(P[1], dtype=np.int32)
    values = np.ascontiguousarray(P[2], dtype=np.float32)
    n = y.shape[0]
    for a in (y, velocity, gains):
        if a.dtype != np.float32 or a.shape != (n, 2) or not a.flags["C_CONTIGUOUS"]:
            raise ValueError("y, velocity and gains must be C-contiguous (n, 2) float32")
    if n < 2:
        raise ValueError("t-SNE needs at least two rows")
    if int(iterations) < 0:
        raise ValueError("iterations must not be negative")
    _check_csr(n, indptr, indices, values)
    grad = np.empty((n, 2), np.float32) if want_grad else None
    kl, z = ctypes.c_double(0.0), ctypes.c_double(0.0)
    model._call("crbm_tsne_descend", n, indptr.ctypes.data_as(_I64P), indices.ctypes.data_as(_I32P), fptr(values), fptr(y),
                fptr(velocity), fptr(gains), int(iterations), float(exaggeration), float(learning_rate), float(momentum),
                fptr(grad), ctypes.byref(kl) if want_kl else None, ctypes.byref(z) if want_kl else None)
    out = {}
    if want_grad:
        out["grad"] = grad
    if want_kl:
        out["kl"], out["z"] = kl.value, z.value
    return out


def _pca_init(X):
    """the first two principal components (host: the covariance is D x D), scaled so that the first has standard
    deviation 1e-4; each component's sign makes its largest loading positive"""
    Xc = X.astype(np.float64) - X.astype(np.float64).mean(axis=0)
    _, vecs = np.linalg.eigh(Xc.T @ Xc)
    comp = vecs[:, ::-1][:, :2]
    if comp.shape[1] < 2:                                   # D = 1: the second component is empty
        comp = np.concatenate([comp, np.zeros((comp.shape[0], 1))], axis=1)
    big = np.abs(comp).argmax(axis=0)
    comp = comp * np.where(comp[big, np.arange(2)] < 0, -1.0, 1.0)
    y = Xc @ comp
    sd = y[:, 0].std()
    return (y / sd * 1e-4 if sd > 0 else y).astype(np.float32)


def tsneEmbed(model, X, perplexity=30.0, early_exaggeration=12.0, learning_rate="auto", max_iter=1000, init="pca", seed=None,
              return_info=False):
    """Embed the rows of X (n, D) in the plane with t-SNE; returns (n, 2) float32.  `model` is any CRBM: it lends its
    device.  The defaults are those of scikit-learn's TSNE(): learning_rate 'auto' = max(n / early_exaggeration / 4, 50),
    250 iterations at the early exaggeration with momentum 0.5 and the rest at 1 and 0.8, init 'pca' (the first two
    principal components, the first scaled to standard deviation 1e-4), 'random' (1e-4 N(0, 1) from
    np.random.default_rng(seed)) or an (n, 2) array.  k = min(n - 1, floor(3 perplexity)) exact nearest neighbours by
    Euclidean distance; the repulsion is exact (all n^2 pairs), so there is no angle parameter.  All max_iter iterations
    run: scikit-learn's early stopping (on the gradient norm, and after 300 iterations without progress) is not
    reproduced.  return_info=True adds a dict with 'kl' (pairs (iteration, KL of P, never exaggerated, at the positions
    that iteration started from) for every 50th iteration, and (max_iter, KL of the returned y)), 'beta', 'k' and
    'seconds' for the four stages (neighbors, affinities, symmetrize, descend)."""
    X = np.ascontiguousarray(X, dtype=np.float32)
    if X.ndim != 2:
        raise ValueError("X must be (n, D)")
    n = X.shape[0]
    perplexity = float(perplexity)
    max_iter = int(max_iter)
    if n < 2:
        raise ValueError("t-SNE needs at least two rows")
    if not np.isfinite(X).all():
        raise ValueError("X is not finite")
    if not (math.isfinite(perplexity) and perplexity > 0.0):
        raise ValueError("the perplexity must be finite and positive")
    if perplexity >= n:
        raise ValueError("the perplexity must be below the number of rows")
    if max_iter < 0:
        raise ValueError("max_iter must not be negative")
    if not (float(early_exaggeration) >= 1.0):
        raise ValueError("early_exaggeration must be at least 1")
    k = min(n - 1, int(math.floor(3.0 * perplexity)))
    if k < 1 or k > MAX_K:
        raise ValueError("k = min(n - 1, floor(3 perplexity)) must lie in [1, %d]" % MAX_K)
    if learning_rate == "auto":
        lr = max(n / float(early_exaggeration) / 4.0, 50.0)
    else:
        lr = float(learning_rate)
        if not (math.isfinite(lr) and lr > 0.0):
            raise ValueError("learning_rate must be 'auto' or a positive number")
    if isinstance(init, str):
        if init == "pca":
            y = _pca_init(X)
        elif init == "random":
            y = (1e-4 * np.random.default_rng(seed).standard_normal((n, 2))).astype(np.float32)
        else:
            raise ValueError("init must be 'pca', 'random' or an (n, 2) array")
    else:
        y = np.array(init, dtype=np.float32, order="C")
        if y.shape != (n, 2) or not np.isfinite(y).all():
            raise ValueError("init must be a finite (n, 2) array: two components only")
    seconds = {}
    t = time.perf_counter()
    idx, d2 = neighbors(model, X, k)
    seconds["neighbors"] = time.perf_counter() - t
    t = time.perf_counter()
    p, beta = affinities(model, d2, perplexity)
    seconds["affinities"] = time.perf_counter() - t
    t = time.perf_counter()
    P = symmetrize(idx, p)
    seconds["symmetrize"] = time.perf_counter() - t
    t = time.perf_counter()
    velocity = np.zeros((n, 2), np.float32)
    gains = np.ones((n, 2), np.float32)
    first = min(_EXPLORATION, max_iter)
    kls = []
    done = 0
    for count, ex, mom in ((first, float(early_exaggeration), 0.5), (max_iter - first, 1.0, 0.8)):
        # pieces of 50 only when the KL is wanted: the state passes through the host exactly, so the bits are the same
        piece = _KL_EVERY if return_info else max(count, 1)
        while count > 0:
            step = min(piece, count)
            got = descend(model, P, y, velocity, gains, step, ex, lr, mom, want_kl=return_info)
            if return_info:
                kls.append((done + step - 1, got["kl"]))
            done += step
            count -= step
    seconds["descend"] = time.perf_counter() - t
    if not return_info:
        return y
    kls.append((max_iter, descend(model, P, y, velocity, gains, 0, 1.0, lr, 0.8, want_kl=True)["kl"]))
    return y, {"kl": kls, "beta": beta, "k": k, "seconds": seconds}
