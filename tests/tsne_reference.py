"""float64 NumPy restatement of the t-SNE of crbm_amd/csrc/crbm_tsne.h, the yardstick of tests/test_gpu_tsne.py,
tests/test_emu_tsne.py and tests/test_tsne_reference.py (which pins it to scikit-learn's private functions, to a finite
difference of its own KL and to the planted data set).  Only the squared distances are float32, exactly as the kernel
takes them (difference form, d ascending, no fused multiply-add: the same bits); everything after is float64.
kl_gradient is the dense one; kl_gradient_csr (row blocks, no n x n array) and kl_gradient_grouped (rows on few distinct
positions) are pinned to it and serve the large shapes.  The host rules of the header (slice_tiles, slices, sum_chunks,
knn_lds_bytes, the waves per block) are restated at the end, for a test to assert which path its shape takes.

Also the data of those tests: feature rows with duplicates and distance ties, descending rows (every candidate goes to
the head of the neighbour list), the planted three-cluster set, and a sparse symmetric P of any size."""
import numpy as np

EPS = 2.2e-16
STEPS = 100


# ---- data ---------------------------------------------------------------------------------------------------------------
def feature_rows(n, D, seed, eighths=False, duplicates=12):
    """uniform [0, 1) float32 rows; `eighths`: rounded to multiples of 1/8 (many distance ties); the rows
    3, 8, 13, ... (`duplicates` of them, as many as fit) are copies of row 3: zero distances and ties by index"""
    rng = np.random.default_rng(seed)
    X = rng.random((n, D), dtype=np.float32)
    if eighths:
        X = (np.round(X * 8) / 8).astype(np.float32)
    dup = np.arange(3, n, 5)[:duplicates]
    if dup.size > 1:
        X[dup] = X[dup[0]]
    return X


def descending_rows(n):
    """(n, 1): x_i = 0.25 (n - i), exact in float32.  Every row is nearer to the rows before row j than row j is, so in
    the neighbour kernel's scan (j ascending) each candidate of rows i > j displaces the head of the list: the longest
    shift the list can make, at every insertion.  i - m and i + m tie and go by index."""
    return (0.25 * (n - np.arange(n, dtype=np.float32)))[:, None].astype(np.float32)


def planted(n, D=10, seed=0):
    """three centres uniform in [0.1, 0.9]^D; row i = centre of i mod 3 + 0.05 N(0, 1), clipped to [0, 1]"""
    rng = np.random.default_rng(seed)
    centres = rng.uniform(0.1, 0.9, size=(3, D))
    labels = np.arange(n) % 3
    X = np.clip(centres[labels] + 0.05 * rng.standard_normal((n, D)), 0.0, 1.0).astype(np.float32)
    return X, labels


# ---- a. neighbours ------------------------------------------------------------------------------------------------------
def d2_matrix(X):
    """(n, n) float32: sum over d ascending of (x_id - x_jd)^2, every operation rounded to float32"""
    X = np.ascontiguousarray(X, np.float32)
    n, D = X.shape
    acc = np.zeros((n, n), np.float32)
    for d in range(D):
        diff = X[:, d][:, None] - X[:, d][None, :]
        acc = acc + diff * diff
    return acc


def neighbors(X, k):
    """idx (n, k) int32 and d2 (n, k) float32: the k nearest other rows by (d2, j) ascending"""
    d2 = d2_matrix(X)
    n = d2.shape[0]
    assert 1 <= k <= n - 1
    order = np.argsort(d2, axis=1, kind="stable")                    # ties by j ascending
    keep = order != np.arange(n)[:, None]                              # self out, wherever the sort put it
    idx = order[keep].reshape(n, n - 1)[:, :k]
    return idx.astype(np.int32), np.take_along_axis(d2, idx, axis=1)


# ---- b. affinities ------------------------------------------------------------------------------------------------------
def entropy(d2, beta):
    """entropy of p_j ~ exp(-beta d2_j) per row, float64, the row's smallest d2 subtracted inside the exponent"""
    dd = np.asarray(d2, np.float64)
    dd = dd - dd.min(axis=1, keepdims=True)
    e = np.exp(-np.asarray(beta, np.float64)[:, None] * dd)
    S = e.sum(axis=1)
    return np.log(S) + np.asarray(beta, np.float64) * (dd * e).sum(axis=1) / S


def conditional(d2, beta):
    dd = np.asarray(d2, np.float64)
    dd = dd - dd.min(axis=1, keepdims=True)
    e = np.exp(-np.asarray(beta, np.float64)[:, None] * dd)
    return e / e.sum(axis=1, keepdims=True)


def affinities(d2, perplexity, steps=STEPS, tol=0.0):
    """beta (n) and p (n, k) float64 by bisection from beta = 1, doubling or halving while a bound is open, `steps`
    evaluations.  tol > 0 stops a row once |H - log(perplexity)| <= tol (what scikit-learn does, at 1e-5); the kernel
    and the default do not stop."""
    d2 = np.asarray(d2, np.float64)
    n = d2.shape[0]
    target = np.log(perplexity)
    beta = np.ones(n)
    lo = np.full(n, -np.inf)
    hi = np.full(n, np.inf)
    done = np.zeros(n, bool)
    for _ in range(steps):
        H = entropy(d2, beta)
        diff = H - target
        done |= np.abs(diff) <= tol if tol > 0 else False
        up = (diff > 0) & ~done
        down = ~(diff > 0) & ~done
        lo = np.where(up, beta, lo)
        hi = np.where(down, beta, hi)
        with np.errstate(invalid="ignore", over="ignore"):
            nb = np.where(up, np.where(np.isinf(hi), beta * 2.0, 0.5 * (beta + hi)),
                          np.where(np.isinf(lo), beta * 0.5, 0.5 * (beta + lo)))
        beta = np.where(done, beta, nb)
    return beta, conditional(d2, beta)


def reachable(d2, perplexity):
    """rows for which some beta gives entropy log(perplexity): the entropy falls from log k (beta -> 0) to log m
    (beta -> inf), m = how many distances tie for the smallest.  A row of equal distances (m = k) reaches nothing."""
    d2 = np.asarray(d2)
    m = (d2 == d2.min(axis=1, keepdims=True)).sum(axis=1)
    return (m < perplexity) & (perplexity < d2.shape[1])


# ---- symmetrisation -----------------------------------------------------------------------------------------------------
def symmetrize_dense(idx, p):
    """(n, n) float64: P_ij = (p_{j|i} + p_{i|j}) / 2n over the union of both directions"""
    n = idx.shape[0]
    C = np.zeros((n, n))
    np.put_along_axis(C, idx.astype(np.int64), np.asarray(p, np.float64), axis=1)
    return (C + C.T) / (2.0 * n)


def dense_to_csr(P):
    """CSR of the entries that are not zero: indptr int64, indices int32 (ascending in a row), values float64"""
    n = P.shape[0]
    rows, cols = np.nonzero(P)
    indptr = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(rows, minlength=n), out=indptr[1:])
    return indptr, cols.astype(np.int32), P[rows, cols]


def csr_to_dense(n, indptr, indices, values):
    P = np.zeros((n, n))
    rows = np.repeat(np.arange(n), np.diff(indptr))
    P[rows, indices] = values
    return P


# ---- c. KL, gradient, update --------------------------------------------------------------------------------------------
def kl_gradient(P, y, exaggeration=1.0, want_kl=True):
    """dict: kl = sum P log(max(P, eps) / max(w / Z, eps)) (P as given), grad = 4 (exaggeration A - R / Z), and the
    parts z, A (n, 2), R (n, 2) -- float64, dense P (n, n)"""
    y = np.asarray(y, np.float64)
    dx = y[:, 0][:, None] - y[:, 0][None, :]
    dy = y[:, 1][:, None] - y[:, 1][None, :]
    w = 1.0 / (1.0 + dx * dx + dy * dy)
    np.fill_diagonal(w, 0.0)
    Z = w.sum()
    pw, ww = P * w, w * w
    A = np.stack([(pw * dx).sum(axis=1), (pw * dy).sum(axis=1)], axis=1)
    R = np.stack([(ww * dx).sum(axis=1), (ww * dy).sum(axis=1)], axis=1)
    kl = None
    if want_kl:
        nz = P > 0
        wz = (w / Z)[nz]
        kl = float((P[nz] * np.log(np.maximum(P[nz], EPS) / np.maximum(wz, EPS))).sum())
    return {"kl": kl, "z": float(Z), "A": A, "R": R, "grad": 4.0 * (exaggeration * A - R / Z)}


def _attraction_csr(csr, y, Z, want_kl):
    """A (n, 2) and the KL of a CSR P at y (float64), w / Z the q of the pairs"""
    indptr, indices, values = csr
    n = y.shape[0]
    rows = np.repeat(np.arange(n), np.diff(indptr))
    cols = np.asarray(indices, np.int64)
    p = np.asarray(values, np.float64)
    dx, dy = y[rows, 0] - y[cols, 0], y[rows, 1] - y[cols, 1]
    w = 1.0 / (1.0 + dx * dx + dy * dy)
    pw = p * w
    A = np.stack([np.bincount(rows, pw * dx, minlength=n), np.bincount(rows, pw * dy, minlength=n)], axis=1)
    kl = None
    if want_kl:
        nz = p > 0
        kl = float((p[nz] * np.log(np.maximum(p[nz], EPS) / np.maximum(w[nz] / Z, EPS))).sum())
    return A, kl


def kl_gradient_csr(csr, y, exaggeration=1.0, want_kl=True, block=256):
    """kl_gradient from a CSR P = (indptr, indices, values): the same dict, float64.  The repulsion goes in blocks of
    `block` rows against all n (five float64 arrays of block x n: 170 MB at n = 16 385), so no n x n array is ever built"""
    y = np.asarray(y, np.float64)
    n = y.shape[0]
    R = np.zeros((n, 2))
    s = np.zeros(n)
    for i0 in range(0, n, block):
        i1 = min(i0 + block, n)
        dx = y[i0:i1, 0][:, None] - y[:, 0][None, :]
        dy = y[i0:i1, 1][:, None] - y[:, 1][None, :]
        w = 1.0 / (1.0 + dx * dx + dy * dy)
        w[np.arange(i1 - i0), np.arange(i0, i1)] = 0.0
        s[i0:i1] = w.sum(axis=1)
        w *= w
        R[i0:i1, 0] = (w * dx).sum(axis=1)
        R[i0:i1, 1] = (w * dy).sum(axis=1)
    Z = float(s.sum())
    A, kl = _attraction_csr(csr, y, Z, want_kl)
    return {"kl": kl, "z": Z, "A": A, "R": R, "grad": 4.0 * (exaggeration * A - R / Z)}


def kl_gradient_grouped(csr, points, group, exaggeration=1.0, want_kl=True):
    """kl_gradient_csr at y = points[group], whose rows take only G = len(points) distinct positions: s_i and R_i depend on
    the group alone, s_g = sum_h c_h w_gh - 1 (the row itself out; the others at its position count with w = 1) and
    R_g = sum_h c_h w_gh^2 (p_g - p_h), c_h the rows of group h -- O(G^2), float64, exact"""
    pts = np.asarray(points, np.float64)
    group = np.asarray(group, np.int64)
    c = np.bincount(group, minlength=pts.shape[0]).astype(np.float64)
    dx = pts[:, 0][:, None] - pts[:, 0][None, :]
    dy = pts[:, 1][:, None] - pts[:, 1][None, :]
    w = 1.0 / (1.0 + dx * dx + dy * dy)
    s = (w * c[None, :]).sum(axis=1) - 1.0
    ww = w * w * c[None, :]
    Rg = np.stack([(ww * dx).sum(axis=1), (ww * dy).sum(axis=1)], axis=1)
    Z = float((c * s).sum())
    y = pts[group]
    A, kl = _attraction_csr(csr, y, Z, want_kl)
    R = Rg[group]
    return {"kl": kl, "z": Z, "A": A, "R": R, "grad": 4.0 * (exaggeration * A - R / Z)}


def at_exaggeration(ref, exaggeration):
    """the dict of kl_gradient* with its gradient at another exaggeration (A, R, Z and the KL do not depend on it)"""
    return dict(ref, grad=4.0 * (exaggeration * ref["A"] - ref["R"] / ref["z"]))


def sparse_joint(n, seed, per_row=6, empty_row=None):
    """a symmetric CSR P (indptr int64, indices int32 ascending in a row, values float32) that sums to 1, built without
    an n x n array: every row draws `per_row` partners, the pairs are taken in both directions with one float32 value
    each, so rows have unequal lengths.  Rows 0 and n - 1 are partners: attraction reaches across the whole y buffer.
    `empty_row` has no entries and is nobody's partner."""
    assert n >= 4 and empty_row not in (0, n - 1)
    rng = np.random.default_rng(seed)
    i = np.repeat(np.arange(n, dtype=np.int64), per_row)
    j = rng.integers(0, n, size=i.size, dtype=np.int64)
    i, j = np.append(i, 0), np.append(j, n - 1)
    keep = i != j
    if empty_row is not None:
        keep &= (i != empty_row) & (j != empty_row)
    i, j = i[keep], j[keep]
    pairs = np.unique(np.minimum(i, j) * n + np.maximum(i, j))
    lo, hi = pairs // n, pairs % n
    v = rng.uniform(0.2, 1.0, size=pairs.size)
    v = (v / (2.0 * v.sum())).astype(np.float32)                       # each pair twice: the whole sums to 1
    rows, cols, vals = np.concatenate([lo, hi]), np.concatenate([hi, lo]), np.concatenate([v, v])
    order = np.argsort(rows * n + cols, kind="stable")
    rows, cols, vals = rows[order], cols[order], vals[order]
    indptr = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(rows, minlength=n), out=indptr[1:])
    length = np.diff(indptr)
    assert np.unique(length).size > 1, "rows of unequal length"
    assert cols[indptr[1] - 1] == n - 1 and cols[indptr[n - 1]] == 0
    assert empty_row is None or (length[empty_row] == 0 and not (cols == empty_row).any())
    assert abs(float(vals.astype(np.float64).sum()) - 1.0) < 1e-6
    return indptr, cols.astype(np.int32), vals


# ---- the header's host rules, restated: a test asserts with them that its shape takes the path it is meant to take --------
TJ, SUM_CHUNK, MAX_SLICES, KNN_TILE = 256, 256, 64, 64


def slice_tiles(n):
    tiles = (n + TJ - 1) // TJ
    want = min((2048 + tiles - 1) // tiles, MAX_SLICES, tiles)
    return (tiles + want - 1) // want


def slices(n):
    tiles = (n + TJ - 1) // TJ
    return (tiles + slice_tiles(n) - 1) // slice_tiles(n)


def sum_chunks(n):
    return (n + SUM_CHUNK - 1) // SUM_CHUNK


def knn_lds_bytes(D, k, waves):
    return ((KNN_TILE + waves) * (D | 1) + waves * k * 2) * 4


def knn_launch(D, k):
    """(waves per block, bytes of LDS) of crbm_tsne_neighbors: eight waves, halved while the request is above 128 KB"""
    waves = 8
    while waves > 1 and knn_lds_bytes(D, k, waves) > 128 * 1024:
        waves >>= 1
    return waves, knn_lds_bytes(D, k, waves)


def update(y, velocity, gains, grad, learning_rate, momentum):
    """scikit-learn's rule; returns the new y, velocity, gains"""
    inc = velocity * grad < 0.0
    gains = np.maximum(np.where(inc, gains + 0.2, gains * 0.8), 0.01)
    velocity = momentum * velocity - learning_rate * gains * grad
    return y + velocity, velocity, gains


def descend(P, y, velocity, gains, iterations, exaggeration, learning_rate, momentum):
    for _ in range(iterations):
        g = kl_gradient(P, y, exaggeration, want_kl=False)["grad"]
        y, velocity, gains = update(y, velocity, gains, g, learning_rate, momentum)
    return y, velocity, gains


def embed(X, perplexity=30.0, early_exaggeration=12.0, learning_rate="auto", max_iter=1000, seed=None, y0=None):
    """the driver with scikit-learn's schedule: 250 iterations at the early exaggeration with momentum 0.5, the rest at
    1 and 0.8; y0 or 1e-4 N(0, 1) from default_rng(seed).  Returns y and the final KL (float64, dense P)."""
    n = X.shape[0]
    k = min(n - 1, int(3.0 * perplexity))
    idx, d2 = neighbors(X, k)
    _, p = affinities(d2, perplexity)
    P = symmetrize_dense(idx, p)
    lr = max(n / early_exaggeration / 4.0, 50.0) if learning_rate == "auto" else float(learning_rate)
    y = 1e-4 * np.random.default_rng(seed).standard_normal((n, 2)) if y0 is None else np.array(y0, np.float64)
    v, g = np.zeros((n, 2)), np.ones((n, 2))
    first = min(250, max_iter)
    y, v, g = descend(P, y, v, g, first, early_exaggeration, lr, 0.5)
    y, v, g = descend(P, y, v, g, max_iter - first, 1.0, lr, 0.8)
    return y, kl_gradient(P, y)["kl"], P


def neighbour_purity(y, labels):
    """share of the points whose nearest neighbour in the plane carries their own label"""
    y = np.asarray(y, np.float64)
    d = ((y[:, None, :] - y[None, :, :]) ** 2).sum(axis=2)
    np.fill_diagonal(d, np.inf)
    return float((labels[d.argmin(axis=1)] == labels).mean())
