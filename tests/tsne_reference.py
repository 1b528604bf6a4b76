"""float64 NumPy restatement of the t-SNE of crbm_amd/csrc/crbm_tsne.h, the yardstick of tests/test_gpu_tsne.py,
tests/test_emu_tsne.py and tests/test_tsne_reference.py (which pins it to scikit-learn's private functions, to a finite
difference of its own KL and to the planted data set).  Only the squared distances are float32, exactly as the kernel
takes them (difference form, d ascending, no fused multiply-add: the same bits); everything after is float64.

Also the data of those tests: feature rows with duplicates and distance ties, and the planted three-cluster set."""
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
