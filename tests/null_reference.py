"""The yardstick of the analytic null (crbm_amd.scoreDistribution, crbm_score_distribution): a float64 NumPy dynamic
programme in scatter form -- every (context, letter) pushes its mass to next_context, nothing of the kernel's gather
table -- the position weight matrix read off the oracle by probing it, a stationary distribution by power iteration, the
brute-force enumeration of all 4^M windows with their Markov probabilities, and check_tails, which holds tail bounds to
the enumeration by inequalities that need no tolerance."""
import itertools

import numpy as np

from oracle.crbm_oracle import onehot_of

SLACK = 1e-12                                                    # rounding of a sum of at most 4^6 probabilities


def contexts(order):
    return (4 ** (order + 1) - 1) // 3


def context_of(letters, order):
    """the index of the context of a letter history (oldest first): its last `order` letters, fewer when fewer exist"""
    tail = list(letters)[-order:] if order else []
    v = 0
    for a in tail:
        v = 4 * v + int(a)
    return (4 ** len(tail) - 1) // 3 + v


def letters_of(s):
    """the letters of context s, oldest first"""
    j = 0
    while s >= (4 ** (j + 1) - 1) // 3:
        j += 1
    v = s - (4 ** j - 1) // 3
    return [(v >> (2 * (j - 1 - i))) & 3 for i in range(j)]


def next_context(order, s, a):
    return context_of(letters_of(s) + [a], order)


def dirichlet_probabilities(order, seed):
    return np.random.default_rng(seed).dirichlet(np.ones(4), size=contexts(order))


def stationary(P, order, iters=20000):
    """power iteration on the full-length contexts (averaged over two steps, so that a periodic chain settles too)"""
    NS, base = contexts(order), (4 ** order - 1) // 3
    pi = np.zeros(NS)
    pi[base:] = 1.0 / (NS - base)
    nxt = np.array([[next_context(order, s, a) for a in range(4)] for s in range(NS)])

    def step(v):
        out = np.zeros(NS)
        np.add.at(out, nxt, v[:, None] * P)
        return out
    for _ in range(iters):
        one = step(pi)
        new = 0.5 * (one + step(one))
        new /= new.sum()
        if np.abs(new - pi).max() < 1e-16:
            pi = new
            break
        pi = new
    return pi


def start(P, order, kind):
    if kind == "run":
        init = np.zeros(contexts(order))
        init[0] = 1.0
        return init
    return stationary(P, order)


def quantise(w, c, step):
    """the contract's quantisation of one row: w (M, 4), c scalar -> q (M, 4) int64, offset, err, G"""
    q0 = np.rint(np.asarray(w, np.float64) / step)
    err = float(np.abs(w - step * q0).max(axis=1).sum())
    low = q0.min(axis=1, keepdims=True)
    q = (q0 - low).astype(np.int64)
    return q, float(c + step * low.sum()), err, int(q.max(axis=1).sum()) + 1


def dp(q, P, init, order):
    """pmf (G,) float64 of the integer score of one row q (M, 4) >= 0: scatter over next_context"""
    q = np.asarray(q, np.int64)
    M, NS = q.shape[0], contexts(order)
    G = int(q.max(axis=1).sum()) + 1
    f = np.zeros((NS, G))
    f[:, 0] = init
    for j in range(M):
        g = np.zeros((NS, G))
        for s in range(NS):
            if not f[s].any():
                continue
            for a in range(4):
                d = int(q[j, a])
                g[next_context(order, s, a), d:] += P[s, a] * f[s, :G - d]
        f = g
    return f.sum(axis=0)


def window_pwm(o):
    """(w, c): w (R, M, 4), c (R,) float64, rows r = k * S + s, read off the oracle's activations of one-hot windows of
    length M: the score is affine in the one-hot input, so the all-A window and the 3 M single substitutions fix it"""
    M, K = o.motif_length, o.num_motifs

    def scores(letters):
        D = onehot_of(np.asarray(letters)[None, :])
        fwd, rev = o._bottomUpActivity(D)[0, :, 0, 0], o._bottomUpActivity(D, True)[0, :, 0, 0]
        return np.stack([fwd, rev], axis=1) if o.doublestranded else (fwd + rev)[:, None]      # (K, S)
    base = scores(np.zeros(M, np.int64))
    S = base.shape[1]
    w = np.zeros((K, S, M, 4))
    for j in range(M):
        for a in range(1, 4):
            letters = np.zeros(M, np.int64)
            letters[j] = a
            w[:, :, j, a] = scores(letters) - base
    return w.reshape(K * S, M, 4), base.reshape(K * S).astype(np.float64)


def enumerate_windows(w, c, P, init, order):
    """(x, p): the score c + sum_j w[j][a_j] and the Markov probability of every one of the 4^M windows of one row"""
    M = w.shape[0]
    letters = np.array(list(itertools.product(range(4), repeat=M)), np.int64)               # (4^M, M)
    nxt = np.array([[next_context(order, s, a) for a in range(4)] for s in range(contexts(order))])
    xs, ps = [], []
    for s0 in np.flatnonzero(init):
        s = np.full(letters.shape[0], s0, np.int64)
        p = np.full(letters.shape[0], float(init[s0]))
        x = np.full(letters.shape[0], float(c))
        for j in range(M):
            a = letters[:, j]
            p = p * P[s, a]
            x = x + w[j, a]
            s = nxt[s, a]
        xs.append(x)
        ps.append(p)
    return np.concatenate(xs), np.concatenate(ps)


def exact_tail(x, p, t):
    """P(X >= t) of the enumeration, t an array"""
    order = np.argsort(x)
    xs, cum = x[order], np.concatenate([[0.0], np.cumsum(p[order])])
    return cum[-1] - cum[np.searchsorted(xs, t, side="left")]


def grid_tail(pmf, offset, step, t):
    """P(offset + step Q >= t), t an array"""
    tail = np.concatenate([np.cumsum(pmf[::-1])[::-1], [0.0]])
    n = np.clip(np.ceil((np.asarray(t, np.float64) - offset) / step), 0, pmf.size).astype(np.int64)
    return tail[n]


def check_tails(lower, upper, x, p, t, err):
    """lower and upper (arrays over the thresholds t) against the enumeration (x, p) of one row:
         lower <= P(X >= t) <= upper,   upper <= P(X >= t - 2 err),   lower >= P(X >= t + 2 err).
    Rigorous for bounds taken at t + err and t - err from a grid within err of every score; SLACK covers the rounding of
    the sums."""
    t = np.asarray(t, np.float64)
    exact = exact_tail(x, p, t)
    assert np.all(lower <= exact + SLACK), ("lower above the exact tail", float((lower - exact).max()))
    assert np.all(exact <= upper + SLACK), ("upper below the exact tail", float((exact - upper).max()))
    wide = 2.0 * err
    assert np.all(upper <= exact_tail(x, p, t - wide) + SLACK), "upper is looser than the quantisation allows"
    assert np.all(lower >= exact_tail(x, p, t + wide) - SLACK), "lower is looser than the quantisation allows"
