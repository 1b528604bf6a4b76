"""TEST INFRASTRUCTURE: the float64 yardstick of annealed importance sampling (crbm_ais, CRBM.logPartition), built on
OracleCRBM and the oracle's Philox uniforms with two kinds of their own.  Any alphabet, no pooling.

    log p*_beta(v) = sum_{strands,k,s} softplus(beta x[k,s](v)) + sum_p (beta c[v_p] + (1 - beta) cA[v_p])
    log Z_A        = L logsumexp(cA) + S K Lh ln 2                  (the base-rate model, beta = 0)

Run r (global index idx[r]) draws v_0 ~ softmax(cA) (kind AIS_V, step word 0) and for t = 0 .. T-1
    logw += log p*_{betas[t+1]}(v_t) - log p*_{betas[t]}(v_t)
    h, h' ~ Bernoulli(sigmoid(betas[t+1] x(v_t)))                    (kind AIS_H, strand 0 / 1, step word t + 1)
    v_{t+1} ~ softmax(betas[t+1] (c + W^T h + rc(W)^T h') + (1 - betas[t+1]) cA)   (kind AIS_V, step word t + 1)
with the sampling rules of the persistent chain (h = [p > u]; first letter whose cumulative probability exceeds u).
Betas are float32 values widened to float64: what the library is handed.
"""
import itertools

import numpy as np

from oracle.crbm_oracle import hidden_uniforms, visible_uniforms, onehot_of

KIND_AIS_H = 6
KIND_AIS_V = 7


def ladder(betas):
    """int T -> linspace(0, 1, T + 1); the float32 values as float64"""
    if isinstance(betas, (int, np.integer)):
        betas = np.linspace(0.0, 1.0, int(betas) + 1)
    return np.asarray(betas, dtype=np.float32).astype(np.float64)


def base_bias(o, cA=None):
    return (o.c if cA is None else np.asarray(cA, dtype=np.float64)).reshape(-1)


def _softplus(x):
    return np.logaddexp(0.0, x)


def activations(o, codes):
    """[x] or [x, x'] of letter codes (n, L), each (n,K,1,Lh), bias included"""
    D = onehot_of(codes, np.float64, o.input_dims)
    acts = [o._bottomUpActivity(D, False)]
    if o.doublestranded:
        acts.append(o._bottomUpActivity(D, True))
    return acts


def log_p_star(o, codes, beta, cA=None, acts=None):
    """log p*_beta of every row of codes, (n,) float64"""
    cA = base_bias(o, cA)
    acts = activations(o, codes) if acts is None else acts
    out = sum(_softplus(beta * x).sum(axis=(1, 2, 3)) for x in acts)
    bias = beta * o.c.reshape(-1) + (1.0 - beta) * cA
    return out + bias[codes].sum(axis=1)


def log_partition_base(o, L, cA=None):
    cA = base_bias(o, cA)
    S = 2 if o.doublestranded else 1
    return L * np.logaddexp.reduce(cA) + S * o.num_motifs * (L - o.motif_length + 1) * np.log(2.0)


def base_draw(o, L, cA, seed, idx):
    """v_0 (n, L) codes, with the probabilities (n,1,A,L) and the uniforms (n,L) that decided them"""
    cA = base_bias(o, cA)
    n = len(idx)
    P = np.broadcast_to((np.exp(cA - cA.max()) / np.exp(cA - cA.max()).sum())[None, None, :, None], (n, 1, len(cA), L)).copy()
    u = visible_uniforms(seed, 0, idx, L, KIND_AIS_V)
    return np.argmax(o._topDownSample(P, u)[:, 0], axis=1), P, u


def ais_step(o, v, t, betas, cA, seed, idx):
    """Step t from letter codes v (n, L).  Returns (dlogw (n,), probabilities, uniforms, h, h', v_next) with
    probabilities = dict(h=, hp=, v=) and uniforms likewise; hp entries are None for single-stranded models.  Also
    returns the scale of the quantities differenced under key 'scale' of the probabilities dict: |log p*_{b1}(v)|."""
    betas = ladder(betas)
    cA = base_bias(o, cA)
    b0, b1 = betas[t], betas[t + 1]
    n, L = v.shape
    K, Lh = o.num_motifs, L - o.motif_length + 1
    acts = activations(o, v)
    hi = log_p_star(o, v, b1, cA, acts)
    # differenced per unit before summing, like the kernel: the sum of two totals would round at the scale of |F|
    dlogw = sum((_softplus(b1 * x) - _softplus(b0 * x)).sum(axis=(1, 2, 3)) for x in acts)
    dlogw = dlogw + (b1 - b0) * (o.c.reshape(-1) - cA)[v].sum(axis=1)
    P, U, H = {"scale": np.abs(hi)}, {}, []
    for strand, x in enumerate(acts):
        p = 1.0 / (1.0 + np.exp(-b1 * x))
        u = hidden_uniforms(seed, t + 1, idx, K, Lh, strand, KIND_AIS_H)
        H.append((p > u).astype(np.float64))
        P["hp" if strand else "h"], U["hp" if strand else "h"] = p, u
    if not o.doublestranded:
        H.append(None)
        P["hp"] = U["hp"] = None
    y = o._topDownActivity(H[0], H[1])                      # c included
    y = b1 * y + (1.0 - b1) * cA.reshape(1, 1, -1, 1)
    pv = o._topDownProbability(y)
    uv = visible_uniforms(seed, t + 1, idx, L, KIND_AIS_V)
    P["v"], U["v"] = pv, uv
    v_next = np.argmax(o._topDownSample(pv, uv)[:, 0], axis=1)
    return dlogw, P, U, H[0], H[1], v_next


def ais(o, L, runs, betas, cA=None, seed=None, run_offset=0, states=False):
    """The whole ladder for `runs` runs.  Returns dict(logw (runs,), v (runs, L) final codes, scale (runs,) =
    max_t |log p*_{betas[t+1]}(v_t)|) and, with states=True, 'trajectory': the codes v_0 .. v_T."""
    betas = ladder(betas)
    seed = o.seed if seed is None else int(seed)
    idx = np.arange(runs) + run_offset
    v, _, _ = base_draw(o, L, cA, seed, idx)
    logw = np.zeros(runs)
    scale = np.zeros(runs)
    traj = [v]
    for t in range(len(betas) - 1):
        d, P, _, _, _, v = ais_step(o, v, t, betas, cA, seed, idx)
        logw += d
        scale = np.maximum(scale, P["scale"])
        if states:
            traj.append(v)
    out = {"logw": logw, "v": v, "scale": scale}
    if states:
        out["trajectory"] = traj
    return out


def estimate(logw, logZ_base):
    """dict(logZ, stderr, ess) from the log weights (float64 reduction; delta-method standard error)"""
    lw = np.asarray(logw, dtype=np.float64)
    w = np.exp(lw - lw.max())
    return {"logZ": logZ_base + lw.max() + np.log(w.mean()),
            "stderr": w.std() / (w.mean() * np.sqrt(len(lw))),
            "ess": w.sum() ** 2 / (w * w).sum()}


def all_sequences(A, L):
    """(A^L, L) uint8 codes of every sequence"""
    return np.array(list(itertools.product(range(A), repeat=L)), dtype=np.uint8)


def exact_log_partition(o, L):
    """log Z = logsumexp over all A^L sequences of log p*_1(v)"""
    return np.logaddexp.reduce(log_p_star(o, all_sequences(o.input_dims, L), 1.0))


# ---- comparing an implementation with the yardstick ---------------------------------------------------------------
TIE = 1e-6          # |p - u| below which float32 and float64 arithmetic may legitimately decide differently


def _visible_gap(P, u):
    """distance of every uniform from the nearest inner threshold of its position's cumulative distribution, (n, L)"""
    cum = np.cumsum(P[:, 0], axis=1)[:, :max(P.shape[2] - 1, 1)]
    return np.min(np.abs(cum - u[:, None, :]), axis=1)


def check_against_yardstick(segment, o, L, runs, betas, cA, seed, rtol, max_tied=None, run_offset=0, label=""):
    """`segment(t0, t1, state, logw) -> (state (runs, L) uint8, logw (runs,) float32)` runs steps [t0, t1) of the
    ladder for runs run_offset .. run_offset + runs - 1 (t0 == 0: state and logw are None, the runs start from the
    base-rate model).  The final letters must EQUAL the yardstick's.  A run that differs is replayed through one-step
    segments from the yardstick's states, and every step whose sample differs must show a tie (a hidden unit or a
    visible threshold with |p - u| < TIE in that run and step); a run that differs without one fails.  Log weights of
    the runs that did not differ: |got - want| <= rtol |want| + rtol max_t |log p*_{betas[t+1]}(v_t)|; the weight
    increment of every replayed step obeys the same bound at that step's scale.  At most `max_tied` runs may be set
    aside.  Returns (number of runs set aside, worst error / bound of the compared log weights)."""
    betas = ladder(betas)
    T = len(betas) - 1
    idx = np.arange(runs) + run_offset
    want = ais(o, L, runs, betas, cA, seed, run_offset=run_offset, states=True)
    state, logw = segment(0, T, None, None)
    assert state.shape == (runs, L) and logw.shape == (runs,) and np.all(np.isfinite(logw))
    differ = (state != want["v"]).any(axis=1)
    if differ.any():
        tied = np.zeros(runs, dtype=bool)
        _, P0, u0 = base_draw(o, L, cA, seed, idx)
        base_tie = (_visible_gap(P0, u0) < TIE).any(axis=1)
        for t in range(T):
            vt = want["trajectory"][t]
            if t == 0:
                s1, lw1 = segment(0, 1, None, None)
            else:
                s1, lw1 = segment(t, t + 1, np.ascontiguousarray(vt, dtype=np.uint8), np.zeros(runs, np.float32))
            d, P, U, _, _, vn = ais_step(o, vt, t, betas, cA, seed, idx)
            tie = (_visible_gap(P["v"], U["v"]) < TIE).any(axis=1)
            for key in ("h", "hp"):
                if P[key] is not None:
                    tie |= (np.abs(P[key] - U[key]) < TIE).any(axis=(1, 2, 3))
            if t == 0:
                tie |= base_tie
            bad = (s1 != vn).any(axis=1)
            assert not np.any(bad & ~tie), "%s step %d: runs %s differ away from a tie" % (label, t, np.nonzero(bad & ~tie)[0])
            tied |= bad
            ok = ~base_tie if t == 0 else np.ones(runs, dtype=bool)
            err, bound = np.abs(lw1 - d), rtol * np.abs(d) + rtol * P["scale"]
            assert np.all(err[ok] <= bound[ok]), "%s step %d: weight increment off by %.3g of its bound" % (label, t, (err / bound)[ok].max())
        assert not np.any(differ & ~tied), "%s: runs %s differ although no sample sits on a tie" % (label, np.nonzero(differ & ~tied)[0])
    clean = ~differ
    err, bound = np.abs(logw - want["logw"]), rtol * np.abs(want["logw"]) + rtol * want["scale"]
    worst = float((err / bound)[clean].max()) if clean.any() else 0.0
    print("%s: %d of %d runs set aside as tied; logw worst error / bound %.3g (max |logw| %.4g, scale %.4g)"
          % (label, int(differ.sum()), runs, worst, np.abs(want["logw"]).max(), want["scale"].max()))
    assert np.all(err[clean] <= bound[clean])
    if max_tied is not None:
        assert differ.sum() <= max_tied, "%d runs set aside as tied, at most %d allowed" % (differ.sum(), max_tied)
    return int(differ.sum()), worst
