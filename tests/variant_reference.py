"""The yardstick of the variant effects (CRBM.variantEffects, crbm_variant_effects_codes): a float64 NumPy reference on
the oracle.  A stream is a 1-D uint8 array of codes, 0..3 = A,C,G,T and 4 = no letter; the free energy of a stream is
    F(stream) = - sum_{valid windows s, strands, motifs k} softplus(x_{k,strand}(s)) - sum_{letters p} c[v_p]
with the activations of the oracle's _bottomUpActivity (the reverse-complemented filter for the second strand of a
double-stranded model, nothing for a single-stranded one).  Per variant (pos, alt): the context
[pos - M + 1, pos + M - 1] with code 4 outside the stream, its M windows, those of them that are valid (all M codes
letters) scored with the context as it is and with alt at its centre, as tests/scan_reference.py scores windows;
    per_motif[i, k] = - sum_{valid windows, strands} softplus(x_alt) - softplus(x_ref)
    dfe[i]          = sum_k per_motif[i, k] - (c[alt] - c[ref])
    windows[i]      = the number of valid windows
and all three 0 where the variant sits on a code 4."""
import numpy as np

from oracle.crbm_oracle import onehot_of, _softplus


def contexts(stream, pos, M):
    """(V, 2M - 1) uint8: codes [pos - M + 1, pos + M - 1] of every variant, 4 outside the stream"""
    stream = np.asarray(stream, np.uint8)
    pos = np.asarray(pos, np.int64)
    idx = pos[:, None] + np.arange(-(M - 1), M)[None, :]
    inside = (idx >= 0) & (idx < stream.size)
    ctx = np.full(idx.shape, 4, np.uint8)
    ctx[inside] = stream[idx[inside]]
    return ctx


def _hidden_terms(o, ctx):
    """(V, K, M) float64: sum over the strands of softplus(x) of the M windows of every context (any letter under a code 4)"""
    D = onehot_of(np.where(ctx > 3, 0, ctx))
    sp = _softplus(o._bottomUpActivity(D))[:, :, 0, :]
    if o.doublestranded:
        sp = sp + _softplus(o._bottomUpActivity(D, True))[:, :, 0, :]
    return sp


def variant_effects(o, stream, pos, alt):
    """dict of dfe (V,), per_motif (V, K) and windows (V,) in float64 / int64, and exact_zero (V,) bool: the variant sits
    on a code 4 or alt == ref, where every output is 0 by definition"""
    M, K = o.motif_length, o.num_motifs
    pos, alt = np.asarray(pos, np.int64), np.asarray(alt, np.int64)
    V = pos.size
    ctx = contexts(stream, pos, M)
    ref = ctx[:, M - 1].astype(np.int64)
    letter = ctx < 4
    bad = np.concatenate([np.zeros((V, 1), np.int64), np.cumsum(~letter, axis=1)], axis=1)
    valid = (bad[:, M:] - bad[:, :M]) == 0                        # (V, M): window m covers context codes [m, m + M)
    mutant = ctx.copy()
    mutant[:, M - 1] = np.where(ref < 4, alt, 4)
    diff = _hidden_terms(o, mutant) - _hidden_terms(o, ctx)       # (V, K, M)
    per_motif = -(diff * valid[:, None, :]).sum(axis=2)
    c = np.asarray(o.c, np.float64).ravel()
    on_letter = ref < 4
    bias = np.where(on_letter, c[alt] - c[np.where(on_letter, ref, 0)], 0.0)
    return {"dfe": per_motif.sum(axis=1) - bias, "per_motif": per_motif, "windows": valid.sum(axis=1).astype(np.int64),
            "exact_zero": ~on_letter | (alt == ref)}


def forced_positions(stream, M):
    """the positions every test adds to its random ones: 0, 1, M-2, M-1, T-M, T-2, T-1, both neighbours of every gap
    edge, and a position inside a gap (those inside [0, T), duplicates removed, ascending)"""
    stream = np.asarray(stream)
    T = stream.size
    want = [0, 1, M - 2, M - 1, T - M, T - 2, T - 1]
    gap = stream > 3
    edges = np.flatnonzero(gap[1:] != gap[:-1])                   # the pair (e, e + 1) straddles an edge
    want += edges.tolist() + (edges + 1).tolist()
    inside = np.flatnonzero(gap)
    if inside.size:
        want.append(int(inside[inside.size // 2]))
    return np.unique([p for p in want if 0 <= p < T]).astype(np.int64)


def variant_list(stream, M, n_random, seed):
    """(pos, alt) of a test: n_random random positions, the forced ones, one duplicate and one alt == ref"""
    stream = np.asarray(stream)
    rng = np.random.default_rng(seed)
    pos = np.concatenate([rng.integers(0, stream.size, size=n_random), forced_positions(stream, M)]).astype(np.int64)
    alt = rng.integers(0, 4, size=pos.size).astype(np.uint8)
    letters = np.flatnonzero(stream[pos] < 4)
    i = int(letters[letters.size // 2])
    pos = np.concatenate([pos, pos[i:i + 1], pos[i:i + 1]])
    alt = np.concatenate([alt, alt[i:i + 1], stream[pos[i]:pos[i] + 1].astype(np.uint8)])    # the duplicate, then alt == ref
    return pos, alt


def check(got, want, rtol, label=""):
    """the project's mutagenesis criterion, |got - want| <= rtol |want| + rtol max|want| with the maximum over the
    compared array, on dfe and per_motif separately; windows exactly; exact zeros where the definition has them: all
    of a variant on a code 4 or with alt == ref, the hidden part of one without a valid window"""
    assert np.array_equal(got["windows"], want["windows"]), label
    for key in ("dfe", "per_motif"):
        g, w = np.asarray(got[key], np.float64), want[key]
        assert g.shape == w.shape, (label, key, g.shape, w.shape)
        assert np.all(np.isfinite(g)), (label, key)
        scale = np.abs(w).max() if w.size else 0.0
        err = np.abs(g - w)
        bound = rtol * np.abs(w) + rtol * scale
        print("%s %s: max err %.3g, bound at the largest %.3g" % (label, key, err.max() if err.size else 0.0, 2 * rtol * scale))
        assert np.all(err <= bound), (label, key, float((err - bound).max()), np.argwhere(err > bound)[:5].tolist())
    z = want["exact_zero"]
    assert np.all(np.asarray(got["dfe"])[z] == 0.0) and np.all(np.asarray(got["per_motif"])[z | (want["windows"] == 0)] == 0.0), label
