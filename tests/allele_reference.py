"""The yardstick of the allele effects (CRBM.alleleEffects, crbm_allele_effects_codes): a float64 NumPy reference on the
oracle, in the terms of tests/variant_reference.py.  Variant i = (pos, R, alt) replaces the R codes stream[pos:pos+R]
by the letters of alt.  With left = codes [pos - M + 1, pos) and right = codes [pos + R, pos + R + M - 1), code 4
outside the stream, refhap = left . ref . right has R + M - 1 windows and althap = left . alt . right has A + M - 1; a
window is valid when all its M codes are letters;
    S_hap[k]        = sum over the valid windows of hap and the strands of softplus(x_k)
    per_motif[i, k] = -(S_alt[k] - S_ref[k])
    dfe[i]          = sum_k per_motif[i, k] - (sum_j c[alt_j] - sum_j c[ref_j])
    windows[i]      = (valid windows of refhap, valid windows of althap)
    mass            = S_alt + S_ref, per motif (V, K) and in total (V,): what the two sums that are actually computed hold
and everything 0 where R = A = 0 or the replaced span holds a code 4 (exact_zero)."""
import numpy as np

from tests.variant_reference import _hidden_terms

LETTERS = np.frombuffer(b"ACGTN", np.uint8)


def haplotypes(stream, pos, R, alt, M):
    """(refhap, althap) of one variant, uint8 codes"""
    stream = np.asarray(stream, np.uint8)
    T = stream.size
    idx = np.arange(pos - (M - 1), pos + R + (M - 1))
    inside = (idx >= 0) & (idx < T)
    ref = np.full(idx.size, 4, np.uint8)
    ref[inside] = stream[idx[inside]]
    return ref, np.concatenate([ref[:M - 1], np.asarray(alt, np.uint8), ref[M - 1 + R:]])


def _sums(o, haps):
    """per haplotype: (S (K,), valid windows); haplotypes of one length go through the oracle together"""
    M, K = o.motif_length, o.num_motifs
    S, nwin = np.zeros((len(haps), K)), np.zeros(len(haps), np.int64)
    by_len = {}
    for i, h in enumerate(haps):
        by_len.setdefault(h.size, []).append(i)
    for n, members in by_len.items():
        if n < M:
            continue
        ctx = np.stack([haps[i] for i in members])
        bad = np.concatenate([np.zeros((len(members), 1), np.int64), np.cumsum(ctx > 3, axis=1)], axis=1)
        valid = (bad[:, M:] - bad[:, :n - M + 1]) == 0                  # (members, n - M + 1)
        S[members] = (_hidden_terms(o, ctx) * valid[:, None, :]).sum(axis=2)
        nwin[members] = valid.sum(axis=1)
    return S, nwin


def allele_effects(o, stream, pos, R, alts):
    """dict of dfe (V,), per_motif (V, K), windows (V, 2), exact_zero (V,), mass {'dfe': (V,), 'per_motif': (V, K)}"""
    M, K = o.motif_length, o.num_motifs
    V = len(pos)
    c = np.asarray(o.c, np.float64).ravel()
    refs, alth = [], []
    zero = np.zeros(V, bool)
    bias = np.zeros(V)
    for i in range(V):
        r, a = haplotypes(stream, int(pos[i]), int(R[i]), alts[i], M)
        span = r[M - 1:M - 1 + int(R[i])]
        zero[i] = (R[i] == 0 and len(alts[i]) == 0) or bool((span > 3).any())
        if not zero[i]:
            bias[i] = c[np.asarray(alts[i], np.int64)].sum() - c[span.astype(np.int64)].sum()
        refs.append(r)
        alth.append(a)
    S_ref, n_ref = _sums(o, refs)
    S_alt, n_alt = _sums(o, alth)
    keep = ~zero
    per_motif = -(S_alt - S_ref) * keep[:, None]
    mass = (S_alt + S_ref) * keep[:, None]
    return {"dfe": per_motif.sum(axis=1) - bias, "per_motif": per_motif,
            "windows": (np.stack([n_ref, n_alt], axis=1) * keep[:, None]).astype(np.int64), "exact_zero": zero,
            "mass": {"dfe": mass.sum(axis=1), "per_motif": mass}}


def forced_ra(M):
    return [(1, 1), (2, 2), (3, 3), (0, 1), (0, M), (0, 70), (1, 0), (M, 0), (70, 0), (2, 5), (130, 1), (1, 130)]


def allele_list(stream, M, n_random, seed):
    """(pos int64 (V,), R int32 (V,), alts: list of V uint8 arrays) of a test: n_random random positions with R and A
    drawn from 0..3; the forced (R, A) of forced_ra at random positions; positions 0 and T - R and pos = T with R = 0;
    both neighbours of every gap edge; a short insertion between two neighbouring codes 4 (no valid window on either
    haplotype); a span that covers a code 4; an R = A = 0 variant; a duplicate (the last entry, of the (2, 5) allele)"""
    stream = np.asarray(stream)
    T = stream.size
    rng = np.random.default_rng(seed)
    pos, R, alts = [], [], []

    def add(p, r, a):
        r = int(min(r, T))
        p = int(min(max(p, 0), T - r))
        pos.append(p); R.append(r); alts.append(rng.integers(0, 4, size=int(a)).astype(np.uint8))
        return len(pos) - 1
    for _ in range(n_random):
        r = int(rng.integers(0, 4))
        add(rng.integers(0, T - r + 1), r, rng.integers(0, 4))
    dup = None
    for r, a in forced_ra(M):
        i = add(rng.integers(0, max(T - r, 0) + 1), r, a)
        if (r, a) == (2, 5):
            dup = i
    for r, a in ((1, 1), (2, 1), (0, 2), (3, 0)):
        add(0, r, a)
        add(T - r, r, a)
    add(T, 0, 2)
    gap = stream > 3
    edges = np.flatnonzero(gap[1:] != gap[:-1])
    combos = [(1, 1), (0, 2), (2, 0), (1, 3), (0, 1), (1, 0)]
    for n, e in enumerate(edges.tolist()):
        for d in (0, 1):
            r, a = combos[(2 * n + d) % len(combos)]
            add(e + d, r, a)
    pairs = np.flatnonzero(gap[1:] & gap[:-1])
    if pairs.size:
        add(int(pairs[0]) + 1, 0, 2)
    inside = np.flatnonzero(gap)
    if inside.size:
        add(int(inside[inside.size // 2]) - 1, 3, 2)                   # a span that covers a code 4
    add(T // 2, 0, 0)
    pos.append(pos[dup]); R.append(R[dup]); alts.append(alts[dup].copy())
    return np.array(pos, np.int64), np.array(R, np.int32), alts


def pack(alts):
    """(alt_off int64 (V + 1,), alt_codes uint8) of crbm_allele_effects_codes"""
    off = np.zeros(len(alts) + 1, np.int64)
    np.cumsum([len(a) for a in alts], out=off[1:])
    codes = np.concatenate([np.asarray(a, np.uint8) for a in alts]) if len(alts) else np.zeros(0, np.uint8)
    return off, np.ascontiguousarray(codes, np.uint8)


def strings(stream, pos, R, alts):
    """(ref, alt) as the lists of strings CRBM.alleleEffects takes"""
    stream = np.asarray(stream)
    ref = [LETTERS[stream[p:p + r]].tobytes().decode() for p, r in zip(pos.tolist(), R.tolist())]
    return ref, [LETTERS[np.asarray(a, np.int64)].tobytes().decode() for a in alts]


def covers_every_count(want, R, alts, M):
    """full, partial and zero window counts on both haplotypes (M = 1 has no partial count: a window is one code, and a
    code 4 in the replaced span makes the variant an exact zero)"""
    w = want["windows"]
    full = np.stack([np.asarray(R) + M - 1, np.array([len(a) for a in alts]) + M - 1], axis=1)
    live = ~want["exact_zero"]
    for h in (0, 1):
        assert (live & (w[:, h] == full[:, h]) & (full[:, h] > 0)).any(), h
        assert (live & (w[:, h] == 0)).any(), h
        assert M == 1 or (live & (0 < w[:, h]) & (w[:, h] < full[:, h])).any(), h


def check(got, want, rtol, label=""):
    """|got - want| <= rtol |want| + rtol max|want| + rtol mass, on dfe and on per_motif separately -- the project's fp32
    parity standard (1e-4 relative) applied to the two sums S_alt and S_ref that are actually computed, on top of the
    mutagenesis criterion; windows and the exact zeros exactly"""
    assert np.array_equal(np.asarray(got["windows"], np.int64), want["windows"]), label
    for key in ("dfe", "per_motif"):
        g, w = np.asarray(got[key], np.float64), want[key]
        assert g.shape == w.shape, (label, key, g.shape, w.shape)
        assert np.all(np.isfinite(g)), (label, key)
        scale = np.abs(w).max() if w.size else 0.0
        err = np.abs(g - w)
        bound = rtol * np.abs(w) + rtol * scale + rtol * want["mass"][key]
        print("%s %s: max err %.3g, max|want| %.3g, max mass %.3g" % (label, key, err.max() if err.size else 0.0, scale,
                                                                        want["mass"][key].max() if w.size else 0.0))
        assert np.all(err <= bound), (label, key, float((err - bound).max()), np.argwhere(err > bound)[:5].tolist())
    z = want["exact_zero"]
    assert np.all(np.asarray(got["dfe"])[z] == 0.0) and np.all(np.asarray(got["per_motif"])[z] == 0.0), label
    assert np.all(np.asarray(got["windows"])[z] == 0), label
    none = want["windows"].sum(axis=1) == 0
    assert np.all(np.asarray(got["per_motif"])[none] == 0.0), label
