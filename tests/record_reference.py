"""The yardstick of the record summaries (CRBM.recordSummary, crbm_scan_records_codes): a float64 NumPy reference on
the oracle.  A stream is a 1-D uint8 array of codes, 0..3 = A,C,G,T and 4 = no letter; `offsets` are those of
sequences.seqsToStream: record r is stream[offsets[r]:offsets[r + 1] - 1], one code 4 between two records.  A window
belongs to the record its start lies in; the separator keeps every valid window inside one record.  Per record:
    windows            its valid windows (tests/scan_reference.window_valid)
    letters[a]         its letters A, C, G, T
    per_motif[k]       - sum_{valid windows, strands} softplus(x_k): the hidden terms of tests/variant_reference.py (the
                       reverse-complemented filter for the second strand of a double-stranded model, nothing for a
                       single-stranded one), WITHOUT the visible bias the oracle's _freeEnergyPerMotif adds to every column
    fe                 sum_k per_motif[k] - sum_a letters[a] c[a]: variant_reference's F restricted to the record
    best site          the argmax of tests/scan_reference.stream_scores over the record's valid windows and the strands
and the two rules the emulation and the GPU are held to: check_best and check_fe."""
import numpy as np

from oracle.crbm_oracle import onehot_of, _softplus
from tests.scan_reference import stream_scores, window_valid


def make_stream(records):
    """(stream, offsets) of a list of uint8 code arrays, in seqsToStream's convention"""
    lengths = np.array([len(r) for r in records], np.int64)
    offsets = np.zeros(len(records) + 1, np.int64)
    np.cumsum(lengths + 1, out=offsets[1:])
    stream = np.full(max(int(offsets[-1]) - 1, 0), 4, np.uint8)
    for r, a in zip(records, offsets[:-1]):
        stream[a:a + len(r)] = r
    return stream, offsets


def split_records(stream, offsets):
    return [np.asarray(stream[offsets[r]:offsets[r + 1] - 1], np.uint8) for r in range(len(offsets) - 1)]


def record_stream(seed, M):
    """(stream, offsets): records of length 0, 0, 1, M - 1, M, M + 1, 63, 64, 65, then 40 of random length 1..399, then
    one of 1500; about half of the records above 60 letters carry a gap run of 1..4 codes.  About 10 800 letters."""
    rng = np.random.default_rng(seed)
    lengths = [0, 0, 1, M - 1, M, M + 1, 63, 64, 65] + rng.integers(1, 400, size=40).tolist() + [1500]
    records = []
    for L in lengths:
        r = rng.integers(0, 4, size=L, dtype=np.uint8)
        if L > 60 and rng.random() < 0.5:
            n = int(rng.integers(1, 5))
            at = int(rng.integers(0, L - n + 1))
            r[at:at + n] = 4
        records.append(r)
    return make_stream(records)


def softplus_terms(o, stream):
    """(K, T - M + 1) float64: softplus(x_k) of every window summed over the strands (any letter under a code 4)"""
    stream = np.asarray(stream, np.uint8)
    D = onehot_of(np.where(stream > 3, 0, stream)[None, :])
    sp = _softplus(o._bottomUpActivity(D))[0, :, 0, :]
    if o.doublestranded:
        sp = sp + _softplus(o._bottomUpActivity(D, True))[0, :, 0, :]
    return sp


def record_summary(o, stream, offsets):
    """dict of windows (R,), letters (R, 4) int64; per_motif (R, K), fe (R,) float64; start, strand (R, K) int64 and
    prob (R, K) float64 of the reference's own best site (ties to the smaller start, then to +; -1, 0, 0 without a valid
    window); P (S, K, T - M + 1) and valid of stream_scores for check_best"""
    stream = np.asarray(stream, np.uint8)
    offsets = np.asarray(offsets, np.int64)
    M, K, R = o.motif_length, o.num_motifs, offsets.size - 1
    c = np.asarray(o.c, np.float64).ravel()
    valid = window_valid(stream, M)
    letters = np.zeros((R, 4), np.int64)
    windows = np.zeros(R, np.int64)
    per_motif = np.zeros((R, K))
    start = np.full((R, K), -1, np.int64)
    strand = np.zeros((R, K), np.int64)
    prob = np.zeros((R, K))
    if valid.size:
        P, _ = stream_scores(o, stream)
        sp = softplus_terms(o, stream)
    else:
        P = np.zeros((2 if o.doublestranded else 1, K, 0))
    for r in range(R):
        a, b = int(offsets[r]), int(offsets[r + 1]) - 1
        letters[r] = np.bincount(stream[a:b][stream[a:b] < 4], minlength=4)
        hi = min(b - M + 1, valid.size)                       # window starts [a, hi) lie in the record
        if hi <= a:
            continue
        v = valid[a:hi]
        windows[r] = v.sum()
        if not v.any():
            continue
        per_motif[r] = -(sp[:, a:hi] * v[None, :]).sum(axis=1)
        Pr = P[:, :, a:hi]                                    # invalid windows hold -1
        for k in range(K):
            best = Pr[:, k, :].max()
            st, s = np.nonzero(Pr[:, k, :] == best)
            i = np.lexsort((st, s))[0]
            start[r, k], prob[r, k] = s[i], best
            strand[r, k] = (-1 if st[i] else 1) if o.doublestranded else 0
    fe = per_motif.sum(axis=1) - letters @ c
    return {"windows": windows, "letters": letters, "per_motif": per_motif, "fe": fe, "start": start, "strand": strand,
            "prob": prob, "P": P, "valid": valid, "offsets": offsets, "ds": bool(o.doublestranded), "c": c, "M": M, "stream": stream}


def _gather_input(stream, M, ds, st, pos):
    """what the score of window `pos` on strand index `st` is a function of, as the kernels evaluate it: the M letters,
    reverse-complemented for the - strand of a double-stranded model (the forward gather of the reverse-complemented
    window).  Two windows with the same input get the same bits; a single-stranded window and its reverse complement
    get x + x' and x' + x, the same sum added in another order, which float32 need not round alike."""
    w = stream[pos:pos + M]
    return (3 - w[::-1] if ds and st else w).tobytes()


def check_best(got, ref, rtol, label=""):
    """THE BEST-SITE RULE.  p* is the reference maximum of a (record, motif) cell, its near-max set the windows with
    P >= p* (1 - 2 rtol).  got's (start, strand) must lie in that set, its prob within rtol of the reference there.
    Where every member of the set has the same reference value and the same letters in front of the gather
    (_gather_input) -- an exact tie: identical letters give identical bits -- got must name the smallest start, then +.
    Cells whose set holds two different values are ambiguous: membership alone; at most 1 % of the cells may be.
    Cells whose set holds one value under different letters (a single-stranded window and its reverse complement
    elsewhere in the record: sigma(x + x') and sigma(x' + x)) are mirror ties: the reference cannot say which of them
    float32 ranks first, so membership alone is demanded there as well; they are counted apart and do not enter the cap.
    Cells without a valid window: start -1, strand 0, prob exactly 0.
    Returns (ambiguous cells, cells with a valid window, exact ties of more than one window, mirror ties)."""
    P, offsets, ds, M, stream = ref["P"], ref["offsets"], ref["ds"], ref["M"], ref["stream"]
    R, K = ref["start"].shape
    g_start, g_strand, g_prob = (np.asarray(got[f]) for f in ("start", "strand", "prob"))
    assert g_start.shape == (R, K) and g_strand.shape == (R, K) and g_prob.shape == (R, K), label
    ambiguous = cells = ties = mirror = 0
    for r in range(R):
        if ref["windows"][r] == 0:
            assert np.all(g_start[r] == -1) and np.all(g_strand[r] == 0) and np.all(g_prob[r] == 0.0), (label, r)
            continue
        a = int(offsets[r])
        hi = min(int(offsets[r + 1]) - 1 - M + 1, P.shape[2])
        Pr = P[:, :, a:hi]
        for k in range(K):
            cells += 1
            best = Pr[:, k, :].max()
            near = Pr[:, k, :] >= best * (1 - 2 * rtol)
            near &= Pr[:, k, :] >= 0
            s = int(g_start[r, k])
            assert np.isin(g_strand[r, k], (1, -1) if ds else (0,)), (label, r, k)
            st = 1 if g_strand[r, k] == -1 else 0
            assert 0 <= s < Pr.shape[2] and near[st, s], (label, r, k, s, st, "not a near-maximal window")
            want = Pr[st, k, s]
            assert abs(float(g_prob[r, k]) - want) <= rtol * want, (label, r, k, float(g_prob[r, k]), want)
            values = np.unique(Pr[:, k, :][near])
            sts, ss = np.nonzero(near)
            if values.size > 1:
                ambiguous += 1
            elif len({_gather_input(stream, M, ds, int(t), a + int(p)) for t, p in zip(sts, ss)}) > 1:
                mirror += 1
            else:
                i = np.lexsort((sts, ss))[0]
                assert (s, st) == (int(ss[i]), int(sts[i])), (label, r, k, "exact tie: the smallest start, then +", s, st)
                ties += int(near.sum() > 1)
    assert ambiguous <= 0.01 * max(cells, 1), (label, ambiguous, cells)
    return ambiguous, cells, ties, mirror


def check_fe(got, ref, rtol, unit, label=""):
    """THE FREE-ENERGY TOLERANCE, derived: a window's term is rounded once to `unit` (half a unit each) on top of the
    float32 evaluation: |got - ref| <= rtol |ref| + windows unit / 2 per cell of per_motif; for fe the sum of the row's
    bounds plus rtol sum_a letters |c_a|.  windows and letters exactly; a record without a valid window has a
    per_motif row of exact zeros."""
    assert np.array_equal(np.asarray(got["windows"]), ref["windows"]), label
    assert np.array_equal(np.asarray(got["letters"]), ref["letters"]), label
    pm, fe = np.asarray(got["per_motif"], np.float64), np.asarray(got["fe"], np.float64)
    assert pm.shape == ref["per_motif"].shape and fe.shape == ref["fe"].shape, label
    bound = rtol * np.abs(ref["per_motif"]) + ref["windows"][:, None] * unit / 2
    err = np.abs(pm - ref["per_motif"])
    print("%s per_motif: max err %.3g, its bound %.3g" % (label, err.max() if err.size else 0.0,
                                                          bound.ravel()[err.argmax()] if err.size else 0.0))
    assert np.all(err <= bound), (label, "per_motif", np.argwhere(err > bound)[:5].tolist(), float((err - bound).max()))
    assert np.all(pm[ref["windows"] == 0] == 0.0), label
    fbound = bound.sum(axis=1) + rtol * (ref["letters"] * np.abs(ref["c"])[None, :]).sum(axis=1)
    ferr = np.abs(fe - ref["fe"])
    print("%s fe: max err %.3g, its bound %.3g" % (label, ferr.max() if ferr.size else 0.0,
                                                   fbound[ferr.argmax()] if ferr.size else 0.0))
    assert np.all(ferr <= fbound), (label, "fe", np.argwhere(ferr > fbound)[:5].tolist())
