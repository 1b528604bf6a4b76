"""In-silico mutagenesis and the pseudo-log-likelihood (CRBM.mutagenesis / pseudoLogLikelihood, crbm_mutagenesis*) on
every model class of test_gpu_sweeps against the float64 oracle, want[n,p,a] = L (o.freeEnergy(v with p -> a) -
o.freeEnergy(v)) and pll from want; bit for bit across input forms, slab sizes and runs; the fused kernel against the
general path; against the shipped freeEnergy of mutants; and config #2's double-stranded model over 65 536 resident
sequences.

Tolerance: |got - want| <= RTOL |want| + RTOL max|want| (the project's fp32 parity criterion at the scale of the
output, the maximum over the compared call); dF of the sequence's own letter is exactly 0.  pll: rtol = RTOL and
atol = 2 RTOL L max|want| (each of the L position terms moves by at most the largest error of its dF entries)."""
import ctypes

import numpy as np
import pytest

from tests.test_gpu_parity import make_pair, RTOL
from tests.test_gpu_sweeps import CLASSES, ids, _model, _codes, _onehot, _budget, _in_bytes

pytestmark = pytest.mark.gpu

FUSED, GENERAL = 1, 2          # crbm_launch_info.mutagenesis_route


def oracle_mutagenesis(o, codes, A):
    """want (n,L,A) float64 and pll (n) from it: the brute force over the (A-1) L mutants of every row"""
    n, L = codes.shape
    base = o.freeEnergy(_onehot(codes, A))
    want = np.zeros((n, L, A))
    for p in range(L):
        for a in range(A):
            mut = codes.copy()
            mut[:, p] = a
            want[:, p, a] = L * (o.freeEnergy(_onehot(mut, A)) - base)
    want[np.arange(n)[:, None], np.arange(L)[None, :], codes] = 0.0
    return want, pll_of(want)


def pll_of(d):
    d = np.asarray(d, dtype=np.float64)
    mn = d.min(axis=2, keepdims=True)
    return -(np.log(np.exp(-(d - mn)).sum(axis=2)) - mn[..., 0]).sum(axis=1)


def check_df(got, want, codes, label=""):
    n, L, A = want.shape
    scale = np.abs(want).max()
    err = np.abs(got - want)
    bound = RTOL * np.abs(want) + RTOL * scale
    print("%s dF: max|want| %.4g, median|want| %.3g, max err %.3g, worst err/bound %.3g"
          % (label, scale, np.median(np.abs(want[want != 0])), err.max(), (err / bound).max()))
    assert np.all(err <= bound)
    own = got[np.arange(n)[:, None], np.arange(L)[None, :], codes]
    assert np.all(own == 0.0)
    return scale


def check_pll(got, want, L, scale, label=""):
    print("%s pll: max err %.3g, atol %.3g, mean pll/L %.4g" % (label, np.abs(got - want).max(), 2 * RTOL * L * scale,
                                                               want.mean() / L))
    np.testing.assert_allclose(got, want, rtol=RTOL, atol=2 * RTOL * L * scale)
    assert np.all(got <= 0)


def _route(m):
    from crbm_amd import _lib
    info = _lib.CrbmLaunchInfo()
    m._check(m._lib.crbm_get_launch_info(m._h(), ctypes.byref(info)))
    return info.mutagenesis_route


def _resident(m, lo, hi, L, A, dfe=True, pll=True):
    from crbm_amd._lib import fptr
    d = np.full((hi - lo, L, A), np.nan, np.float32)
    p = np.full((hi - lo,), np.nan, np.float32)
    m._call("crbm_mutagenesis_resident", lo, hi, fptr(d) if dfe else None, fptr(p) if pll else None)
    return (d if dfe else None), (p if pll else None)


def _bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _row_bytes(src, K, L, A, fused, dfe):
    """a LOWER bound of the bytes per row that crbm_mutagenesis* counts (crbm_api.hip, mutagenesis_any): input, outputs
    and -- on the general path -- the row's 1 + (A-1) L expanded rows with their free energies (the scratch of slabbed
    free energies comes on top): a budget of r times this gives slabs of at most r rows"""
    LW = (L + 15) // 16 + 2 if A == 4 else (L + 3) // 4 + 2
    work = 0 if fused else (1 + (A - 1) * L) * (LW * 4 + (K + 1) * 4)
    return _in_bytes(src, A, L) + (L * A * 4 if dfe else 0) + 4 + work


@pytest.mark.parametrize("cls", CLASSES, ids=ids(CLASSES))
def test_mutagenesis_against_oracle_sources_slabs_runs(cls, monkeypatch):
    """Every class against the oracle with its route asserted (specialised classes without pooling: the fused kernel;
    everything else: the general path); one-hot, codes and resident input, in one slab and in seven: dF and pll the
    same bits in all six and in a repeated call; pseudoLogLikelihood (no dense array) equals the value reduced from
    mutagenesis in float64 and is <= 0."""
    name, K, M, ds, A, pool, Lf, L, env, spec = cls
    n, lo = 27, 5
    fused = spec and pool == 1
    m, o = _model(cls, monkeypatch)
    allc = _codes(n + 11, L, A, seed=K + M + 2)
    m._upload(allc, 0)
    codes = allc[lo:lo + n]
    data = _onehot(codes, A)
    no = n if L <= 200 else 3          # rows against the oracle: its brute force takes 8 s per row at 1200 bp
    want, wpll = oracle_mutagenesis(o, codes[:no], A)
    _budget(monkeypatch, 0, None)
    dfe = m.mutagenesis(codes)
    assert _route(m) == (FUSED if fused else GENERAL)
    assert dfe.shape == (n, L, A) and dfe.dtype == np.float32
    scale = check_df(dfe[:no], want, codes[:no], name)
    pll = m.pseudoLogLikelihood(codes)
    assert pll.shape == (n,) and pll.dtype == np.float32
    check_pll(pll[:no], wpll, L, scale, name)
    check_pll(pll, pll_of(dfe), L, scale, name + " (from its own dF)")
    # the same bits from one-hot input, the resident rows, a second run, and seven slabs on both streams
    assert _bits(dfe, m.mutagenesis(data)) and _bits(pll, m.pseudoLogLikelihood(data))
    rd, rp = _resident(m, lo, lo + n, L, A)
    assert _bits(dfe, rd) and _bits(pll, rp)
    assert _bits(dfe, m.mutagenesis(codes)) and _bits(pll, m.pseudoLogLikelihood(codes))
    for src, x in (("codes", codes), ("onehot", data)):
        _budget(monkeypatch, _row_bytes(src, K, L, A, fused, True), 4)      # slabs of at most 4 rows: 7 or more
        assert _bits(dfe, m.mutagenesis(x))
        _budget(monkeypatch, _row_bytes(src, K, L, A, fused, False), 4)
        assert _bits(pll, m.pseudoLogLikelihood(x))
    _budget(monkeypatch, _row_bytes("resident", K, L, A, fused, True), 4)
    rd, rp = _resident(m, lo, lo + n, L, A)
    assert _bits(dfe, rd) and _bits(pll, rp)
    _budget(monkeypatch, _row_bytes("resident", K, L, A, fused, False), 4)
    _, rp = _resident(m, lo, lo + n, L, A, dfe=False)
    assert _bits(pll, rp)
    d_only, _ = _resident(m, lo, lo + n, L, A, pll=False)
    assert _bits(dfe, d_only)
    # a budget below any row: one row per slab whatever the library counts per row -- 27 slabs alternating between the
    # two streams for certain
    monkeypatch.setenv("CRBM_SLAB_BYTES", "1")
    assert _bits(dfe, m.mutagenesis(codes)) and _bits(pll, m.pseudoLogLikelihood(data))
    rd, rp = _resident(m, lo, lo + n, L, A)
    assert _bits(dfe, rd) and _bits(pll, rp)


# The general path's rounding is that of the per-motif free energies it differences: each carries about half an ulp of
# v_k = sum over positions and strands of softplus, so K motifs contribute up to K ulp(v_k).  For that to stay inside
# RTOL max|dF| whatever the data, the class compared here is a short-sequence one: 10 x 5 double-stranded at 64 bp has
# v_k ~ 2 * 60 * 3 < 512 (ulp 3e-5, K ulp = 3e-4) against RTOL max|dF| of a few 1e-4; at config #2's 200 bp v_k passes
# 1024 and K ulp(v_k) = 1.2e-3 exceeds the bound although the typical error does not ("Mutagenesis").
SPEC_SHORT = ("spec_10x5_ds_L64", 10, 5, True, 4, 1, 200, 64, {}, True)


def test_fused_kernel_against_general_path(monkeypatch):
    """one specialised class on both routes: CRBM_MUT_FUSED=0 forces expand + free energy + combine; both against the
    oracle and against each other within the tolerance"""
    name, K, M, ds, A, pool, Lf, L, env, spec = SPEC_SHORT
    n = 24
    m, o = _model(SPEC_SHORT, monkeypatch)
    codes = _codes(n, L, A, seed=19)
    want, wpll = oracle_mutagenesis(o, codes, A)
    fd, fp_ = m.mutagenesis(codes), m.pseudoLogLikelihood(codes)
    assert _route(m) == FUSED
    monkeypatch.setenv("CRBM_MUT_FUSED", "0")
    gd, gp = m.mutagenesis(codes), m.pseudoLogLikelihood(codes)
    assert _route(m) == GENERAL
    scale = check_df(fd, want, codes, "fused")
    check_df(gd, want, codes, "general")
    check_pll(fp_, wpll, L, scale, "fused")
    check_pll(gp, wpll, L, scale, "general")
    err = np.abs(fd.astype(np.float64) - gd)
    print("fused vs general: max diff %.3g, bound %.3g" % (err.max(), RTOL * scale))
    assert np.all(err <= RTOL * np.abs(gd) + RTOL * scale)
    # the forced general path in seven slabs: the same bits
    _budget(monkeypatch, _row_bytes("codes", K, L, A, False, True), 4)
    assert _bits(gd, m.mutagenesis(codes))
    monkeypatch.delenv("CRBM_MUT_FUSED")
    assert _bits(fd, m.mutagenesis(codes)) and _route(m) == FUSED


# a specialised POOLED class at (nearly) config #2's length: the general route through launch_free_energy's specialised
# pooled kernel (free_energy_body, POOL > 1); 198 bp because the hidden length must be a multiple of the pooling
SPEC_POOLED = ("spec_10x15_ss_pool4_L198", 10, 15, False, 4, 4, 48, 198, {}, True)


def test_specialised_pooled_class_against_oracle(monkeypatch):
    name, K, M, ds, A, pool, Lf, L, env, spec = SPEC_POOLED
    n = 12
    m, o = _model(SPEC_POOLED, monkeypatch)
    codes = _codes(n, L, A, seed=23)
    want, wpll = oracle_mutagenesis(o, codes, A)
    dfe, pll = m.mutagenesis(codes), m.pseudoLogLikelihood(codes)
    assert _route(m) == GENERAL
    scale = check_df(dfe, want, codes, name)
    check_pll(pll, wpll, L, scale, name)
    _budget(monkeypatch, _row_bytes("codes", K, L, A, False, True), 4)
    assert _bits(dfe, m.mutagenesis(codes))


SHIPPED = [CLASSES[0], CLASSES[2], CLASSES[4]]


@pytest.mark.parametrize("cls", SHIPPED, ids=ids(SHIPPED))
def test_mutagenesis_agrees_with_shipped_free_energy(cls, monkeypatch):
    """for a handful of (n, p, a): dF against the GPU's own freeEnergy of mutant and base, within the tolerance of the
    module docstring.  The reference is formed from freeEnergy(permotif=True), fem_k = -v_k - cs, differenced per motif
    and then summed, sum_k ((fem'_k - fem_k) + dc) - dc with dc = c[a] - c[v_p]: L (freeEnergy(mutant) -
    freeEnergy(base)) itself, a difference of two fp32 totals, would carry the rounding of F (2 ulp(F), above the
    tolerance for these classes) -- it is printed beside it."""
    name, K, M, ds, A, pool, Lf, L, env, spec = cls
    n = 6
    m, o = _model(cls, monkeypatch)
    codes = _codes(n, L, A, seed=31)
    dfe = m.mutagenesis(codes)
    rng = np.random.default_rng(5)
    picks = [(int(rng.integers(n)), int(p), int(rng.integers(A))) for p in (0, 1, M - 1, L // 2, L - M, L - 1)]
    muts = np.stack([codes[i] for i, p, a in picks])
    for j, (i, p, a) in enumerate(picks):
        muts[j, p] = a
    fem0 = m.freeEnergy(codes, True).astype(np.float64)
    fem1 = m.freeEnergy(muts, True).astype(np.float64)
    tot0, tot1 = m.freeEnergy(codes).astype(np.float64), m.freeEnergy(muts).astype(np.float64)
    c = m.c.get_value().astype(np.float64).ravel()
    scale = np.abs(dfe).max()
    for j, (i, p, a) in enumerate(picks):
        dc = c[a] - c[codes[i, p]]
        ref = float(np.sum((fem1[j] - fem0[i]) + dc) - dc)
        bound = RTOL * abs(ref) + RTOL * scale
        print(name, (i, p, a), "dF %.6g, per-motif reference %.6g (err/bound %.3g), L (fe' - fe) %.6g"
              % (dfe[i, p, a], ref, abs(dfe[i, p, a] - ref) / bound, L * (tot1[j] - tot0[i])))
        assert abs(dfe[i, p, a] - ref) <= bound


def test_null_outputs_and_short_sequences_are_argument_errors():
    """dfe == pll == NULL and L < motif_length are CRBM_ERR_INVALID from the library itself (the Python methods never
    pass either); the handle stays usable"""
    from crbm_amd import _lib
    m, o = make_pair(4, 5, ds=True)
    h = m._h()
    codes = _codes(3, 20, 4, seed=1)
    m._upload(codes, 0)
    u8 = ctypes.POINTER(ctypes.c_uint8)
    out = np.zeros((3, 20, 4), np.float32)
    assert m._lib.crbm_mutagenesis_resident(h, 0, 1, None, None) == _lib.ERR_INVALID
    assert m._lib.crbm_mutagenesis_codes(h, codes.ctypes.data_as(u8), 3, 20, None, None) == _lib.ERR_INVALID
    assert m._lib.crbm_mutagenesis(h, _lib.fptr(_onehot(codes, 4)), 3, 20, None, None) == _lib.ERR_INVALID
    short = np.zeros((2, 4), np.uint8)
    assert m._lib.crbm_mutagenesis_codes(h, short.ctypes.data_as(u8), 2, 4, _lib.fptr(out), None) == _lib.ERR_INVALID
    assert m.mutagenesis(codes).shape == (3, 20, 4)


def test_mutagenesis_scale_cfg2_resident_and_parameter_change():
    """config #2's model (10 x 15, double-stranded) over 65 536 x 200 bp resident: pll only (nothing of size n L A
    exists), then dF and pll of the first and last 64 rows against the oracle; a parameter change between two calls is
    seen by the second"""
    K, M, n, L = 10, 15, 65536, 200
    m, o = make_pair(K, M, ds=True, Lf=186, bshift=3.0, wscale=0.7)
    codes = _codes(n, L, 4, seed=78)
    m._upload(codes, 0)
    _, pll = _resident(m, 0, n, L, 4, dfe=False)
    assert _route(m) == FUSED
    assert np.all(np.isfinite(pll)) and np.all(pll <= 0)
    print("cfg2: mean pll/L %.4f" % (pll.mean() / L))
    for a, b in ((0, 64), (n - 64, n)):
        want, wpll = oracle_mutagenesis(o, codes[a:b], 4)
        d, p = _resident(m, a, b, L, 4)
        scale = check_df(d, want, codes[a:b], "cfg2 rows %d..%d" % (a, b))
        check_pll(p, wpll, L, scale, "cfg2")
        assert _bits(p, pll[a:b])
    _, again = _resident(m, 0, n, L, 4, dfe=False)
    assert _bits(pll, again)
    # new parameters: the second call must see them (tables rebuilt before the sweep)
    W2 = (o.W * 0.5).astype(np.float32)
    m.motifs.set_value(W2)
    o.W = W2.astype(np.float64)
    want, wpll = oracle_mutagenesis(o, codes[:16], 4)
    d, p = _resident(m, 0, 16, L, 4)
    scale = check_df(d, want, codes[:16], "cfg2 after set_value")
    check_pll(p, wpll, L, scale, "cfg2 after set_value")
    assert not _bits(p, pll[:16])
