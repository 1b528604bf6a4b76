"""CPU-only tests of the analytic null's host side (crbm_amd/null.py): header, SIGNATURES and exported symbols agree and
the ABI version stays 5; the position weight matrix against the oracle probed with one-hot windows; quantisation, err and
offset against the contract; next_context and the stationary distribution against tests/null_reference.py; the
ValueError of a reducible chain; the arithmetic of tail_bounds, thresholds, pvalues and binned on a hand-made pmf; the
prob = 1 clip; save / load; what scoreDistribution refuses before the C side.  (The predecessor table is built by
crbm_null.h: tests/test_emu_null.py holds it to next_context.)"""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import null_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_abi_declares_the_entry_points():
    import crbm_amd
    from crbm_amd import _lib
    header = open(os.path.join(ROOT, "include", "crbm_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    want = {
        "crbm_score_distribution": ["crbm_handle* h", "const int32_t* q", "int32_t R", "int32_t M", "int32_t order", "const double* trans",
                                    "const double* init", "int64_t G", "double* pmf"],
        "crbm_null_ms": ["crbm_handle* h", "float* ms"],
    }
    lib = _lib.load()
    for name, args in want.items():
        decl = re.search(r"\bint %s\((.*?)\);" % name, code, flags=re.S)
        assert decl, name + " is not declared"
        assert [" ".join(a.split()) for a in decl.group(1).split(",")] == args
        res, argtypes = _lib.SIGNATURES[name]
        assert res is ctypes.c_int32 and len(argtypes) == len(args) and getattr(lib, name).argtypes == argtypes
    assert re.search(r"#define\s+CRBM_AMD_ABI_VERSION\s+5\b", header) and _lib.ABI_VERSION == 5      # additive: the version stays
    doc = header[header.index("The analytic null"):header.index("int crbm_score_distribution(")]
    for word in ("CRBM_NULL_TILE", "CRBM_NULL_BYTES", "CRBM_NULL_VARIANT", "CRBM_ERR_INVALID", "2^24", "1e-9", "index order"):
        assert word in doc, word
    q = np.zeros((1, 1, 4), np.int32)
    one = np.ones(4)
    dp = ctypes.POINTER(ctypes.c_double)
    assert lib.crbm_score_distribution(None, q.ctypes.data_as(_lib._I32P), 1, 1, 0, (one / 4).ctypes.data_as(dp), one.ctypes.data_as(dp), 1,
                                       one.ctypes.data_as(dp)) == _lib.ERR_INVALID
    assert lib.crbm_null_ms(None, None) == _lib.ERR_INVALID
    for name in ("ScoreDistribution", "scoreDistribution", "null"):
        assert hasattr(crbm_amd, name), name
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in want:
        assert name in integration
    assert '"crbm_null.h"' in open(os.path.join(ROOT, "crbm_amd", "csrc", "build.py")).read()
    assert "crbm_null.h" not in open(os.path.join(ROOT, "crbm_amd", "csrc", "crbm_jit.h")).read()    # not part of the per-model source


def test_next_context_and_contexts():
    from crbm_amd import null
    from crbm_amd.background import contexts, context_index
    for order in range(4):
        assert contexts(order) == R.contexts(order)
        for s in range(contexts(order)):
            for a in range(4):
                assert null.next_context(order, s, a) == R.next_context(order, s, a) == context_index((R.letters_of(s) + [a])[-order:] if order else [])


@pytest.mark.parametrize("ds", [True, False])
def test_window_pwm_is_the_oracles_score(ds):
    from crbm_amd import null
    from tests.test_gpu_parity import make_pair
    m, o = make_pair(3, 6, ds=ds, bshift=1.5)
    w, c = null.window_pwm(m)
    wr, cr = R.window_pwm(o)                                     # relative to the all-A window
    assert w.shape == wr.shape == (3 * (2 if ds else 1), 6, 4) and w.dtype == np.float64
    assert np.abs((w - w[:, :, :1]) - wr).max() < 1e-12
    assert np.abs(c + w[:, :, 0].sum(axis=1) - cr).max() < 1e-12
    Wm = np.asarray(m.motifs.get_value(), np.float64)
    if ds:                                                       # rows are (motif, strand): + then the reverse complement
        assert np.array_equal(w[0], Wm[0, 0].T) and np.array_equal(w[1], Wm[0, 0, ::-1, ::-1].T)
        assert c[0] == c[1] == float(m.bias.get_value()[0, 0])


def test_quantisation_follows_the_contract():
    from crbm_amd import null
    rng = np.random.default_rng(3)
    w, c = rng.standard_normal((5, 7, 4)) * 2.0, rng.standard_normal(5)
    w[2, 3] = 0.4                                                # a position whose four weights quantise equal
    for step in (2.0 ** -10, 2.0 ** -4, 0.3):
        q, offset, err, G = null.quantise(w, c, step)
        assert q.dtype == np.int32 and q.shape == w.shape and q.flags["C_CONTIGUOUS"] and G.dtype == np.int64
        assert np.all(q.min(axis=2) == 0) and np.all(q[2, 3] == 0)
        assert np.all(err <= 7 * step / 2 + 1e-15)
        for r in range(5):
            qr, off_r, err_r, G_r = R.quantise(w[r], c[r], step)
            assert np.array_equal(q[r], qr) and offset[r] == off_r and err[r] == pytest.approx(err_r, abs=1e-15) and G[r] == G_r
        letters = rng.integers(0, 4, size=(200, 7))
        j = np.arange(7)
        for r in range(5):
            x = c[r] + w[r, j, letters].sum(axis=1)
            Q = q[r, j, letters].sum(axis=1)
            assert np.all((Q >= 0) & (Q < G[r])) and np.all(np.abs(x - (offset[r] + step * Q)) <= err[r] + 1e-12)
    with pytest.raises(ValueError, match="step"):
        null.quantise(w * 1e6, c, 2.0 ** -20)


@pytest.mark.parametrize("order", [0, 1, 2, 3])
def test_stationary_against_the_reference(order):
    from crbm_amd import null
    P = R.dirichlet_probabilities(order, 50 + order)
    got = null.stationary(P, order)
    assert got.shape == (R.contexts(order),) and np.abs(got - R.stationary(P, order)).max() < 1e-12
    assert np.all(got[:(4 ** order - 1) // 3] == 0) and abs(got.sum() - 1.0) < 1e-14
    run = null.start_distribution(P, order, "run")
    assert run[0] == 1.0 and run.sum() == 1.0
    with pytest.raises(ValueError, match="start"):
        null.start_distribution(P, order, "middle")


def test_a_reducible_chain_is_refused():
    from crbm_amd import null, MarkovBackground
    from crbm_amd.background import kmer_slots
    counts = np.zeros(kmer_slots(1), np.uint64)
    counts[0], counts[3] = 5, 5                                  # A and T ...
    counts[4 + 0], counts[4 + 15] = 5, 5                         # ... AA and TT only: two closed classes at pseudocount 0
    bg = MarkovBackground(1, counts)
    P = bg.probabilities(0.0)
    with pytest.raises(ValueError) as e:
        null.stationary(P, 1)
    assert "pseudocount" in str(e.value) and 'start="run"' in str(e.value)
    assert abs(null.stationary(bg.probabilities(1.0), 1).sum() - 1.0) < 1e-14


def hand_made():
    from crbm_amd import ScoreDistribution
    pmf = np.zeros((2, 1, 6))
    pmf[0, 0] = [0.5, 0.25, 0.125, 0.0625, 0.03125, 0.03125]
    pmf[1, 0, :3] = [0.9, 0.09, 0.01]                            # a shorter row: zero beyond its own range
    return ScoreDistribution(pmf, [[-2.0], [0.0]], [[0.25], [0.0]], 1.0, False, 2, "stationary")


def test_tail_bounds_arithmetic():
    d = hand_made()
    assert d.G == 6 and d.tail().shape == (2, 1, 7) and np.all(d.tail()[:, 0, 0] == 1.0) and np.all(d.tail()[:, 0, 6] == 0.0)
    lower, upper = d.tail_bounds(0.0)
    # row 0: grid -2, -1, 0, ...; err 0.25: upper = P(grid >= -0.25) = P(Q >= 2), lower = P(grid >= 0.25) = P(Q >= 3)
    assert upper[0, 0] == 0.25 and lower[0, 0] == 0.125
    # row 1: err 0: both P(Q >= 0) = 1
    assert upper[1, 0] == lower[1, 0] == 1.0
    lower, upper = d.tail_bounds(np.array([[100.0], [1.5]]))
    assert upper[0, 0] == lower[0, 0] == 0.0 and upper[1, 0] == lower[1, 0] == pytest.approx(0.01)
    lower, upper = d.tail_bounds(-np.inf)
    assert np.all(lower == 1.0) and np.all(upper == 1.0)


def test_thresholds_arithmetic():
    d = hand_made()
    thr, resolved = d.thresholds(0.07)
    # row 0: the tail 1, .5, .25, .125, .0625, .03125, 0: n = 4, x = -2 + 0.25 + 3 = 1.25; row 1: 1, .1, .01, 0: n = 2, x = 1
    sig = lambda x: np.float32(1.0 / (1.0 + np.exp(-x)))
    assert thr.dtype == np.float32 and thr.shape == (2, 1) and resolved.all()
    assert thr[0, 0] == np.nextafter(sig(1.25), np.float32(1)) and thr[1, 0] == np.nextafter(sig(1.0), np.float32(1))
    thr, resolved = d.thresholds(1.0)
    assert np.all(thr == 0.0) and resolved.all()
    thr, _ = d.thresholds(0.0)                                   # above every score of the row
    assert thr[0, 0] == np.nextafter(sig(-2.0 + 0.25 + 5.0), np.float32(1)) and thr[1, 0] == np.nextafter(sig(2.0), np.float32(1))
    from crbm_amd import ScoreDistribution
    far = ScoreDistribution(d.pmf, d.offset + 40.0, d.err, 1.0, False, 2, "run")
    thr, resolved = far.thresholds(0.07)
    assert np.all(thr == 1.0) and not resolved.any()             # sigmoid(39) is 1 in float32
    for bad in (-0.1, 1.1, "x"):
        with pytest.raises(ValueError, match="fpr"):
            d.thresholds(bad)


def test_pvalues_and_the_saturated_site():
    from crbm_amd import CRBM
    SITE_DTYPE = CRBM.SITE_DTYPE
    d = hand_made()
    sites = np.zeros(5, SITE_DTYPE)
    sites["motif"] = [0, 0, 1, 1, 0]
    sites["strand"] = [0, 1, 0, 0, 0]                            # (strand 1 of a single-stranded record is s = 0)
    logit = np.array([0.0, -1.0, 1.5, -3.0, 0.0])
    sites["prob"] = (1.0 / (1.0 + np.exp(-logit))).astype(np.float32)
    sites["prob"][4] = 1.0                                       # saturated
    p = d.pvalues(sites)
    assert p[0] == 0.25                                          # row 0 at x = 0: P(Q >= 2)
    assert p[1] == 0.5                                           # x = -1: grid >= -1.25: Q >= 1
    assert p[2] == pytest.approx(0.01) and p[3] == 1.0
    x1 = np.log(np.float64(np.nextafter(np.float32(1), np.float32(0)))) - np.log1p(-np.float64(np.nextafter(np.float32(1), np.float32(0))))
    assert 16 < x1 < 17 and p[4] == 0.0                          # the tail at logit(1 - 2^-24), beyond this row's range ...
    from crbm_amd import ScoreDistribution
    wide = ScoreDistribution(d.pmf, d.offset + 15.0, d.err, 1.0, False, 2, "run")
    assert wide.pvalues(sites[4:])[0] == 0.0625                  # ... and inside this one's: 13 + Q >= 16.39: Q >= 4, not 0
    sites["strand"][0] = -1
    with pytest.raises(ValueError, match="double-stranded"):
        d.pvalues(sites)


def test_binned_follows_the_bin_rule():
    from crbm_amd import ScoreHistogram
    d = hand_made()
    b = d.binned(4, -1.5, 2.5)                                   # row 0: grid -2 .. 3: bins 0 0 1 2 3 3; row 1: grid 0 1 2: bins 1 2 3
    assert b.shape == (2, 1, 4)
    assert np.allclose(b[0, 0], [0.75, 0.125, 0.0625, 0.0625]) and np.allclose(b[1, 0], [0.0, 0.9, 0.09, 0.01])
    h = ScoreHistogram(np.zeros((2, 1, 4), np.int64), np.linspace(-1.5, 2.5, 5), 0, False)
    grid = d.offset[0, 0] + d.step * np.arange(6)
    assert np.array_equal(h.bin_of(grid), [0, 0, 1, 2, 3, 3])
    with pytest.raises(ValueError):
        d.binned(0, 0.0, 1.0)
    with pytest.raises(ValueError):
        d.binned(4, 1.0, 1.0)


def test_save_load_round_trip(tmp_path):
    from crbm_amd import ScoreDistribution
    d = hand_made()
    path = str(tmp_path / "null.npz")
    d.save(path)
    e = ScoreDistribution.load(path)
    assert np.array_equal(e.pmf, d.pmf) and np.array_equal(e.offset, d.offset) and np.array_equal(e.err, d.err)
    assert (e.step, e.doublestranded, e.order, e.start) == (1.0, False, 2, "stationary")
    with pytest.raises(ValueError):
        ScoreDistribution(d.pmf, d.offset, d.err, 1.0, True, 2, "run")         # S = 1 is not double-stranded
    with pytest.raises(ValueError):
        ScoreDistribution(-d.pmf, d.offset, d.err, 1.0, False, 2, "run")


def test_refusals_before_the_c_side(monkeypatch):
    import warnings
    from crbm_amd import CRBM, MarkovBackground, scoreDistribution
    from crbm_amd.background import kmer_slots
    bg = MarkovBackground(1, np.ones(kmer_slots(1), np.uint64))

    def model(**kw):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", UserWarning)
            m = CRBM(3, 4, batchsize=8, fantasy_hidden_len=12, seed=1, **kw)
        monkeypatch.setattr(m, "_h", lambda: None)
        monkeypatch.setattr(m, "_call", lambda *a: (_ for _ in ()).throw(AssertionError("reached the library")))
        return m
    with pytest.raises(ValueError, match="pooling"):
        scoreDistribution(model(pooling=2), bg)
    with pytest.raises(ValueError, match="input_dims"):
        scoreDistribution(model(input_dims=20), bg)
    m = model()
    with pytest.raises(ValueError, match="MarkovBackground"):
        scoreDistribution(m, np.zeros((5, 3), np.uint32))
    for step in (0.0, -1.0, float("nan"), None, True):
        with pytest.raises(ValueError, match="step"):
            scoreDistribution(m, bg, step=step)
    with pytest.raises(ValueError, match="start"):
        scoreDistribution(m, bg, start="gap")
    with pytest.raises(ValueError, match="larger step"):
        scoreDistribution(m, bg, step=2.0 ** -30)
    with pytest.raises(AssertionError, match="reached the library"):          # and what is in order goes to the device
        scoreDistribution(m, bg, step=2.0 ** -4)
