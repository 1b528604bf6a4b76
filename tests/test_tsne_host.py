"""CPU-only tests of the t-SNE surface: header, SIGNATURES and exported symbols agree and the ABI version stays 5; what
crbm_amd.tsne, tsneEmbed and runTSNE refuse is refused before the C side (no device here; the C side's own checks are the
header's *_refusal functions, run by tests/test_emu_tsne.py, and a null handle); symmetrize against a dense
(P + P^T) / 2n."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("crbm_tsne_neighbors", "crbm_tsne_affinities", "crbm_tsne_descend", "crbm_tsne_descend_ms")


def test_abi_declares_the_tsne_entry_points():
    import crbm_amd
    from crbm_amd import _lib
    header = open(os.path.join(ROOT, "include", "crbm_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    want = {
        "crbm_tsne_neighbors": ["crbm_handle* h", "const float* X", "int64_t n", "int32_t D", "int32_t k", "int32_t* idx", "float* d2"],
        "crbm_tsne_affinities": ["crbm_handle* h", "const float* d2", "int64_t n", "int32_t k", "float perplexity", "float* p", "float* beta"],
        "crbm_tsne_descend": ["crbm_handle* h", "int64_t n", "const int64_t* indptr", "const int32_t* indices", "const float* values",
                              "float* y", "float* velocity", "float* gains", "int32_t iterations", "float exaggeration",
                              "float learning_rate", "float momentum", "float* grad_last", "double* kl", "double* z"],
        "crbm_tsne_descend_ms": ["crbm_handle* h", "float* ms"],
    }
    lib = _lib.load()
    for name in NAMES:
        decl = re.search(r"\bint %s\((.*?)\);" % name, code, flags=re.S)
        assert decl, name + " is not declared"
        assert [" ".join(a.split()) for a in decl.group(1).split(",")] == want[name]
        res, args = _lib.SIGNATURES[name]
        assert res is ctypes.c_int32 and len(args) == len(want[name]) and getattr(lib, name).argtypes == args
    assert re.search(r"#define\s+CRBM_AMD_ABI_VERSION\s+5\b", header) and _lib.ABI_VERSION == 5      # additive: the version stays
    doc = header[header.index("t-SNE of row features"):header.index("int crbm_tsne_neighbors(")]
    for word in ("utils.py:159-160", "difference form", "(d2, j)", "k > 1024", "log(perplexity)", "2.2e-16", "same bits", "CRBM_ERR_INVALID"):
        assert word in doc, word
    X = np.zeros((4, 2), np.float32)
    idx, d2 = np.zeros((4, 1), np.int32), np.zeros((4, 1), np.float32)
    assert lib.crbm_tsne_neighbors(None, _lib.fptr(X), 4, 2, 1, idx.ctypes.data_as(_lib._I32P), _lib.fptr(d2)) == _lib.ERR_INVALID
    assert lib.crbm_tsne_affinities(None, _lib.fptr(d2), 4, 1, 1.0, _lib.fptr(d2), _lib.fptr(d2)) == _lib.ERR_INVALID
    assert lib.crbm_tsne_descend(None, 4, None, None, None, None, None, None, 1, 1.0, 1.0, 0.5, None, None, None) == _lib.ERR_INVALID
    assert lib.crbm_tsne_descend_ms(None, None) == _lib.ERR_INVALID
    for name in ("tsneEmbed", "symmetrize", "runTSNE", "tsne"):
        assert hasattr(crbm_amd, name), name
    assert "early stopping" in crbm_amd.tsneEmbed.__doc__ and "not" in crbm_amd.tsneEmbed.__doc__
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NAMES[:3]:
        assert name in integration and "utils.py:159-160" in integration
    assert '"crbm_tsne.h"' in open(os.path.join(ROOT, "crbm_amd", "csrc", "build.py")).read()


def _model(monkeypatch):
    """no GPU here: the checks must fire before any call"""
    from crbm_amd import CRBM
    m = CRBM(3, 4, batchsize=8, fantasy_hidden_len=10, seed=1)
    monkeypatch.setattr(m, "_h", lambda: None)
    monkeypatch.setattr(m, "_call", lambda *a: (_ for _ in ()).throw(AssertionError("reached the library")))
    return m


def test_refusals_before_the_c_side(monkeypatch):
    from crbm_amd import tsne, tsneEmbed, runTSNE
    m = _model(monkeypatch)
    X = np.random.default_rng(0).random((40, 3)).astype(np.float32)
    for bad, k, why in ((X[:1], 1, "two rows"), (X, 0, r"\[1, n - 1\]"), (X, 40, r"\[1, n - 1\]"), (X[:, :0], 3, "D must"),
                        (np.zeros((4, 257), np.float32), 2, "D must"), (np.zeros((1100, 2), np.float32), 1025, "above 1024"),
                        (X[0], 3, r"\(n, D\)")):
        with pytest.raises(ValueError, match=why):
            tsne.neighbors(m, bad, k)
    nan = X.copy()
    nan[3, 1] = np.inf
    with pytest.raises(ValueError, match="finite"):
        tsne.neighbors(m, nan, 3)
    d2 = np.abs(X[:, :3])
    for perplexity in (0.0, -1.0, 4.0, np.inf, np.nan):
        with pytest.raises(ValueError, match="perplexity"):
            tsne.affinities(m, d2, perplexity)
    with pytest.raises(ValueError, match="negative or not finite"):
        tsne.affinities(m, -d2, 2.0)
    with pytest.raises(ValueError, match="k must"):
        tsne.affinities(m, np.zeros((3, 3), np.float32), 2.0)
    y, v, g = (np.zeros((4, 2), np.float32) for _ in range(3))
    good = (np.array([0, 1, 2, 3, 4]), np.array([1, 0, 3, 2]), np.full(4, 0.25, np.float32))
    for P, iterations, why in (((good[0] + 1, good[1], good[2]), 1, "start at 0"), ((np.array([0, 2, 1, 3, 4]), good[1], good[2]), 1, "ascend"),
                               ((np.array([0, 1, 2, 3, 5]), good[1], good[2]), 1, "number of values"), ((good[0][:4], good[1], good[2]), 1, "n \\+ 1"),
                               ((good[0], np.array([1, 0, 4, 2]), good[2]), 1, "outside"), ((good[0], np.array([1, 0, -1, 2]), good[2]), 1, "outside"),
                               (good, -1, "iterations")):
        with pytest.raises(ValueError, match=why):
            tsne.descend(m, P, y, v, g, iterations, 1.0, 1.0, 0.5)
    with pytest.raises(ValueError, match="float32"):
        tsne.descend(m, good, y.astype(np.float64), v, g, 1, 1.0, 1.0, 0.5)
    with pytest.raises(ValueError, match="two rows"):
        tsne.descend(m, (np.array([0, 0]), good[1][:0], good[2][:0]), y[:1], v[:1], g[:1], 1, 1.0, 1.0, 0.5)
    with pytest.raises(AssertionError, match="reached the library"):       # and a good call gets that far
        tsne.descend(m, good, y, v, g, 1, 1.0, 1.0, 0.5)
    for kw, why in ((dict(perplexity=40.0), "below the number of rows"), (dict(perplexity=np.nan), "finite and positive"),
                    (dict(perplexity=0.2), r"\[1, 1024\]"), (dict(init="spectral"), "init must"), (dict(init=np.zeros((40, 3))), "two components"),
                    (dict(max_iter=-1), "max_iter"), (dict(learning_rate=0.0), "learning_rate"), (dict(early_exaggeration=0.5), "early_exaggeration")):
        with pytest.raises(ValueError, match=why):
            tsneEmbed(m, X, **kw)
    with pytest.raises(ValueError, match="finite"):
        tsneEmbed(m, nan)
    with pytest.raises(ValueError, match="two rows"):
        tsneEmbed(m, X[:1])
    with pytest.raises(ValueError, match=r"\[1, 1024\]"):
        tsneEmbed(m, np.zeros((2000, 2), np.float32), perplexity=400.0)
    with pytest.raises(AssertionError, match="reached the library"):
        tsneEmbed(m, X, perplexity=5.0)
    with pytest.raises(AssertionError, match="reached the library"):       # runTSNE: the features come from the device
        runTSNE(m, np.zeros((5, 12), np.uint8))


def test_pca_init_scale_and_determinism():
    from crbm_amd.tsne import _pca_init
    X = np.random.default_rng(3).random((50, 6)).astype(np.float32) * np.array([5, 1, 1, 1, 1, 1], np.float32)
    y = _pca_init(X)
    assert y.shape == (50, 2) and y.dtype == np.float32 and abs(y[:, 0].std() - 1e-4) < 1e-9
    assert y[:, 0].std() >= y[:, 1].std() and np.array_equal(y, _pca_init(X.copy()))
    assert abs(np.corrcoef(y[:, 0], X[:, 0])[0, 1]) > 0.95
    assert _pca_init(X[:, :1]).shape == (50, 2)


@pytest.mark.parametrize("n,k,seed", [(2, 1, 0), (7, 3, 1), (60, 9, 2), (300, 90, 3)])
def test_symmetrize_against_dense(n, k, seed):
    from crbm_amd import symmetrize
    rng = np.random.default_rng(seed)
    idx = np.stack([rng.permutation(np.delete(np.arange(n), i))[:k] for i in range(n)]).astype(np.int32)
    p = rng.random((n, k)).astype(np.float32)
    p /= p.sum(axis=1, keepdims=True)
    C = np.zeros((n, n))
    np.put_along_axis(C, idx.astype(np.int64), p.astype(np.float64), axis=1)
    dense = (C + C.T) / (2.0 * n)
    if n > 2:
        assert ((C > 0) & (C.T == 0)).any()                                # one-sided edges
    indptr, indices, values = symmetrize(idx, p)
    assert indptr.dtype == np.int64 and indices.dtype == np.int32 and values.dtype == np.float32
    assert indptr[0] == 0 and indptr[-1] == values.size == indices.size == np.count_nonzero(dense)
    got = np.zeros((n, n))
    for i in range(n):
        cols = indices[indptr[i]:indptr[i + 1]]
        assert np.all(np.diff(cols) > 0)                                   # columns ascend, none twice
        got[i, cols] = values[indptr[i]:indptr[i + 1]]
    assert np.array_equal(got, dense.astype(np.float32).astype(np.float64))
    assert np.array_equal(got, got.T) and abs(values.astype(np.float64).sum() - 1.0) < 1e-6
    again = symmetrize(idx.copy(), p.copy())
    assert all(np.array_equal(a, b) for a, b in zip(again, (indptr, indices, values)))


def test_symmetrize_refuses():
    from crbm_amd import symmetrize
    with pytest.raises(ValueError, match="itself"):
        symmetrize(np.array([[0], [0]]), np.ones((2, 1), np.float32))
    with pytest.raises(ValueError, match="outside"):
        symmetrize(np.array([[1], [2]]), np.ones((2, 1), np.float32))
    with pytest.raises(ValueError, match=r"\(n, k\)"):
        symmetrize(np.array([[1], [0]]), np.ones((2, 2), np.float32))
