"""CPU-only tests of the Markov background surface: header, SIGNATURES and exported symbols agree and the ABI version
stays 5; what fitBackground and sampleBackground refuse is refused before the C side (no device here; the C side's own
checks are the header's *_refusal functions, run by tests/test_emu_background.py, and a null handle); the threshold
table of MarkovBackground, its context indexing, save / load and +."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import background_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_abi_declares_the_background_entry_points():
    import crbm_amd
    from crbm_amd import _lib
    header = open(os.path.join(ROOT, "include", "crbm_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    want = {
        "crbm_stream_kmer_counts": ["crbm_handle* h", "const uint8_t* codes", "int64_t T", "int32_t order", "uint64_t* counts"],
        "crbm_background_sample": ["crbm_handle* h", "const uint32_t* thr", "int32_t order", "int64_t T", "int64_t pos0",
                                   "uint64_t seed", "const uint8_t* tmpl", "uint8_t* out"],
        "crbm_background_ms": ["crbm_handle* h", "float* ms"],
    }
    lib = _lib.load()
    for name, args in want.items():
        decl = re.search(r"\bint %s\((.*?)\);" % name, code, flags=re.S)
        assert decl, name + " is not declared"
        assert [" ".join(a.split()) for a in decl.group(1).split(",")] == args
        res, argtypes = _lib.SIGNATURES[name]
        assert res is ctypes.c_int32 and len(argtypes) == len(args) and getattr(lib, name).argtypes == argtypes
    assert re.search(r"#define\s+CRBM_AMD_ABI_VERSION\s+5\b", header) and _lib.ABI_VERSION == 5      # additive: the version stays
    doc = header[header.index("Markov backgrounds"):header.index("int crbm_stream_kmer_counts(")]
    for word in ("(P & 3)", "P >> 34", "8 << 28", "KIND_BACKGROUND", "empty context", "does not ascend", "CRBM_BG_CHUNK", "CRBM_ERR_INVALID"):
        assert word in doc, word
    layout = open(os.path.join(ROOT, "crbm_amd", "csrc", "crbm_layout.h")).read()
    assert re.search(r"KIND_BACKGROUND\s*=\s*8\b", layout) and R.KIND_BACKGROUND == 8
    got = np.zeros(4, np.uint64)
    s = np.zeros(4, np.uint8)
    assert lib.crbm_stream_kmer_counts(None, s.ctypes.data_as(_lib._U8P), 4, 0, got.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))) == _lib.ERR_INVALID
    assert lib.crbm_background_sample(None, None, 0, 4, 0, 1, None, s.ctypes.data_as(_lib._U8P)) == _lib.ERR_INVALID
    assert lib.crbm_background_ms(None, None) == _lib.ERR_INVALID
    for name in ("MarkovBackground", "fitBackground", "sampleBackground", "background"):
        assert hasattr(crbm_amd, name), name
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in want:
        assert name in integration
    assert '"crbm_background.h"' in open(os.path.join(ROOT, "crbm_amd", "csrc", "build.py")).read()
    jit = open(os.path.join(ROOT, "crbm_amd", "csrc", "crbm_jit.h")).read()
    assert "crbm_background.h" not in jit                        # not part of the per-model source


def _model(monkeypatch):
    """no GPU here: the checks must fire before any call"""
    from crbm_amd import CRBM
    m = CRBM(3, 4, batchsize=8, fantasy_hidden_len=10, seed=1)
    monkeypatch.setattr(m, "_h", lambda: None)
    monkeypatch.setattr(m, "_call", lambda *a: (_ for _ in ()).throw(AssertionError("reached the library")))
    return m


def test_refusals_before_the_c_side(monkeypatch):
    from crbm_amd import fitBackground, sampleBackground, MarkovBackground
    m = _model(monkeypatch)
    s = np.zeros(30, np.uint8)
    for order in (-1, 4, 1.0, True, None):
        with pytest.raises(ValueError, match="order"):
            fitBackground(m, s, order=order)
    bad = s.copy()
    bad[3] = 5
    for stream, why in ((bad, "0..4"), (s.astype(np.int32), "uint8"), (s.reshape(5, 6), "one-dimensional"), ([0, 1], "uint8")):
        with pytest.raises(ValueError, match=why):
            fitBackground(m, stream)
        with pytest.raises(ValueError, match=why):
            sampleBackground(m, stream, R.dirichlet_table(1, 0), 1)
    with pytest.raises(AssertionError, match="reached the library"):
        fitBackground(m, s, order=2)
    good = R.dirichlet_table(1, 0)
    down = good.copy()
    down[3] = [9, 8, 10]
    for table, why in ((good[:4], "contexts"), (good.astype(np.int64), "uint32"), (good[:, :2], "contexts"), (good.ravel(), "contexts"),
                       (down, "does not ascend")):
        with pytest.raises(ValueError, match=why):
            sampleBackground(m, 10, table, 1)
    with pytest.raises(ValueError, match="negative"):
        sampleBackground(m, -1, good, 1)
    with pytest.raises(ValueError, match="seed"):
        sampleBackground(m, 10, good, 1.5)
    with pytest.raises(ValueError, match="cut behind gaps"):
        sampleBackground(m, s, good, 1, _cut=10)                 # no gap to cut behind
    with pytest.raises(ValueError, match="needs a template"):
        sampleBackground(m, 11, good, 1, _cut=10)
    with pytest.raises(AssertionError, match="reached the library"):
        sampleBackground(m, 10, good, 1)
    with pytest.raises(AssertionError, match="reached the library"):
        sampleBackground(m, s, MarkovBackground(1, np.ones(20, np.uint64)), 1)
    for order, counts in ((4, np.zeros(340)), (1, np.zeros(20)), (1, np.zeros(21, np.uint64)), (1, -np.ones(20, np.int64))):
        with pytest.raises(ValueError):
            MarkovBackground(order, counts)
    with pytest.raises(ValueError, match="pseudocount"):
        MarkovBackground(0, np.ones(4, np.uint64)).thresholds(-1.0)


def test_gap_cuts():
    from crbm_amd.background import _gap_cuts
    s = np.zeros(30, np.uint8)
    s[[4, 5, 12, 20, 29]] = 4
    cuts = list(_gap_cuts(s, 10))
    assert cuts == [(0, 6), (6, 13), (13, 21), (21, 30)]
    for lo, hi in cuts[:-1]:
        assert hi - lo <= 10 and s[hi - 1] == 4                  # a piece ends behind a gap
    assert cuts[0][0] == 0 and cuts[-1][1] == 30 and all(a[1] == b[0] for a, b in zip(cuts, cuts[1:]))
    assert list(_gap_cuts(s, 30)) == [(0, 30)] and list(_gap_cuts(s[:0], 5)) == [(0, 0)]


def test_thresholds():
    from crbm_amd.background import MarkovBackground, context_index, contexts, kmer_offset, kmer_slots
    assert [contexts(o) for o in range(4)] == [1, 5, 21, 85] and [kmer_slots(o) for o in range(4)] == [4, 20, 84, 340]
    for letters in ((), (2,), (3, 1), (0, 0), (1, 2, 3), (3, 3, 3)):
        assert context_index(letters) == R.context_index(letters)
    stream = R.gapped_stream(4000, seed=8, gap_share=0.05)
    stream[(stream == 2) & (np.roll(stream, 1) == 1)] = 0        # no CG: a letter the counts never saw in that context
    for order in range(4):
        bg = MarkovBackground(order, R.kmer_counts(stream, order))
        thr = bg.thresholds()
        assert thr.shape == (contexts(order), 3) and thr.dtype == np.uint32
        assert np.all(thr[:, 1:] >= thr[:, :-1])                 # rows ascend
        P = R.probabilities_of(thr)
        assert np.all(P > 0)                                     # the pseudocount keeps every letter possible
        for j in range(order + 1):                               # a context of j letters uses the (j + 1)-mer counts
            n = bg.counts[kmer_offset(j + 1):kmer_offset(j + 2)].reshape(-1, 4).astype(np.float64)
            for v in range(4 ** j):
                letters = [(v >> (2 * (j - 1 - i))) & 3 for i in range(j)]
                p = (n[v] + 1.0) / (n[v].sum() + 4.0)
                want = np.minimum(np.floor(2.0 ** 32 * np.cumsum(p)[:3]), 2.0 ** 32 - 1).astype(np.uint32)
                assert np.array_equal(thr[R.context_index(letters)], want), (order, letters)
        zero = bg.thresholds(pseudocount=0.0)
        assert np.all(zero[:, 1:] >= zero[:, :-1])
        if order >= 1:
            ctx = R.context_index([0] * (order - 1) + [1])       # ... C, then G never: its interval is empty without a pseudocount
            assert zero[ctx][2] == zero[ctx][1] and thr[ctx][2] > thr[ctx][1]
    never = MarkovBackground(1, np.zeros(20, np.uint64)).thresholds(0.0)
    assert np.array_equal(never, np.tile(np.array([2 ** 30, 2 ** 31, 3 * 2 ** 30], np.uint32), (5, 1)))     # nothing seen: uniform
    sure = np.zeros(20, np.uint64)
    sure[3] = 10                                                 # only T: the last threshold stays within 32 bits
    assert MarkovBackground(1, sure).thresholds(0.0)[0].tolist() == [0, 0, 0]
    sure[:] = 0
    sure[0] = 10
    assert MarkovBackground(1, sure).thresholds(0.0)[0].tolist() == [2 ** 32 - 1] * 3


def test_save_load_add(tmp_path):
    from crbm_amd.background import MarkovBackground
    a = MarkovBackground(2, R.kmer_counts(R.gapped_stream(900, seed=1), 2))
    b = MarkovBackground(2, R.kmer_counts(R.gapped_stream(700, seed=2), 2))
    c = a + b
    assert c.order == 2 and np.array_equal(c.counts, a.counts + b.counts) and c.counts.dtype == np.uint64
    path = str(tmp_path / "bg.npz")
    c.save(path)
    d = MarkovBackground.load(path)
    assert d.order == 2 and np.array_equal(d.counts, c.counts) and np.array_equal(d.thresholds(), c.thresholds())
    with pytest.raises(ValueError, match="different order"):
        a + MarkovBackground(1, np.zeros(20, np.uint64))
    with pytest.raises(TypeError):
        a + 1
    assert np.array_equal(a.kmers(2), a.counts[4:20].reshape(4, 4))
