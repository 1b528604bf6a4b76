"""Markov backgrounds on the GPU (crbm_amd.fitBackground / sampleBackground, crbm_stream_kmer_counts /
crbm_background_sample) against tests/background_reference.py.  Integers only, so every comparison is equality: the
j-mer counts of gapped streams for every segmenting; samples of order 0..3 bit for bit at chunk lengths 8, 64 and the
default; tables with memory, where restarting a chunk from anything but its true entry context shows; pos0, pieces and
seeds; the consumer (scoreHistogram of the sample); and the refusals."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import background_reference as R
from tests.test_gpu_parity import make_pair

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_U32P = ctypes.POINTER(ctypes.c_uint32)
_U64P = ctypes.POINTER(ctypes.c_uint64)
CHUNKS = [8, 64, None]                                           # None: the default of crbm_background.h


@pytest.fixture(scope="module")
def model():
    """config #2's double-stranded model: it lends its device, and scores the consumer's streams"""
    return make_pair(10, 15, ds=True, Lf=186, bshift=3.0, wscale=0.7)[0]


def _chunk(monkeypatch, chunk):
    if chunk is None:
        monkeypatch.delenv("CRBM_BG_CHUNK", raising=False)
        header = open(os.path.join(ROOT, "crbm_amd", "csrc", "crbm_background.h")).read()
        return int(re.search(r"CHUNK_DEFAULT = (\d+);", header).group(1))
    monkeypatch.setenv("CRBM_BG_CHUNK", str(chunk))
    return chunk


def test_counts_equal_the_reference(model, monkeypatch):
    from crbm_amd import fitBackground
    for T, seed in ((3001, 1), (4999, 2)):
        s = R.gapped_stream(T, seed=seed, gap_share=0.08, max_run=7)
        s[0] = s[-1] = 4                                         # a gap at the first position and at the last
        s[200:210] = [4, 1, 4, 2, 3, 4, 0, 1, 2, 4]              # runs shorter than order + 1
        for order in range(4):
            want = R.kmer_counts(s, order)
            monkeypatch.delenv("CRBM_SLAB_BYTES", raising=False)
            bg = fitBackground(model, s, order=order)
            assert bg.order == order and bg.counts.dtype == np.uint64 and np.array_equal(bg.counts, want)
            for seg in (T // 3 + 1, 700, 64):                    # three segments and more: the halo
                monkeypatch.setenv("CRBM_SLAB_BYTES", str(seg))
                assert np.array_equal(fitBackground(model, s, order=order).counts, want), (order, seg)
            monkeypatch.delenv("CRBM_SLAB_BYTES", raising=False)
            assert np.array_equal(fitBackground(model, s[1:-1], order=order).counts, R.kmer_counts(s[1:-1], order))
            assert np.array_equal(fitBackground(model, s, order=order, _cut=1200).counts, want)     # pieces cut behind gaps
    for order in range(4):
        for T in range(0, order + 2):                            # T < order + 1 and T = 0
            short = (np.arange(T) % 4).astype(np.uint8)
            assert np.array_equal(fitBackground(model, short, order=order).counts, R.kmer_counts(short, order))


def edge_template(T, C):
    """gaps at C - 1, C and C + 1 (of three chunks), a run that begins at a chunk's last position, runs shorter than the
    order, random gap runs"""
    s = R.gapped_stream(T, seed=T + C, gap_share=0.03, max_run=4)
    s[C - 1] = 4
    s[2 * C] = 4
    s[3 * C + 1] = 4
    s[5 * C - 3:5 * C - 1] = 4
    s[5 * C - 1] = 0
    s[6 * C:6 * C + 8] = [4, 0, 4, 1, 2, 4, 3, 4]
    s[9 * C - 1:9 * C + 2] = 4                                   # ... and a gap run across a chunk's edge
    return s


_WANT = {}


def reference(key, table, order, template, seed, pos0=0):
    """the reference's stream, computed once per case and never written to"""
    if key not in _WANT:
        _WANT[key] = R.sample(table, order, template, seed, pos0=pos0)
        _WANT[key].setflags(write=False)
    return _WANT[key]


@pytest.mark.parametrize("chunk", CHUNKS, ids=["c8", "c64", "default"])
@pytest.mark.parametrize("order", [0, 1, 2, 3])
def test_samples_equal_the_reference_bit_for_bit(model, monkeypatch, order, chunk):
    """T leaves the last chunk partial and needs more than one block of 64 lanes at chunk lengths 8 and 64 (T = 8259:
    1033 chunks of 8, 130 of 64, 33 of the default 256); the default's own blocks and groups are
    test_default_chunk_many_blocks"""
    from crbm_amd import sampleBackground
    C = _chunk(monkeypatch, chunk)
    table = R.dirichlet_table(order, 20 + order)
    T = 8259
    for name, template in (("int", T), ("edges", edge_template(T, C))):
        got = sampleBackground(model, template, table, 77 + order)
        assert got.dtype == np.uint8 and np.array_equal(got, reference((order, name, C if name == "edges" else 0), table, order, template, 77 + order))
    for template in (1, np.full(3 * C + 1, 4, np.uint8), np.array([4], np.uint8), 0):      # T = 1, all gaps, T = 0
        assert np.array_equal(sampleBackground(model, template, table, 5), R.sample(table, order, template, 5))


def test_default_chunk_many_blocks(model, monkeypatch):
    """the default chunk length with more than one block and more than one group: 70 001 letters are 274 chunks of 256,
    five blocks of 64 lanes and five groups of 64 chunks"""
    from crbm_amd import sampleBackground
    monkeypatch.delenv("CRBM_BG_CHUNK", raising=False)
    table = R.dirichlet_table(3, 31)
    tmpl = R.gapped_stream(70001, seed=6, gap_share=0.01, max_run=30)
    got = sampleBackground(model, tmpl, table, 123)
    assert np.array_equal(got, reference("default-many", table, 3, tmpl, 123))
    monkeypatch.setenv("CRBM_BG_CHUNK", "8")
    assert np.array_equal(sampleBackground(model, tmpl, table, 123), got)
    monkeypatch.setenv("CRBM_SLAB_BYTES", str(3 * 20011))        # four segments: the context is carried on the device
    assert np.array_equal(sampleBackground(model, tmpl, table, 123), got)


@pytest.mark.parametrize("chunk", CHUNKS, ids=["c8", "c64", "default"])
def test_tables_with_memory(model, monkeypatch, chunk):
    from crbm_amd import sampleBackground
    C = _chunk(monkeypatch, chunk)
    T = 6 * max(C, 64) + 70 * 8 + 5
    gaps = np.zeros(T, np.uint8)
    gaps[3 * C + 2] = 4
    cases = (("dirichlet", R.dirichlet_table(3, 99), 3, T), ("stuck", R.stuck_table(3), 3, T), ("stuck-gap", R.stuck_table(3), 3, gaps),
             ("rotation", R.rotation_table(), 1, T), ("rotation-gap", R.rotation_table(), 1, gaps))
    for name, table, order, template in cases:
        want = reference((name, T, C if "gap" in name else 0), table, order, template, 4)
        assert np.array_equal(sampleBackground(model, template, table, 4), want), name
    rot = sampleBackground(model, T, R.rotation_table(), 4)
    assert np.all(np.diff(rot.astype(np.int64)) % 4 == 1)        # the whole multi-chunk run hangs on its first letter


def test_pos0_pieces_and_seeds(model, monkeypatch):
    from crbm_amd import sampleBackground, _lib
    monkeypatch.setenv("CRBM_BG_CHUNK", "64")
    table = R.dirichlet_table(2, 3)
    tmpl = R.gapped_stream(4000, seed=17, gap_share=0.03, max_run=3)
    whole = sampleBackground(model, tmpl, table, 9)
    assert np.array_equal(whole, reference("pieces", table, 2, tmpl, 9))
    from crbm_amd.background import _gap_cuts
    assert len(list(_gap_cuts(tmpl, 1500))) == 3
    assert np.array_equal(sampleBackground(model, tmpl, table, 9, _cut=1500), whole)         # three pieces, each with its pos0
    pos0 = 2 ** 34 - 6                                           # crosses the carry into counter word 1
    out = np.full(300, 9, np.uint8)
    model._call("crbm_background_sample", table.ctypes.data_as(_U32P), 2, 300, pos0, 9, None, out.ctypes.data_as(_lib._U8P))
    assert np.array_equal(out, R.sample(table, 2, 300, seed=9, pos0=pos0))
    seed = (1 << 63) | 12345
    assert np.array_equal(sampleBackground(model, 300, table, seed), R.sample(table, 2, 300, seed=seed))
    assert np.array_equal(sampleBackground(model, 300, table, seed - (1 << 64)), R.sample(table, 2, 300, seed=seed))


def test_consumer_score_histogram(model):
    """fit -> sample -> scoreHistogram on config #2's double-stranded model: the counts of the device's stream are those
    of the reference's stream"""
    from crbm_amd import fitBackground, sampleBackground
    data = R.sample(R.dirichlet_table(2, 41), 2, R.gapped_stream(6000, seed=9, gap_share=0.02), seed=1)
    bg = fitBackground(model, data, order=3)
    assert np.array_equal(bg.counts, R.kmer_counts(data, 3))
    null = sampleBackground(model, data, bg, seed=2)
    want = R.sample(bg.thresholds(), 3, data, seed=2)
    assert np.array_equal(null, want) and np.array_equal(null == 4, data == 4)
    h, hw = model.scoreHistogram(null, bins=64, lo=-8.0, hi=8.0), model.scoreHistogram(want.copy(), bins=64, lo=-8.0, hi=8.0)
    assert h.windows == hw.windows > 0 and np.array_equal(h.counts, hw.counts)


def test_refusals_leave_outputs_untouched_and_the_handle_usable(model):
    from crbm_amd import _lib, fitBackground, sampleBackground
    lib, h = model._lib, model._h()
    s = np.zeros(50, np.uint8)
    bad = s.copy()
    bad[49] = 5
    table = R.dirichlet_table(1, 0)
    down = table.copy()
    down[4] = [3, 2, 9]
    counts = np.full(340, 7, np.uint64)
    out = np.full(50, 9, np.uint8)
    cp, op, sp, tp = counts.ctypes.data_as(_U64P), out.ctypes.data_as(_lib._U8P), s.ctypes.data_as(_lib._U8P), table.ctypes.data_as(_U32P)

    def refused(rc, why):
        assert rc == _lib.ERR_INVALID and why in lib.crbm_last_error(h).decode(), (rc, lib.crbm_last_error(h))
        assert np.all(counts == 7) and np.all(out == 9)

    for order in (-1, 4):
        refused(lib.crbm_stream_kmer_counts(h, sp, 50, order, cp), "order")
        refused(lib.crbm_background_sample(h, tp, order, 50, 0, 1, None, op), "order")
    refused(lib.crbm_stream_kmer_counts(h, bad.ctypes.data_as(_lib._U8P), 50, 2, cp), "0..4")
    refused(lib.crbm_stream_kmer_counts(h, sp, -1, 2, cp), "stream length")
    refused(lib.crbm_stream_kmer_counts(h, None, 50, 2, cp), "null")
    refused(lib.crbm_stream_kmer_counts(h, sp, 50, 2, None), "null")
    refused(lib.crbm_background_sample(h, tp, 1, 50, 0, 1, bad.ctypes.data_as(_lib._U8P), op), "0..4")
    refused(lib.crbm_background_sample(h, down.ctypes.data_as(_U32P), 1, 50, 0, 1, None, op), "does not ascend")
    refused(lib.crbm_background_sample(h, tp, 1, -1, 0, 1, None, op), "T must")
    refused(lib.crbm_background_sample(h, tp, 1, 50, -1, 1, None, op), "pos0")
    refused(lib.crbm_background_sample(h, None, 1, 50, 0, 1, None, op), "null")
    refused(lib.crbm_background_sample(h, tp, 1, 50, 0, 1, None, None), "null")
    with pytest.raises(ValueError, match="0..4"):
        fitBackground(model, bad)
    with pytest.raises(ValueError, match="contexts"):
        sampleBackground(model, 50, table[:4], 1)
    # and the handle still serves
    assert np.array_equal(fitBackground(model, s, order=1).counts, R.kmer_counts(s, 1))
    assert np.array_equal(sampleBackground(model, 50, table, 1), R.sample(table, 1, 50, 1))
    ms = ctypes.c_float(-1.0)
    assert lib.crbm_background_ms(h, ctypes.byref(ms)) == 0 and ms.value >= 0.0
