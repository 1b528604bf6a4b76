"""The score-histogram kernels (crbm_kernels.h: scan_encode_kernel, scan_hist_body) on CPU threads under
AddressSanitizer + UBSan: tests/emu/hist_main.cpp, a stand-alone program built here and run directly, all blocks of a
grid at once.  Its counts are held to the float64 reference with tests/hist_reference.check_histogram at the
emulation's RTOL (the 1 % cap on scores inside the bands lifted, as tests/test_emu_scan.py lifts its own): single- and
double-stranded models, M = 1, T = M and T < M, motifs in two and three groups of quads, a 40-letter motif, 1 and 1024
bins, counters that do not fit at once (the walk over groups of quads, also with fewer quads than a gather holds), the
three ways a wave spreads its adds, several grid and block sizes with the same bits, a slabbed model whose last slab
overlaps its neighbour, gaps at tile and word edges.  Guard words around the counts must be intact."""
import os
import subprocess

import numpy as np
import pytest

from tests.emu import harness
from tests.hist_reference import stream_logodds, check_histogram
from tests.test_emu_scan import gapped_stream

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL = 2e-5
GUARD, GUARD_WORD = 8, 0xA5A5A5A5DEADBEEF
CFG = {0: (10, 15, True), 1: (10, 5, False), 2: (6, 1, True), 3: (20, 15, True), 4: (36, 6, False), 5: (5, 40, True)}


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("emu_hist") / "hist_main")
    emu = os.path.join(ROOT, "tests", "emu")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g1", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                           "-fno-sanitize-recover=undefined", "-mf16c", "-I", os.path.join(emu, "shim"), "-I", emu,
                           "-I", os.path.join(ROOT, "crbm_amd", "csrc"), os.path.join(emu, "hist_main.cpp"), "-o", path,
                           "-lpthread"])
    return path


def _run(exe, tmp_path, cid, o, stream, lo, hi, nbins, grid=2, threads=128, variant=1, gq=0):
    """counts (K, S, nbins) and the valid windows of one run of the program"""
    K, M = o.num_motifs, o.motif_length
    S = 2 if o.doublestranded else 1
    assert CFG[cid][1:] == (M, bool(o.doublestranded)) and K >= CFG[cid][0]
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(np.array([cid, K, stream.size, nbins, grid, threads, variant, gq], np.int32).tobytes())
        f.write(np.array([lo, hi], np.float32).tobytes())
        f.write(np.ascontiguousarray(o.W.reshape(K, 4, M), np.float32).tobytes())
        f.write(np.ascontiguousarray(o.b.ravel(), np.float32).tobytes())
        f.write(np.ascontiguousarray(o.c.ravel(), np.float32).tobytes())
        f.write(np.ascontiguousarray(stream, np.uint8).tobytes())
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=900)      # the inherited environment, as it is
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    out = np.fromfile(fout, np.uint64)
    cells = K * S * nbins
    assert out.size == cells + 1 + 2 * GUARD
    assert np.all(out[:GUARD] == GUARD_WORD) and np.all(out[GUARD + cells + 1:] == GUARD_WORD), "a guard word was written"
    return out[GUARD:GUARD + cells].reshape(K, S, nbins).astype(np.int64), int(out[GUARD + cells])


def _check(exe, tmp_path, cid, o, stream, lo=-8.0, hi=8.0, nbins=64, **kw):
    X, valid = stream_logodds(o, stream)
    assert valid.any() and not valid.all()
    counts, windows = _run(exe, tmp_path, cid, o, stream, lo, hi, nbins, **kw)
    check_histogram(counts, windows, X, valid, lo, hi, nbins, rtol=RTOL, band_share=1.0)
    return counts, windows


def test_ds_10x15(exe, tmp_path):
    counts, _ = _check(exe, tmp_path, 0, harness.random_model(10, 15, True, 25), gapped_stream(611, 3, 15))
    assert counts[:, :, 0].sum() > 0 and (counts[:, :, 1:-1] > 0).sum() > 50        # clamped scores, and a spread


def test_ss_10x5(exe, tmp_path):
    _check(exe, tmp_path, 1, harness.random_model(10, 5, False, 15), gapped_stream(590, 4, 5))


def test_m1(exe, tmp_path):
    _check(exe, tmp_path, 2, harness.random_model(6, 1, True, 7), gapped_stream(330, 5, 1))


def test_t_eq_m_and_shorter(exe, tmp_path):
    o = harness.random_model(10, 15, True, 25)
    one = np.random.default_rng(9).integers(0, 4, size=15, dtype=np.uint8)           # T = M: one window
    X, valid = stream_logodds(o, one)
    assert valid.tolist() == [True]
    counts, windows = _run(exe, tmp_path, 0, o, one, -8.0, 8.0, 64)
    check_histogram(counts, windows, X, valid, -8.0, 8.0, 64, rtol=RTOL, band_share=1.0)
    assert windows == 1
    gap = one.copy()
    gap[7] = 4                                                                        # ... and none valid
    counts, windows = _run(exe, tmp_path, 0, o, gap, -8.0, 8.0, 64)
    assert windows == 0 and not counts.any()
    counts, windows = _run(exe, tmp_path, 0, o, one[:14], -8.0, 8.0, 64)              # T < M: nothing runs
    assert windows == 0 and not counts.any()


def test_two_quad_groups(exe, tmp_path):
    _check(exe, tmp_path, 3, harness.random_model(20, 15, True, 35), gapped_stream(350, 6, 15))


def test_three_quad_groups(exe, tmp_path):
    _check(exe, tmp_path, 4, harness.random_model(36, 6, False, 42), gapped_stream(333, 7, 6))


def test_m40(exe, tmp_path):
    _check(exe, tmp_path, 5, harness.random_model(5, 40, True, 45), gapped_stream(627, 8, 40))


def test_one_bin_and_1024_bins_walk_the_quad_groups(exe, tmp_path):
    """20 x 15 ds at 1024 bins: a quad's counters take 32 KB, four quads fit beside the table, the fifth is a second
    group.  The same bits as with the groups forced to 1, 2 and 3 quads (fewer than the four of a gather: the gather
    is repeated); at 64 bins all five quads fit, and forced groups of 1, 3 and 4 quads give the same bits again."""
    o = harness.random_model(20, 15, True, 35)
    stream = gapped_stream(350, 6, 15)
    X, valid = stream_logodds(o, stream)
    counts, windows = _run(exe, tmp_path, 3, o, stream, 0.0, 1.0, 1)
    assert windows == valid.sum() and np.all(counts == windows) and counts.shape == (20, 2, 1)
    big, _ = _check(exe, tmp_path, 3, o, stream, lo=-16.0, hi=16.0, nbins=1024)
    for gq in (1, 2, 3):
        assert np.array_equal(big, _run(exe, tmp_path, 3, o, stream, -16.0, 16.0, 1024, gq=gq)[0]), gq
    small, _ = _check(exe, tmp_path, 3, o, stream)
    for gq in (1, 3, 4):
        assert np.array_equal(small, _run(exe, tmp_path, 3, o, stream, -8.0, 8.0, 64, gq=gq)[0]), gq
    # its 16-to-1 re-binning is a 64-bin histogram over the same range: held to the reference, not to equality with a
    # run at 64 bins (x - lo is rounded before it is scaled, so the two runs may part at an edge)
    check_histogram(big.reshape(20, 2, 64, 16).sum(axis=3), int(valid.sum()), X, valid, -16.0, 16.0, 64, rtol=RTOL, band_share=1.0)


def test_geometries_and_variants_give_the_same_bits(exe, tmp_path):
    o = harness.random_model(20, 15, True, 35)
    stream = gapped_stream(611, 12, 15)
    counts, _ = _check(exe, tmp_path, 3, o, stream)
    for grid, threads, variant in ((3, 64, 1), (1, 256, 1), (2, 128, 0), (2, 256, 2), (5, 64, 2)):
        other, _ = _run(exe, tmp_path, 3, o, stream, -8.0, 8.0, 64, grid=grid, threads=threads, variant=variant)
        assert np.array_equal(counts, other), (grid, threads, variant)


def test_slabs_with_an_overlapping_last_slab(exe, tmp_path):
    """23 motifs as slabs of 10: the last slab is moved back to motifs 13..22 and skips the seven its neighbour counts;
    6-letter motifs single-stranded likewise, 80 motifs as slabs of 36"""
    _check(exe, tmp_path, 0, harness.random_model(23, 15, True, 51), gapped_stream(350, 13, 15))
    _check(exe, tmp_path, 4, harness.random_model(80, 6, False, 52), gapped_stream(333, 14, 6), nbins=1024, lo=-16.0, hi=16.0)


def test_hist_plan_budget_and_the_refusal_of_a_table_that_leaves_no_room(exe):
    """hist_plan (crbm_layout.h) is what the driver launches with and refuses by (gq == 0: CRBM_ERR_INVALID).  A quad's
    counters take 16 S nbins bytes; table + counters + one word stay within 160 KB; all quads when they fit, else a
    multiple of the gather's four, else what fits, else 0; extra counter sets only while they cost no extra group.
    The refusal needs a gather table above 128 KB - 4 at 1024 bins double-stranded (above 144 KB - 4 single-stranded): a
    served model may have one (tables up to 160 KB are served), so the refusal is real, not dead code."""
    def plan(tab, NQ, S, nbins, copies=1):
        out = subprocess.run([exe, "plan"] + [str(x) for x in (tab, NQ, S, nbins, copies)], capture_output=True, text=True, timeout=60)
        assert out.returncode == 0, out.stderr
        gq, c, lds = (int(x) for x in out.stdout.split())
        assert lds == tab + 16 * S * nbins * gq * c + 4 and lds <= 160 * 1024
        return gq, c
    assert plan(15360, 3, 2, 512) == (3, 1)                       # config #2 double-stranded: everything resident
    assert plan(10240, 5, 2, 1024) == (4, 1)                      # 20 x 15 ds: four quads of 32 KB, the fifth a second group
    assert plan(61440, 15, 1, 1024) == (4, 1)                     # 60 x 10 slab model on a 60 KB table: 6 fit, 4 are used
    assert plan(100000, 15, 2, 1024) == (1, 1)                    # fewer than a gather's four
    assert plan(128 * 1024 - 4, 5, 2, 1024) == (1, 1) and plan(128 * 1024, 5, 2, 1024) == (0, 1)
    assert plan(150000, 5, 2, 1024) == (0, 1) and plan(150000, 5, 2, 64) == (5, 1)
    assert plan(15360, 3, 2, 512, 8) == (3, 3) and plan(15360, 3, 2, 64, 8) == (3, 8) and plan(10240, 5, 2, 1024, 8) == (4, 1)
