"""The record-summary kernels (crbm_kernels.h: scan_encode_kernel, scan_records_body) and the host's part of
crbm_scan_records_codes (crbm_layout.h: records_unit_exp; crbm_sweep.h: records_check, records_x_max, records_finish) on
CPU threads under AddressSanitizer + UBSan: tests/emu/records_main.cpp, a stand-alone program built here and run
directly, all blocks of a grid at once.  Its outputs are held to the float64 reference of tests/record_reference.py with
check_fe and check_best at the emulation's RTOL: single- and double-stranded models, M = 1, a 40-letter motif, motifs in
two and three groups of quads, a slabbed model whose last slab overlaps its neighbour, record_stream, one record of 700
letters, 300 records of 1..5 letters; several grid and block sizes and two segmentings with an edge inside a window and
inside a record give the same bits; rows of A ++ [4] ++ B are the rows of A then of B.  Guard words around every
accumulator must be intact.  The unit function's overflow bound is checked for a model with x_max = 80."""
import os
import subprocess

import numpy as np
import pytest

from tests.emu import harness
from tests import record_reference as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL = 2e-5
GUARD, GUARD_WORD = 8, 0xA5A5A5A5DEADBEEF
CFG = {0: (10, 15, True), 1: (10, 5, False), 2: (6, 1, True), 3: (20, 15, True), 4: (36, 6, False), 5: (5, 40, True)}
KEYS = ("windows", "letters", "fe", "per_motif", "start", "strand", "prob")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("emu_records") / "records_main")
    emu = os.path.join(ROOT, "tests", "emu")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g1", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                           "-fno-sanitize-recover=undefined", "-mf16c", "-I", os.path.join(emu, "shim"), "-I", emu,
                           "-I", os.path.join(ROOT, "crbm_amd", "csrc"), os.path.join(emu, "records_main.cpp"), "-o", path,
                           "-lpthread"])
    return path


def _run(exe, tmp_path, cid, o, stream, offsets, grid=2, threads=128, seg=0, want=7, expect=0):
    """the outputs of one run of the program as a dict (and `unit`, `sums`, `keys`, `counts`: the raw accumulators)"""
    K, M = o.num_motifs, o.motif_length
    assert CFG[cid][1:] == (M, bool(o.doublestranded)) and K >= CFG[cid][0]
    R = len(offsets) - 1
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(np.array([cid, K, stream.size, R, grid, threads, seg, want], np.int32).tobytes())
        f.write(np.ascontiguousarray(o.W.reshape(K, 4, M), np.float32).tobytes())
        f.write(np.ascontiguousarray(o.b.ravel(), np.float32).tobytes())
        f.write(np.ascontiguousarray(o.c.ravel(), np.float32).tobytes())
        f.write(np.ascontiguousarray(stream, np.uint8).tobytes())
        f.write(np.ascontiguousarray(offsets, np.int64).tobytes())
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=900)      # the inherited environment, as it is
    assert r.returncode == expect, r.stdout[-2000:] + r.stderr[-4000:]
    if expect:
        return r.stderr
    raw = open(fout, "rb").read()
    e = int(np.frombuffer(raw, np.int32, 1)[0])
    cells = R * K
    nacc = 4 * GUARD + 2 * cells + 5 * R
    acc = np.frombuffer(raw, np.uint64, nacc, 4)
    at = [0, GUARD + cells, 2 * GUARD + 2 * cells, 3 * GUARD + 2 * cells + 5 * R]
    for a in at:
        assert np.all(acc[a:a + GUARD] == GUARD_WORD), "a guard word was written"
    out = {"unit": 2.0 ** -e, "sums": acc[GUARD:GUARD + cells].reshape(R, K), "keys": acc[at[1] + GUARD:at[1] + GUARD + cells].reshape(R, K),
           "counts": acc[at[2] + GUARD:at[2] + GUARD + 5 * R].reshape(R, 5)}
    pos = 4 + 8 * nacc
    for name, dt, shape in (("windows", np.int64, (R,)), ("letters", np.int64, (R, 4)), ("fe", np.float32, (R,)),
                            ("per_motif", np.float32, (R, K)), ("start", np.int32, (R, K)), ("strand", np.int32, (R, K)),
                            ("prob", np.float32, (R, K))):
        n = int(np.prod(shape))
        out[name] = np.frombuffer(raw, dt, n, pos).reshape(shape)
        pos += n * np.dtype(dt).itemsize
    assert pos == len(raw)
    return out


def _same(a, b):
    return all(np.array_equal(a[k], b[k]) for k in KEYS + ("sums", "keys", "counts"))


def _check(exe, tmp_path, cid, o, stream, offsets, label, **kw):
    ref = rr.record_summary(o, stream, offsets)
    got = _run(exe, tmp_path, cid, o, stream, offsets, **kw)
    rr.check_fe(got, ref, RTOL, got["unit"], label)
    amb, cells, ties, mirror = rr.check_best(got, ref, RTOL, label)
    print("%s: %d of %d cells ambiguous, %d exact ties, %d mirror ties" % (label, amb, cells, ties, mirror))
    return got, ref


def test_ds_10x15_on_the_record_stream(exe, tmp_path):
    o = harness.random_model(10, 15, True, 25, draw_c=True)
    stream, offsets = rr.record_stream(2031, 15)
    got, ref = _check(exe, tmp_path, 0, o, stream, offsets, "10x15 ds")
    assert (ref["windows"] == 0).sum() >= 4 and ref["windows"].max() > 1400


def test_ss_10x5(exe, tmp_path):
    _check(exe, tmp_path, 1, harness.random_model(10, 5, False, 15, draw_c=True), *rr.record_stream(2031, 5), label="10x5 ss")


def test_m1(exe, tmp_path):
    got, ref = _check(exe, tmp_path, 2, harness.random_model(6, 1, True, 7, draw_c=True), *rr.record_stream(2031, 1), label="6x1 ds")
    assert np.array_equal(got["windows"], got["letters"].sum(axis=1))        # M = 1: every letter is a window


def test_two_and_three_quad_groups_and_m40(exe, tmp_path):
    _check(exe, tmp_path, 3, harness.random_model(20, 15, True, 35, draw_c=True), *rr.record_stream(2031, 15), label="20x15 ds")
    _check(exe, tmp_path, 4, harness.random_model(36, 6, False, 42, draw_c=True), *rr.record_stream(2031, 6), label="36x6 ss")
    _check(exe, tmp_path, 5, harness.random_model(5, 40, True, 45, draw_c=True), *rr.record_stream(2031, 40), label="5x40 ds")


def test_slabs_with_an_overlapping_last_slab(exe, tmp_path):
    """23 motifs as slabs of 10: the last slab is moved back to motifs 13..22 and skips the seven its neighbour owns"""
    _check(exe, tmp_path, 0, harness.random_model(23, 15, True, 51, draw_c=True), *rr.record_stream(2031, 15), label="23x15 ds slabs")


def test_one_long_record_and_many_tiny_ones(exe, tmp_path):
    o = harness.random_model(10, 5, False, 15, draw_c=True)
    rng = np.random.default_rng(77)
    one = rng.integers(0, 4, size=700, dtype=np.uint8)
    got, ref = _check(exe, tmp_path, 1, o, one, np.array([0, 701]), "one record of 700", grid=1, threads=64)
    assert got["windows"].tolist() == [696]
    tiny = [rng.integers(0, 4, size=int(n), dtype=np.uint8) for n in rng.integers(1, 6, size=300)]
    stream, offsets = rr.make_stream(tiny)
    got, ref = _check(exe, tmp_path, 1, o, stream, offsets, "300 records of 1..5")
    assert set(got["windows"].tolist()) == {0, 1}
    o1 = harness.random_model(6, 1, True, 7, draw_c=True)
    _check(exe, tmp_path, 2, o1, stream, offsets, "300 records of 1..5, M = 1")


def test_geometries_and_segmentings_give_the_same_bits(exe, tmp_path):
    """seg = 1000 window starts: edges at 1000, 2000, ... fall inside records and inside windows (a segment's halo is
    the M - 1 letters behind its starts); seg = 777 likewise, and no multiple of a tile"""
    o = harness.random_model(20, 15, True, 35, draw_c=True)
    stream, offsets = rr.record_stream(2031, 15)
    base = _run(exe, tmp_path, 3, o, stream, offsets)
    inside = lambda p: not np.any(offsets == p) and not np.any(offsets == p + 1)
    assert inside(1000) and inside(777) and stream[1000] < 4 and stream[999] < 4
    for grid, threads, seg in ((3, 64, 0), (1, 256, 0), (5, 192, 0), (2, 128, 1000), (3, 64, 777), (64, 64, 0)):
        other = _run(exe, tmp_path, 3, o, stream, offsets, grid=grid, threads=threads, seg=seg)
        assert _same(base, other), (grid, threads, seg)


def test_rows_of_a_concatenation_are_the_rows_of_its_parts(exe, tmp_path):
    o = harness.random_model(10, 15, True, 25, draw_c=True)
    stream, offsets = rr.record_stream(2031, 15)
    recs = rr.split_records(stream, offsets)
    A, B = rr.make_stream(recs[:20]), rr.make_stream(recs[20:])
    whole = _run(exe, tmp_path, 0, o, stream, offsets)
    a, b = _run(exe, tmp_path, 0, o, *A), _run(exe, tmp_path, 0, o, *B, grid=3, threads=64)
    for k in KEYS:
        assert np.array_equal(whole[k], np.concatenate([a[k], b[k]])), k


def test_output_groups_may_be_absent_and_short_streams_count_letters(exe, tmp_path):
    o = harness.random_model(10, 15, True, 25, draw_c=True)
    stream, offsets = rr.record_stream(2031, 15)
    full = _run(exe, tmp_path, 0, o, stream, offsets)
    for want in (1, 2, 4):
        part = _run(exe, tmp_path, 0, o, stream, offsets, want=want)
        for bit, name in ((1, "counts"), (2, "sums"), (4, "keys")):
            assert np.array_equal(part[name], full[name]) if want & bit else not part[name].any(), (want, name)
    short, off = rr.make_stream([np.array([0, 1, 4, 3], np.uint8), np.zeros(0, np.uint8), np.array([2, 2], np.uint8)])
    got = _run(exe, tmp_path, 0, o, short, off)
    assert got["letters"].tolist() == [[1, 1, 0, 1], [0, 0, 0, 0], [0, 0, 2, 0]] and not got["windows"].any()
    assert np.all(got["start"] == -1) and not got["per_motif"].any() and not got["prob"].any()
    c = np.asarray(o.c, np.float32).ravel().astype(np.float64)
    assert np.allclose(got["fe"], -(got["letters"] @ c), rtol=1e-6, atol=0)


def test_bad_record_starts_are_refused(exe, tmp_path):
    o = harness.random_model(10, 15, True, 25)
    stream, offsets = rr.record_stream(2031, 15)
    for bad, word in ((offsets + 1, "start at 0"), (np.concatenate([offsets[:3], offsets[2:]]), "ascend"),
                      (np.concatenate([offsets[:-1], offsets[-1:] + 1]), "T + 1"),
                      (np.concatenate([offsets[:20], offsets[20:21] - 1, offsets[21:]]), "code 4")):
        assert word in _run(exe, tmp_path, 0, o, stream, bad, expect=4)
    five = stream.copy()
    five[5000] = 5
    assert "a code above 4" in _run(exe, tmp_path, 0, o, five, offsets, expect=3)


def test_unit_function_bounds(exe):
    """e is the finest exponent, at most 32, with 2^31 S (max(x_max, 0) + log 2) 2^e < 2^62: the program prints e, whether
    the bound holds at e and whether it fails at e + 1 (or e is 32)"""
    def unit(x_max, S):
        out = subprocess.run([exe, "unit", repr(x_max), str(S)], capture_output=True, text=True, timeout=60)
        assert out.returncode == 0, out.stderr
        e, holds, finest = (int(x) for x in out.stdout.split())
        assert holds == 1 and finest == 1 and e <= 32
        return e
    assert unit(80.0, 2) == 23          # 2 (80 + log 2) = 161.4 < 2^8: 2^31 2^8 2^23 = 2^62
    assert unit(80.0, 1) == 24
    assert unit(-5.0, 1) == 31          # log 2 alone: below 1
    assert unit(0.2, 2) == 30           # 2 (0.2 + log 2) = 1.79 < 2
    assert unit(1e6, 2) == 10
