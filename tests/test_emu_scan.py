"""The stream-scan kernels (crbm_kernels.h: scan_encode_kernel, scan_sites_body in both passes, scan_offsets_kernel) on
CPU threads under AddressSanitizer + UBSan (tests/emu/emu_scan.cpp), against the float64 window scorer of
tests/scan_reference.py at the emulation's RTOL: single- and double-stranded models, M = 1, T = M, T < M, motifs in
two and three groups of quads, a 40-letter motif, gaps at tile edges, at positions 0 and T - 1 and longer than a tile,
T no multiple of 16 or 64, a capacity of 3 with guard records behind it, and two launch geometries with the same bits.

The cases run in a subprocess with the sanitizer runtime preloaded: this file is also that subprocess's script."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))   # also when run as the child's script
from tests.emu import harness  # noqa: E402
from tests.emu.harness import fp  # noqa: E402

LIB = "libcrbm_emu_scan.so"
RTOL = 2e-5
REC = np.dtype([("seq", "<i4"), ("motif", "<i4"), ("start", "<i4"), ("strand", "<i4"), ("prob", "<f4")])   # SiteRec


@pytest.fixture(scope="module")
def emu_env():
    harness.build("emu_scan.cpp", LIB)
    return harness.child_env()


CASES = ["ds_10x15", "ss_10x5", "m1", "t_eq_m_and_shorter", "two_quad_groups", "three_quad_groups", "m40",
         "tiny_capacity", "geometries"]


@pytest.mark.parametrize("which", CASES)
def test_scan_kernels_on_cpu_threads_with_sanitizers(emu_env, which):
    r = harness.run_case(os.path.abspath(__file__), which, emu_env, timeout=900)
    assert r.returncode == 0 and "SCAN OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


# ---- the subprocess side -------------------------------------------------------------------------------------------
def gapped_stream(T, seed, M):
    """random letters with gaps where they hurt: positions 0 and T - 1, both sides of the tile (= validity word) edges
    at 64, 128 and 192, a 16-letter word edge, and a run longer than a tile"""
    s = np.random.default_rng(seed).integers(0, 4, size=T, dtype=np.uint8)
    for p in (0, T - 1, 63, 64, 127, 192, 303, 304):
        if 0 <= p < T:
            s[p] = 4
    if T > 520:
        s[400:400 + 70 + M] = 4
    return s


def _tables(lib, cid, o):
    return harness.model_tables(lib.emu_scan_info, lib.emu_scan_tables, cid, o, tables_at=3)


def _run(lib, cid, tables, stream, thr, capacity, grid=2, threads=128, guard=4):
    recs = np.zeros(capacity + guard, REC)
    recs["seq"] = -7                                            # sentinel: nothing may land at or past `capacity`
    count = np.zeros(1, np.uint64)
    flags = np.zeros(4, np.uint32)
    stream = np.ascontiguousarray(stream, np.uint8)
    lib.emu_scan_run.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_long, ctypes.c_float, ctypes.c_void_p,
                                 ctypes.c_ulonglong, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                                 ctypes.c_void_p, ctypes.c_void_p]
    tiles = lib.emu_scan_run(cid, fp(tables), fp(stream), stream.size, thr, fp(recs), capacity, fp(count), fp(flags),
                             grid, threads, None, None)
    assert np.all(recs["seq"][capacity:] == -7), "a record landed past the capacity"
    return recs, int(count[0]), tiles, int(flags[0])


def _check(lib, cid, o, stream, q=0.9):
    from tests.scan_reference import stream_scores, check_records
    tables = _tables(lib, cid, o)
    P, valid = stream_scores(o, stream)
    assert valid.any() and not valid.all()
    thr = float(np.quantile(P[:, :, valid], q))
    cap = int(P.size)
    recs, count, tiles, flags = _run(lib, cid, tables, stream, thr, cap)
    assert flags == 0
    assert int((P >= thr * (1 + RTOL)).sum()) <= count <= int((P >= thr * (1 - RTOL)).sum())
    assert count > 0
    check_records(recs[:count], P, thr, bool(o.doublestranded), RTOL, band_share=1.0)
    assert np.all(recs["seq"][count:cap] == -7)
    # counting alone gives the same total; threshold 0: every valid window, motif and strand
    _, count0, _, _ = _run(lib, cid, tables, stream, thr, 0)
    assert count0 == count
    _, call, _, _ = _run(lib, cid, tables, stream, 0.0, 0)
    assert call == int(valid.sum()) * P.shape[0] * P.shape[1]
    return tables, recs[:count], thr


def run_case(which):
    from tests.scan_reference import stream_scores, check_records
    lib = harness.load(LIB)
    if which == "ds_10x15":
        _check(lib, 0, harness.random_model(10, 15, True, 25), gapped_stream(611, 3, 15))           # T no multiple of 16 or 64
    elif which == "ss_10x5":
        _check(lib, 1, harness.random_model(10, 5, False, 15), gapped_stream(590, 4, 5))
    elif which == "m1":
        _check(lib, 2, harness.random_model(6, 1, True, 7), gapped_stream(330, 5, 1), q=0.6)
    elif which == "two_quad_groups":
        _check(lib, 3, harness.random_model(20, 15, True, 35), gapped_stream(350, 6, 15))
    elif which == "three_quad_groups":
        _check(lib, 4, harness.random_model(36, 6, False, 42), gapped_stream(333, 7, 6))
    elif which == "m40":
        _check(lib, 5, harness.random_model(5, 40, True, 45), gapped_stream(627, 8, 40))
    elif which == "t_eq_m_and_shorter":
        o = harness.random_model(10, 15, True, 25)
        tables = _tables(lib, 0, o)
        one = np.random.default_rng(9).integers(0, 4, size=15, dtype=np.uint8)         # T = M: one window
        P, valid = stream_scores(o, one)
        assert valid.tolist() == [True]
        recs, count, tiles, _ = _run(lib, 0, tables, one, 0.0, 64)
        assert tiles == 1 and count == 20
        check_records(recs[:count], P, 0.0, True, RTOL)
        gap = one.copy()
        gap[7] = 4                                                                        # ... and none valid
        _, count, _, _ = _run(lib, 0, tables, gap, 0.0, 64)
        assert count == 0
        recs, count, tiles, _ = _run(lib, 0, tables, one[:14], 0.0, 64)                  # T < M: nothing runs
        assert tiles == -2 and count == 0
        bad = gapped_stream(100, 1, 15)
        bad[50] = 5                                                                       # a code above 4 raises the flag
        assert _run(lib, 0, tables, bad, 0.5, 8)[3] == 1
    elif which == "tiny_capacity":
        o = harness.random_model(10, 15, True, 25)
        stream = gapped_stream(300, 11, 15)
        tables = _tables(lib, 0, o)
        P, valid = stream_scores(o, stream)
        full, count_full, _, _ = _run(lib, 0, tables, stream, 0.0, int(P.size))
        assert count_full == int(valid.sum()) * 20
        recs, count, _, _ = _run(lib, 0, tables, stream, 0.0, 3, guard=8)                # (_run checks the guard records)
        assert count == count_full
        assert recs[:3].tobytes() == full[:3].tobytes()
    elif which == "geometries":
        o = harness.random_model(20, 15, True, 35)
        stream = gapped_stream(611, 12, 15)
        tables, recs, thr = _check(lib, 3, o, stream)
        other, count, _, _ = _run(lib, 3, tables, stream, thr, recs.size + 5, grid=3, threads=64)
        assert count == recs.size and other[:count].tobytes() == recs.tobytes()
    else:
        raise SystemExit("unknown case " + which)


if __name__ == "__main__":
    run_case(sys.argv[1])
    print("SCAN OK", sys.argv[1])
