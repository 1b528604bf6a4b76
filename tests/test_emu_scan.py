"""The stream-scan kernels (crbm_kernels.h: scan_encode_kernel, scan_sites_body in both passes, scan_offsets_kernel) on
CPU threads under AddressSanitizer + UBSan (tests/emu/emu_scan.cpp), against the float64 window scorer of
tests/scan_reference.py at the emulation's RTOL: single- and double-stranded models, M = 1, T = M, T < M, motifs in
two and three groups of quads, a 40-letter motif, gaps at tile edges, at positions 0 and T - 1 and longer than a tile,
T no multiple of 16 or 64, a capacity of 3 with guard records behind it, and two launch geometries with the same bits.

The cases run in a subprocess with the sanitizer runtime preloaded: this file is also that subprocess's script."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
EMU = os.path.join(HERE, "emu")
CSRC = os.path.join(ROOT, "crbm_amd", "csrc")
LIB = os.path.join(EMU, "libcrbm_emu_scan.so")
SOURCES = [os.path.join(EMU, "emu_scan.cpp"), os.path.join(EMU, "shim", "hip", "hip_runtime.h"),
           os.path.join(CSRC, "crbm_kernels.h"), os.path.join(CSRC, "crbm_kernels_generic.h"), os.path.join(CSRC, "crbm_layout.h")]
RTOL = 2e-5
REC = np.dtype([("seq", "<i4"), ("motif", "<i4"), ("start", "<i4"), ("strand", "<i4"), ("prob", "<f4")])   # SiteRec


def _gcc_file(name):
    return subprocess.check_output(["gcc", "-print-file-name=" + name], text=True).strip()


@pytest.fixture(scope="module")
def emu_env():
    if not os.path.exists(LIB) or any(os.path.getmtime(s) > os.path.getmtime(LIB) for s in SOURCES):
        cmd = ["g++", "-std=c++17", "-O1", "-g1", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
               "-fno-sanitize-recover=undefined", "-mf16c", "-fPIC", "-shared", "-I", os.path.join(EMU, "shim"), "-I", CSRC,
               os.path.join(EMU, "emu_scan.cpp"), "-o", LIB, "-lpthread"]
        subprocess.check_call(cmd)
    env = dict(os.environ)
    env["LD_PRELOAD"] = _gcc_file("libasan.so") + ":" + _gcc_file("libubsan.so")
    env["ASAN_OPTIONS"] = "detect_leaks=0:abort_on_error=1"
    return env


CASES = ["ds_10x15", "ss_10x5", "m1", "t_eq_m_and_shorter", "two_quad_groups", "three_quad_groups", "m40",
         "tiny_capacity", "geometries"]


@pytest.mark.parametrize("which", CASES)
def test_scan_kernels_on_cpu_threads_with_sanitizers(emu_env, which):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), which], env=emu_env, capture_output=True, text=True,
                       timeout=900)
    assert r.returncode == 0 and "SCAN OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


# ---- the subprocess side -------------------------------------------------------------------------------------------
def _oracle(K, M, ds, seed):
    from oracle.crbm_oracle import OracleCRBM
    rng = np.random.default_rng(seed)
    o = OracleCRBM(K, M, doublestranded=ds, batchsize=4, cd_k=1, fantasy_hidden_len=20, seed=1,
                   W=rng.standard_normal((K, 1, 4, M)).astype(np.float32) * 0.7)
    o.b = (o.b + 3.0 + rng.standard_normal((1, K)) * 0.5).astype(np.float32).astype(np.float64)
    return o


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


def _fp(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _tables(lib, cid, o):
    info = (ctypes.c_int * 4)()
    assert lib.emu_scan_info(cid, info) == 0
    K, M, DS, TABLES = list(info)
    assert (K, M, bool(DS)) == (o.num_motifs, o.motif_length, bool(o.doublestranded))
    W = np.ascontiguousarray(o.W.reshape(K, 4, M), dtype=np.float32)
    b = np.ascontiguousarray(o.b.ravel(), dtype=np.float32)
    c = np.ascontiguousarray(o.c.ravel(), dtype=np.float32)
    tables = np.zeros(TABLES, np.float32)
    lib.emu_scan_tables(cid, _fp(W), _fp(b), _fp(c), _fp(tables))
    return tables


def _run(lib, cid, tables, stream, thr, capacity, grid=2, threads=128, guard=4):
    recs = np.zeros(capacity + guard, REC)
    recs["seq"] = -7                                            # sentinel: nothing may land at or past `capacity`
    count = np.zeros(1, np.uint64)
    flags = np.zeros(4, np.uint32)
    stream = np.ascontiguousarray(stream, np.uint8)
    lib.emu_scan_run.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_long, ctypes.c_float, ctypes.c_void_p,
                                 ctypes.c_ulonglong, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                                 ctypes.c_void_p, ctypes.c_void_p]
    tiles = lib.emu_scan_run(cid, _fp(tables), _fp(stream), stream.size, thr, _fp(recs), capacity, _fp(count), _fp(flags),
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
    sys.path.insert(0, ROOT)
    from tests.scan_reference import stream_scores, check_records
    lib = ctypes.CDLL(LIB)
    if which == "ds_10x15":
        _check(lib, 0, _oracle(10, 15, True, 25), gapped_stream(611, 3, 15))           # T no multiple of 16 or 64
    elif which == "ss_10x5":
        _check(lib, 1, _oracle(10, 5, False, 15), gapped_stream(590, 4, 5))
    elif which == "m1":
        _check(lib, 2, _oracle(6, 1, True, 7), gapped_stream(330, 5, 1), q=0.6)
    elif which == "two_quad_groups":
        _check(lib, 3, _oracle(20, 15, True, 35), gapped_stream(350, 6, 15))
    elif which == "three_quad_groups":
        _check(lib, 4, _oracle(36, 6, False, 42), gapped_stream(333, 7, 6))
    elif which == "m40":
        _check(lib, 5, _oracle(5, 40, True, 45), gapped_stream(627, 8, 40))
    elif which == "t_eq_m_and_shorter":
        o = _oracle(10, 15, True, 25)
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
        o = _oracle(10, 15, True, 25)
        stream = gapped_stream(300, 11, 15)
        tables = _tables(lib, 0, o)
        P, valid = stream_scores(o, stream)
        full, count_full, _, _ = _run(lib, 0, tables, stream, 0.0, int(P.size))
        assert count_full == int(valid.sum()) * 20
        recs, count, _, _ = _run(lib, 0, tables, stream, 0.0, 3, guard=8)                # (_run checks the guard records)
        assert count == count_full
        assert recs[:3].tobytes() == full[:3].tobytes()
    elif which == "geometries":
        o = _oracle(20, 15, True, 35)
        stream = gapped_stream(611, 12, 15)
        tables, recs, thr = _check(lib, 3, o, stream)
        other, count, _, _ = _run(lib, 3, tables, stream, thr, recs.size + 5, grid=3, threads=64)
        assert count == recs.size and other[:count].tobytes() == recs.tobytes()
    else:
        raise SystemExit("unknown case " + which)


if __name__ == "__main__":
    run_case(sys.argv[1])
    print("SCAN OK", sys.argv[1])
