"""The annealed-importance-sampling kernel (crbm_kernels.h: ais_body) on CPU threads under AddressSanitizer + UBSan
(tests/emu/emu_ais.cpp) against the float64 yardstick (tests/ais_reference.py): a double-stranded and a single-stranded
model, M = 1, L = M (one hidden position), 70 and 40 motifs (three and two mask words per position) and a motif of 40
letters; 8 temperatures, 6 runs.  The ladder in one segment and as [0,3) + [3,8), in two launch geometries: the same
bits.  Guard bytes around `state` and guard words around `logw` stay untouched.  The final letters equal the
yardstick's, or the run is replayed step by step from the yardstick's states and every differing sample sits on a
|p - u| < 1e-6 tie; the log weights of the other runs lie within the emulation's 2e-5 at the scale of the quantities
differenced (ais_reference.check_against_yardstick).

Runs set aside as tied on the development machine: 0 of 6 in every case.

The cases run in a subprocess with the sanitizer runtime preloaded: this file is also that subprocess's script."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))   # also when run as the child's script
from tests.emu import harness  # noqa: E402
from tests.emu.harness import fp  # noqa: E402

LIB = "libcrbm_emu_ais.so"
RTOL = 2e-5          # the emulation's tolerance (tests/test_emu_sites.py)
GUARD = 16
T, RUNS, SEED = 8, 6, 77


@pytest.fixture(scope="module")
def emu_env():
    harness.build("emu_ais.cpp", LIB)
    return harness.child_env()


# name -> (configuration of emu_ais.cpp, L, base-rate bias of its own?)
CASES = {"ds_10x15": (0, 75, True), "ss_10x5": (1, 83, False), "m1": (2, 37, True), "one_window": (1, 5, False),
         "k70_three_mask_words": (3, 30, False), "k40_ds_two_mask_words": (4, 21, True), "m40": (5, 90, False)}


@pytest.mark.parametrize("which", list(CASES))
def test_ais_kernel_on_cpu_threads_with_sanitizers(emu_env, which):
    r = harness.run_case(os.path.abspath(__file__), which, emu_env, timeout=1800)
    assert r.returncode == 0 and "AIS OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    print(r.stdout[-600:])


# ---- the subprocess side -------------------------------------------------------------------------------------------
def run_case(which):
    from tests import ais_reference as ref
    lib = harness.load(LIB)
    lib.emu_ais_run.argtypes = [ctypes.c_int] + [ctypes.c_void_p] * 5 + [ctypes.c_int] * 4 + [ctypes.c_uint32, ctypes.c_uint64,
                                                                                             ctypes.c_int, ctypes.c_int]
    cid, L, own_base = CASES[which]
    K, M, DS = harness.case_info(lib.emu_ais_info, cid)[:3]
    o = harness.random_model(K, M, bool(DS), K + M, draw_c=True)
    tables = harness.model_tables(lib.emu_ais_info, lib.emu_ais_tables, cid, o, tables_at=3)
    c = np.ascontiguousarray(o.c.ravel(), dtype=np.float32)
    cA = np.log(np.array([0.3, 0.2, 0.15, 0.35])).astype(np.float32) if own_base else c
    betas = np.linspace(0.0, 1.0, T + 1).astype(np.float32)

    def segment(t0, t1, state, logw, runs=RUNS, offset=0, grid=2, threads=128):
        sbuf = np.full(runs * L + 2 * GUARD, 0xEE, np.uint8)
        wbuf = np.full(runs + 2 * GUARD, -12345.5, np.float32)
        if t0 > 0:
            sbuf[GUARD:GUARD + runs * L] = state.ravel()
            wbuf[GUARD:GUARD + runs] = logw
        lds = lib.emu_ais_run(cid, fp(tables), fp(cA), fp(betas), fp(sbuf[GUARD:]), fp(wbuf[GUARD:]), runs, L, t0, t1, offset,
                              SEED, grid, threads)
        assert 0 < lds <= 160 * 1024
        assert np.all(sbuf[:GUARD] == 0xEE) and np.all(sbuf[-GUARD:] == 0xEE)
        assert np.all(wbuf[:GUARD] == -12345.5) and np.all(wbuf[-GUARD:] == -12345.5)
        return sbuf[GUARD:-GUARD].reshape(runs, L).copy(), wbuf[GUARD:-GUARD].copy()

    tied, worst = ref.check_against_yardstick(segment, o, L, RUNS, betas, cA.astype(np.float64), SEED, RTOL, label=which)
    # one segment against [0,3) + [3,8) in another launch geometry (one wave per block, one block per run), and the
    # runs in two calls with run_offset: the same bits
    s_all, w_all = segment(0, T, None, None)
    assert s_all.max() <= 3
    s3, w3 = segment(0, 3, None, None, grid=RUNS, threads=64)
    s8, w8 = segment(3, T, s3, w3, grid=RUNS, threads=64)
    assert np.array_equal(s_all, s8) and np.array_equal(w_all.view(np.uint32), w8.view(np.uint32))
    sa, wa = segment(0, T, None, None, runs=4, grid=1, threads=64)
    sb, wb = segment(0, T, None, None, runs=2, offset=4, grid=1, threads=128)
    assert np.array_equal(s_all, np.concatenate([sa, sb])) and np.array_equal(w_all.view(np.uint32), np.concatenate([wa, wb]).view(np.uint32))
    # state == nullptr: the log weights alone, the same bits
    wbuf = np.full(RUNS, np.nan, np.float32)
    lib.emu_ais_run(cid, fp(tables), fp(cA), fp(betas), None, fp(wbuf), RUNS, L, 0, T, 0, SEED, 2, 128)
    assert np.array_equal(w_all.view(np.uint32), wbuf.view(np.uint32))
    print("tied runs: %d, worst logw error / bound: %.3g" % (tied, worst))


if __name__ == "__main__":
    run_case(sys.argv[1])
    print("AIS OK", sys.argv[1])
