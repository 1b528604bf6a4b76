"""The mutagenesis kernels (crbm_kernels.h: mutagenesis_body; crbm_kernels_generic.h: mutagenesis_expand_kernel,
mutagenesis_combine_kernel) on CPU threads under AddressSanitizer + UBSan (tests/emu/emu_mutagenesis.cpp), against the
float64 oracle: want[n,p,a] = L (freeEnergy(v with p -> a) - freeEnergy(v)) and pll from want.  Fused pass: a
double-stranded and a single-stranded model, M = 1, L = M (one window), lengths that are no multiple of 16 or 64,
three position chunks, a motif beyond 32 letters, dF == nullptr and pll == nullptr.  General path: expand, the model's
free-energy pass and combine for a pooled and a double-stranded model, and expand / combine for a 5-letter alphabet.
Guard words around every output stay untouched.

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
LIB = os.path.join(EMU, "libcrbm_emu_mutagenesis.so")
SOURCES = [os.path.join(EMU, "emu_mutagenesis.cpp"), os.path.join(EMU, "shim", "hip", "hip_runtime.h"),
           os.path.join(CSRC, "crbm_kernels.h"), os.path.join(CSRC, "crbm_kernels_generic.h"), os.path.join(CSRC, "crbm_layout.h")]
RTOL = 2e-5          # the emulation's tolerance (tests/test_emu_sites.py), applied at the scale of the output
GUARD = 8
SENTINEL = np.float32(-12345.5)


def _gcc_file(name):
    return subprocess.check_output(["gcc", "-print-file-name=" + name], text=True).strip()


@pytest.fixture(scope="module")
def emu_env():
    if not os.path.exists(LIB) or any(os.path.getmtime(s) > os.path.getmtime(LIB) for s in SOURCES):
        cmd = ["g++", "-std=c++17", "-O1", "-g1", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
               "-fno-sanitize-recover=undefined", "-mf16c", "-fPIC", "-shared", "-I", os.path.join(EMU, "shim"), "-I", CSRC,
               os.path.join(EMU, "emu_mutagenesis.cpp"), "-o", LIB, "-lpthread"]
        subprocess.check_call(cmd)
    env = dict(os.environ)
    env["LD_PRELOAD"] = _gcc_file("libasan.so") + ":" + _gcc_file("libubsan.so")
    env["ASAN_OPTIONS"] = "detect_leaks=0:abort_on_error=1"
    return env


CASES = ["ds_10x15", "ss_10x5", "m1", "one_window", "three_chunks", "m40", "general_pool2", "general_ds", "general_alpha5"]


@pytest.mark.parametrize("which", CASES)
def test_mutagenesis_kernels_on_cpu_threads_with_sanitizers(emu_env, which):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), which], env=emu_env, capture_output=True, text=True,
                       timeout=900)
    assert r.returncode == 0 and "MUTAGENESIS OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


# ---- the subprocess side -------------------------------------------------------------------------------------------
def _oracle(K, M, ds, pool, seed, A=4):
    sys.path.insert(0, ROOT)
    from oracle.crbm_oracle import OracleCRBM
    rng = np.random.default_rng(seed)
    kw = {"input_dims": A} if A != 4 else {}
    o = OracleCRBM(K, M, doublestranded=ds, batchsize=4, cd_k=1, fantasy_hidden_len=20, seed=1, pooling=pool,
                   W=rng.standard_normal((K, 1, A, M)).astype(np.float32) * 0.7, **kw)
    o.b = (o.b + 3.0 + rng.standard_normal((1, K)) * 0.5).astype(np.float32).astype(np.float64)
    o.c = (rng.standard_normal((1, A)) * 0.3).astype(np.float32).astype(np.float64)
    return o


def _onehot(codes, A):
    return np.ascontiguousarray(np.eye(A, dtype=np.float32)[codes].transpose(0, 2, 1)[:, None])


def oracle_mutagenesis(o, codes, A):
    """want (n,L,A) float64 = L (freeEnergy(v with p -> a) - freeEnergy(v)), and pll (n) from it"""
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
    mn = d.min(axis=2, keepdims=True)
    return -(np.log(np.exp(-(d - mn)).sum(axis=2)) - mn[..., 0]).sum(axis=1)


def check(dfe, pll, want, wpll, codes):
    n, L, A = want.shape
    scale = np.abs(want).max()
    if dfe is not None:
        err = np.abs(dfe - want)
        assert np.all(err <= RTOL * np.abs(want) + RTOL * scale), (err.max(), scale)
        own = dfe[np.arange(n)[:, None], np.arange(L)[None, :], codes]
        assert np.all(own == 0.0) and not np.any(np.signbit(own))
    if pll is not None:
        np.testing.assert_allclose(pll, wpll, rtol=RTOL, atol=2 * RTOL * L * scale)
        assert np.all(pll <= 0)


def _guarded(shape):
    """an output with GUARD sentinel floats on either side: (whole buffer, view of the payload)"""
    size = int(np.prod(shape))
    buf = np.full(size + 2 * GUARD, SENTINEL, np.float32)
    return buf, buf[GUARD:GUARD + size].reshape(shape)


def _guards_ok(buf):
    return np.all(buf[:GUARD] == SENTINEL) and np.all(buf[-GUARD:] == SENTINEL)


fp = lambda a: a.ctypes.data_as(ctypes.c_void_p)


def _setup(lib, cid, o, codes):
    info = (ctypes.c_int * 6)()
    lib.emu_mut_info(cid, info)
    K, M, DS, POOL, TABLES, TAB = list(info)
    n, L = codes.shape
    W = np.ascontiguousarray(o.W.reshape(K, 4, M), dtype=np.float32)
    b = np.ascontiguousarray(o.b.ravel(), dtype=np.float32)
    c = np.ascontiguousarray(o.c.ravel(), dtype=np.float32)
    tables = np.zeros(TABLES, np.float32)
    lib.emu_mut_tables(cid, fp(W), fp(b), fp(c), fp(tables))
    letters = np.zeros((n, lib.emu_mut_letter_words(4, L)), np.uint32)
    flags = np.zeros(4, np.uint32)
    lib.emu_mut_encode(fp(_onehot(codes, 4)), fp(letters), fp(flags), n, L)
    assert flags[0] == 0
    return tables, letters, c


def run_fused(lib, cid, tables, letters, n, L, want_dfe=True, want_pll=True, grid=2, threads=128):
    dbuf, dfe = _guarded((n, L, 4))
    pbuf, pll = _guarded((n,))
    lib.emu_mut_run(cid, fp(tables), fp(letters), n, L, fp(dbuf[GUARD:]) if want_dfe else None,
                    fp(pbuf[GUARD:]) if want_pll else None, grid, threads)
    assert _guards_ok(dbuf) and _guards_ok(pbuf)
    if not want_dfe:
        assert np.all(dbuf == SENTINEL)
    if not want_pll:
        assert np.all(pbuf == SENTINEL)
    return (dfe.copy() if want_dfe else None), (pll.copy() if want_pll else None)


def run_general(lib, cid, tables, letters, c, n, L, K):
    per = 1 + 3 * L
    LW = letters.shape[1]
    ebuf = np.full(n * per * LW + 2 * GUARD, 0xDEADBEEF, np.uint32)
    lib.emu_mut_expand(fp(letters), fp(ebuf[GUARD:]), n, L, 4, 2, 128)
    assert np.all(ebuf[:GUARD] == 0xDEADBEEF) and np.all(ebuf[-GUARD:] == 0xDEADBEEF)
    rows = np.ascontiguousarray(ebuf[GUARD:-GUARD].reshape(n * per, LW))
    fem = np.zeros((n * per, K), np.float32)
    lib.emu_mut_free_energy(cid, fp(tables), fp(rows), n * per, L, fp(fem), 2, 128)
    dbuf, dfe = _guarded((n, L, 4))
    pbuf, pll = _guarded((n,))
    lib.emu_mut_combine(fp(fem), fp(c), fp(letters), n, L, 4, K, fp(dbuf[GUARD:]), fp(pbuf[GUARD:]), 2, 128)
    assert _guards_ok(dbuf) and _guards_ok(pbuf)
    # pll alone: nothing of the dense array is written, the same bits
    dbuf2, _ = _guarded((n, L, 4))
    pbuf2, pll2 = _guarded((n,))
    lib.emu_mut_combine(fp(fem), fp(c), fp(letters), n, L, 4, K, None, fp(pbuf2[GUARD:]), 1, 64)
    assert np.all(dbuf2 == SENTINEL) and np.array_equal(pll2.view(np.uint32), pll.view(np.uint32))
    return dfe.copy(), pll.copy(), rows


def unpack_rows(rows, L, A):
    if A == 4:
        p = np.arange(L)
        return ((rows[:, p >> 4] >> (2 * (p & 15)).astype(np.uint32)) & 3).astype(np.uint8)
    return rows.view(np.uint8)[:, :L].copy()


def expected_copies(codes, A):
    n, L = codes.shape
    out = np.repeat(codes[:, None, :], 1 + (A - 1) * L, axis=1)
    for p in range(L):
        for x in range(1, A):
            out[:, 1 + p * (A - 1) + (x - 1), p] = (codes[:, p] + x) % A
    return out.reshape(-1, L)


def run_case(which):
    sys.path.insert(0, ROOT)
    lib = ctypes.CDLL(LIB)
    if which == "general_alpha5":
        # bytes per letter: the expand kernel against NumPy, the combine kernel on the oracle's per-motif free energies
        A, K, M, n, L = 5, 7, 6, 3, 23
        o = _oracle(K, M, False, 1, seed=5, A=A)
        codes = np.random.default_rng(8).integers(0, A, size=(n, L), dtype=np.uint8)
        LW = lib.emu_mut_letter_words(A, L)
        letters = np.zeros((n, LW), np.uint32)
        letters.view(np.uint8)[:, :L] = codes
        per = 1 + (A - 1) * L
        ebuf = np.full(n * per * LW + 2 * GUARD, 0xDEADBEEF, np.uint32)
        lib.emu_mut_expand(fp(letters), fp(ebuf[GUARD:]), n, L, A, 2, 128)
        assert np.all(ebuf[:GUARD] == 0xDEADBEEF) and np.all(ebuf[-GUARD:] == 0xDEADBEEF)
        rows = np.ascontiguousarray(ebuf[GUARD:-GUARD].reshape(n * per, LW))
        got = unpack_rows(rows, L, A)
        assert np.array_equal(got, expected_copies(codes, A))
        assert np.all(rows.view(np.uint8)[:, L:] == 0)
        fem = np.ascontiguousarray(o.freeEnergy(_onehot(got, A), True), dtype=np.float32)
        c = np.ascontiguousarray(o.c.ravel(), dtype=np.float32)
        dbuf, dfe = _guarded((n, L, A))
        pbuf, pll = _guarded((n,))
        lib.emu_mut_combine(fp(fem), fp(c), fp(letters), n, L, A, K, fp(dbuf[GUARD:]), fp(pbuf[GUARD:]), 2, 128)
        assert _guards_ok(dbuf) and _guards_ok(pbuf)
        want, wpll = oracle_mutagenesis(o, codes, A)
        check(dfe, pll, want, wpll, codes)
        return
    cid, n, L = {"ds_10x15": (0, 5, 75), "ss_10x5": (1, 5, 83), "m1": (2, 4, 37), "one_window": (0, 3, 15),
                 "three_chunks": (3, 3, 150), "m40": (4, 3, 90), "general_pool2": (5, 3, 48), "general_ds": (0, 3, 45)}[which]
    info = (ctypes.c_int * 6)()
    lib.emu_mut_info(cid, info)
    K, M, DS, POOL, _, _ = list(info)
    o = _oracle(K, M, bool(DS), POOL, seed=K + M)
    codes = np.random.default_rng(K * 3 + L).integers(0, 4, size=(n, L), dtype=np.uint8)
    tables, letters, c = _setup(lib, cid, o, codes)
    want, wpll = oracle_mutagenesis(o, codes, 4)
    if which.startswith("general"):
        dfe, pll, rows = run_general(lib, cid, tables, letters, c, n, L, K)
        assert np.array_equal(unpack_rows(rows, L, 4), expected_copies(codes, 4))
        check(dfe, pll, want, wpll, codes)
        if POOL == 1:
            f_dfe, f_pll = run_fused(lib, cid, tables, letters, n, L)
            check(f_dfe, f_pll, want, wpll, codes)
        return
    dfe, pll = run_fused(lib, cid, tables, letters, n, L)
    check(dfe, pll, want, wpll, codes)
    # pll alone (dF == nullptr) and dF alone: the same bits, nothing else written; another launch geometry: the same bits
    _, pll2 = run_fused(lib, cid, tables, letters, n, L, want_dfe=False)
    dfe2, _ = run_fused(lib, cid, tables, letters, n, L, want_pll=False)
    dfe3, pll3 = run_fused(lib, cid, tables, letters, n, L, grid=1, threads=64)
    for a, b in ((pll, pll2), (dfe, dfe2), (dfe, dfe3), (pll, pll3)):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


if __name__ == "__main__":
    run_case(sys.argv[1])
    print("MUTAGENESIS OK", sys.argv[1])
