"""The mutagenesis kernels (crbm_kernels.h: mutagenesis_body; crbm_kernels_generic.h: mutagenesis_expand_kernel,
mutagenesis_combine_kernel) on CPU threads under AddressSanitizer + UBSan (tests/emu/emu_mutagenesis.cpp), against the
float64 oracle: want[n,p,a] = L (freeEnergy(v with p -> a) - freeEnergy(v)) and pll from want.  Fused pass: a
double-stranded and a single-stranded model, M = 1, L = M (one window), lengths that are no multiple of 16 or 64,
three position chunks, a motif beyond 32 letters, dF == nullptr and pll == nullptr.  General path: expand, the model's
free-energy pass and combine for a pooled and a double-stranded model, and expand / combine for a 5-letter alphabet.
Guard words around every output stay untouched.

The cases run in a subprocess with the sanitizer runtime preloaded: this file is also that subprocess's script."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))   # also when run as the child's script
from tests.emu import harness  # noqa: E402
from tests.emu.harness import fp  # noqa: E402

LIB = "libcrbm_emu_mutagenesis.so"
RTOL = 2e-5          # the emulation's tolerance (tests/test_emu_sites.py), applied at the scale of the output
GUARD = 8
SENTINEL = np.float32(-12345.5)


@pytest.fixture(scope="module")
def emu_env():
    harness.build("emu_mutagenesis.cpp", LIB)
    return harness.child_env()


CASES = ["ds_10x15", "ss_10x5", "m1", "one_window", "three_chunks", "m40", "general_pool2", "general_ds", "general_alpha5"]


@pytest.mark.parametrize("which", CASES)
def test_mutagenesis_kernels_on_cpu_threads_with_sanitizers(emu_env, which):
    r = harness.run_case(os.path.abspath(__file__), which, emu_env, timeout=900)
    assert r.returncode == 0 and "MUTAGENESIS OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


# ---- the subprocess side -------------------------------------------------------------------------------------------
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


def _setup(lib, cid, o, codes):
    n, L = codes.shape
    tables = harness.model_tables(lib.emu_mut_info, lib.emu_mut_tables, cid, o, tables_at=4)
    letters = np.zeros((n, lib.emu_mut_letter_words(4, L)), np.uint32)
    flags = np.zeros(4, np.uint32)
    lib.emu_mut_encode(fp(_onehot(codes, 4)), fp(letters), fp(flags), n, L)
    assert flags[0] == 0
    return tables, letters, np.ascontiguousarray(o.c.ravel(), dtype=np.float32)


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
    lib = harness.load(LIB)
    if which == "general_alpha5":
        # bytes per letter: the expand kernel against NumPy, the combine kernel on the oracle's per-motif free energies
        A, K, M, n, L = 5, 7, 6, 3, 23
        o = harness.random_model(K, M, False, 5, A=A, draw_c=True)
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
    K, M, DS, POOL = harness.case_info(lib.emu_mut_info, cid)[:4]
    o = harness.random_model(K, M, bool(DS), K + M, pool=POOL, draw_c=True)
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
