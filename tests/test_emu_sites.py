"""The motif-site kernels (crbm_kernels.h: motif_sites_body, motif_sites_select_kernel) on CPU threads under
AddressSanitizer + UBSan (tests/emu/emu_sites.cpp), against the float64 oracle: thresholded records (complete, none
below the threshold, exact count past a tiny capacity, writes only below it) and best sites (tie rule) of
double-stranded, pooled and single-stranded models, and of a sequence long enough for two position chunks.

The cases run in a subprocess with the sanitizer runtime preloaded: this file is also that subprocess's script."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))   # also when run as the child's script
from tests.emu import harness  # noqa: E402
from tests.emu.harness import fp  # noqa: E402

LIB = "libcrbm_emu_sites.so"
RTOL = 2e-5
REC = np.dtype([("seq", "<i4"), ("motif", "<i4"), ("start", "<i4"), ("strand", "<i4"), ("prob", "<f4")])   # SiteRec


@pytest.fixture(scope="module")
def emu_env():
    harness.build("emu_sites.cpp", LIB)
    return harness.child_env()


CASES = ["ds_10x15", "ds_6x7_pool2", "ss_10x5", "two_chunks", "tiny_capacity", "select"]


@pytest.mark.parametrize("which", CASES)
def test_site_kernels_on_cpu_threads_with_sanitizers(emu_env, which):
    r = harness.run_case(os.path.abspath(__file__), which, emu_env, timeout=900)
    assert r.returncode == 0 and "SITES OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


# ---- the subprocess side -------------------------------------------------------------------------------------------
def oracle_scores(o, D):
    """(S, n, K, Lh) float64: the + (or single) strand, then the reverse-complemented filter"""
    if o.doublestranded:
        P = [o._bottomUpProbability(o._bottomUpActivity(D)), o._bottomUpProbability(o._bottomUpActivity(D, True))]
    else:
        P = [o.motifHitProbs(D)]
    return np.stack([p[:, :, 0, :] for p in P])


def check_records(recs, P, thr, ds, complete=True):
    """every record is an oracle site (prob within RTOL, >= thr (1 - RTOL)); no duplicates; complete: every oracle
    position with p >= thr (1 + RTOL) is a record"""
    strand_ix = np.where(recs["strand"] == -1, 1, 0)
    if ds:
        assert np.all(np.isin(recs["strand"], (1, -1)))
    else:
        assert np.all(recs["strand"] == 0)
    p_or = P[strand_ix, recs["seq"], recs["motif"], recs["start"]]
    np.testing.assert_allclose(recs["prob"], p_or, rtol=RTOL, atol=1e-7)
    assert np.all(recs["prob"] >= thr * (1 - RTOL))
    keys = set(zip(recs["seq"].tolist(), recs["motif"].tolist(), recs["start"].tolist(), strand_ix.tolist()))
    assert len(keys) == recs.size
    if complete:
        for st, seq, k, pos in np.argwhere(P >= thr * (1 + RTOL)):
            assert (seq, k, pos, st) in keys, (seq, k, pos, st)


def decode_best(keys, ds):
    prob = (keys >> np.uint64(32)).astype(np.uint32).view(np.float32)
    code = (np.uint64(0xFFFFFFFF) - (keys & np.uint64(0xFFFFFFFF))).astype(np.int64)
    strand = np.where(code & 1, -1, 1) if ds else np.zeros_like(code)
    return code >> 1, strand, prob


def check_best(keys, P, ds):
    start, strand, prob = decode_best(keys, ds)
    best = P.max(axis=(0, 3))                                   # (n, K)
    np.testing.assert_allclose(prob, best, rtol=RTOL, atol=1e-7)
    n, K = best.shape
    si = np.where(strand == -1, 1, 0)
    at = P[si, np.arange(n)[:, None], np.arange(K)[None, :], start]
    np.testing.assert_allclose(at, best, rtol=RTOL, atol=1e-7)


def _run_fused(lib, cid, o, D, thr, capacity, grid=2, threads=128):
    n, L, K = D.shape[0], D.shape[3], o.num_motifs
    tables = harness.model_tables(lib.emu_sites_info, lib.emu_sites_tables, cid, o, tables_at=4)
    letters = np.zeros((n, lib.emu_sites_letter_words(L)), np.uint32)
    flags = np.zeros(4, np.uint32)
    lib.emu_sites_encode(fp(np.ascontiguousarray(D, dtype=np.float32)), fp(letters), fp(flags), n, L)
    assert flags[0] == 0
    recs = np.zeros(capacity + 4, REC)
    recs["seq"] = -7                                            # sentinel: nothing may land at or past `capacity`
    count = np.zeros(1, np.uint64)
    best = np.zeros((n, K), np.uint64)
    chunks = lib.emu_sites_run(cid, fp(tables), fp(letters), n, L, ctypes.c_float(thr), fp(recs),
                               ctypes.c_ulonglong(capacity), fp(count), fp(best), grid, threads)
    assert np.all(recs["seq"][capacity:] == -7)
    return recs, int(count[0]), best, chunks


def run_case(which):
    from oracle.crbm_oracle import synthetic_onehot
    lib = harness.load(LIB)
    if which == "select":
        # the generic models' pass: dense oracle probabilities in, the same records and keys out (both strands, one)
        for ds, pool, (n, L) in ((True, 1, (5, 150)), (False, 2, (4, 71))):
            o = harness.random_model(9, 6, ds, 11, pool=pool)
            D = synthetic_onehot(n, L, seed=4)
            P = oracle_scores(o, D).astype(np.float32)
            K, Lh = 9, L - 6 + 1
            thr = float(np.quantile(P, 0.97))
            cap = int(P.size)
            recs = np.zeros(cap, REC)
            count = np.zeros(1, np.uint64)
            best = np.zeros((n, K), np.uint64)
            p0 = np.ascontiguousarray(P[0])
            p1 = np.ascontiguousarray(P[1]) if ds else None
            lib.emu_sites_select(fp(p0), fp(p1) if ds else None, n, K, Lh, int(ds), ctypes.c_float(thr), fp(recs),
                                 ctypes.c_ulonglong(cap), fp(count), fp(best), 2, 128)
            c = int(count[0])
            assert c == int((P >= thr).sum())
            check_records(recs[:c], P.astype(np.float64), thr, ds)
            check_best(best, P.astype(np.float64), ds)
            # exact ties: equal probabilities everywhere -> the first position, + strand
            flat = np.full_like(P, 0.25)
            p0 = np.ascontiguousarray(flat[0])
            p1 = np.ascontiguousarray(flat[1]) if ds else None
            count[:] = 0
            lib.emu_sites_select(fp(p0), fp(p1) if ds else None, n, K, Lh, int(ds), ctypes.c_float(0.5), None,
                                 ctypes.c_ulonglong(0), fp(count), fp(best), 2, 128)
            start, strand, prob = decode_best(best, ds)
            assert np.all(start == 0) and np.all(strand == (1 if ds else 0)) and np.all(prob == np.float32(0.25))
            assert int(count[0]) == 0
        return
    cid, n, L = {"ds_10x15": (0, 6, 120), "ds_6x7_pool2": (1, 6, 96), "ss_10x5": (2, 6, 104),
                 "two_chunks": (3, 2, 400), "tiny_capacity": (0, 3, 90)}[which]
    K, M, DS, POOL = harness.case_info(lib.emu_sites_info, cid)[:4]
    o = harness.random_model(K, M, bool(DS), K + M, pool=POOL)
    D = synthetic_onehot(n, L, seed=K * 3 + 1)
    P = oracle_scores(o, D)
    if which == "tiny_capacity":
        recs, count, best, chunks = _run_fused(lib, cid, o, D, 0.0, 10)
        assert count == n * K * (1 + DS) * (L - M + 1)          # threshold 0: every position is a site
        assert np.all(recs["seq"][:10] >= 0)
        check_records(recs[:10], P, 0.0, bool(DS), complete=False)
        check_best(best, P, bool(DS))
        return
    thr = float(np.quantile(P, 0.9))
    cap = int(P.size)
    recs, count, best, chunks = _run_fused(lib, cid, o, D, thr, cap)
    if which == "two_chunks":
        assert chunks >= 2
    assert int((P >= thr * (1 + RTOL)).sum()) <= count <= int((P >= thr * (1 - RTOL)).sum())
    check_records(recs[:count], P, thr, bool(DS))
    check_best(best, P, bool(DS))
    # no room for records: the same count and keys
    _, count2, best2, _ = _run_fused(lib, cid, o, D, thr, 0)
    assert np.array_equal(best2, best) and count2 == count


if __name__ == "__main__":
    run_case(sys.argv[1])
    print("SITES OK", sys.argv[1])
