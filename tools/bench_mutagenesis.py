"""In-silico mutagenesis at data-set scale: config #2's model (10 x 15, double-stranded) over 10^5 x 200 bp resident
codes by default.
  (a) crbm_mutagenesis_resident with dF (the dense (n,L,4) array copied to the host),
  (b) pll only,
  (c) the way without this kernel: the 600 substituted copies of a chunk of rows built on the host and sent through
      crbm_free_energy_codes, extrapolated to n rows from enough chunks to run >= 0.5 s,
  (d) the library's own general path (CRBM_MUT_FUSED=0) on a share of the rows, extrapolated, for information.
Warm-up call, then `reps` windows of at least 0.25 s of back-to-back calls: minimum and median of the per-call time
over the windows.  One JSON line.

usage: python tools/bench_mutagenesis.py [n_sequences] [L] [K] [M] [ds] [reps]
"""
import ctypes
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from crbm_amd import CRBM  # noqa: E402
from crbm_amd._lib import fptr  # noqa: E402


def timed(fn, reps, window=0.25):
    """per-call time: a warm-up call (buffers allocated, tables built, clocks up), then `reps` windows of back-to-back
    calls, each window at least `window` seconds long (a single call of ~10 ms is too short to time on its own)"""
    fn()
    ts, calls = [], 0
    for _ in range(reps):
        t, k = time.perf_counter(), 0
        while k == 0 or time.perf_counter() - t < window:
            fn()
            k += 1
        ts.append((time.perf_counter() - t) / k)
        calls += k
    return {"min_s": min(ts), "median_s": float(np.median(ts)), "reps": reps, "calls": calls}


def host_copies(codes):
    """the 3 L single-substitution copies of every row, (n * 3 L, L) uint8"""
    n, L = codes.shape
    out = np.repeat(codes[:, None, :], 3 * L, axis=1)
    p = np.repeat(np.arange(L), 3)
    x = np.tile(np.arange(1, 4), L)
    out[:, np.arange(3 * L), p] = (codes[:, p] + x[None, :]) & 3
    return out.reshape(n * 3 * L, L)


def main():
    arg = lambda i, d: int(sys.argv[i]) if len(sys.argv) > i else d
    n, L, K, M, ds, reps = arg(1, 100000), arg(2, 200), arg(3, 10), arg(4, 15), bool(arg(5, 1)), arg(6, 5)
    codes = np.random.default_rng(1234).integers(0, 4, size=(n, L), dtype=np.uint8)
    m = CRBM(K, M, doublestranded=ds, batchsize=64, seed=1)
    m.motifs.set_value((np.random.default_rng(42).standard_normal((K, 1, 4, M)) * 0.7).astype(np.float32))
    m.bias.set_value(m.bias.get_value() + 3.0)
    m._upload(codes, 0)
    out = {"n": n, "L": L, "K": K, "M": M, "ds": ds}
    dfe = np.empty((n, L, 4), np.float32)
    pll = np.empty(n, np.float32)
    out["a_fused_dF"] = timed(lambda: m._call("crbm_mutagenesis_resident", 0, n, fptr(dfe), fptr(pll)), reps)
    out["b_fused_pll_only"] = timed(lambda: m._call("crbm_mutagenesis_resident", 0, n, None, fptr(pll)), reps)
    out["mean_pll_per_base"] = float(pll.mean() / L)
    # (c) the parent's way on chunks of 256 rows; as many chunks as run >= 0.5 s, the copies built inside the timing
    chunk = min(256, n)
    fe = np.empty(chunk * 3 * L, np.float32)
    fe0 = np.empty(chunk, np.float32)
    u8 = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))

    def parent_way(rows):
        muts = host_copies(rows)
        m._call("crbm_free_energy_codes", u8(muts), muts.shape[0], L, fptr(fe), None)
        m._call("crbm_free_energy_codes", u8(rows), rows.shape[0], L, fptr(fe0), None)
        return (fe.reshape(rows.shape[0], L, 3) - fe0[:, None, None]) * L

    parent_way(codes[:chunk])                        # warm-up
    per_chunk = []
    for rep in range(reps):
        t0, done = time.perf_counter(), 0
        while time.perf_counter() - t0 < 0.5 and (done + 1) * chunk <= n:
            parent_way(codes[done * chunk:(done + 1) * chunk])
            done += 1
        per_chunk.append((time.perf_counter() - t0) / done)
    c = {"min_s": min(per_chunk) * n / chunk, "median_s": float(np.median(per_chunk)) * n / chunk, "reps": reps,
         "chunk_rows": chunk, "extrapolated": True}
    # without the host's work (copies built once, outside the timing; the upload of the copies stays inside)
    muts = host_copies(codes[:chunk])
    dev = timed(lambda: m._call("crbm_free_energy_codes", u8(muts), muts.shape[0], L, fptr(fe), None), reps)
    c["without_host_build_min_s"] = dev["min_s"] * n / chunk
    c["without_host_build_median_s"] = dev["median_s"] * n / chunk
    out["c_host_copies_free_energy"] = c
    # (d) the general path on n/50 rows
    nd = max(1, n // 50)
    os.environ["CRBM_MUT_FUSED"] = "0"
    d = timed(lambda: m._call("crbm_mutagenesis_resident", 0, nd, fptr(dfe[:nd]), fptr(pll[:nd])), reps)
    del os.environ["CRBM_MUT_FUSED"]
    out["d_general_path"] = {"min_s": d["min_s"] * n / nd, "median_s": d["median_s"] * n / nd, "reps": reps, "rows": nd,
                             "extrapolated": True}
    out["a_over_c"] = out["a_fused_dF"]["median_s"] / c["median_s"]
    out["a_over_c_without_host_build"] = out["a_fused_dF"]["median_s"] / c["without_host_build_median_s"]
    out["b_over_c"] = out["b_fused_pll_only"]["median_s"] / c["median_s"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
