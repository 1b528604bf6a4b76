"""Motif-site sweep at data-set scale: crbm_motif_sites_resident (thresholded records + best sites, best sites only)
beside crbm_hit_summary_resident on the same resident data set -- config #2's model (10 x 15, double-stranded) over
10^6 x 200 bp random codes by default, at a threshold that yields about one site per (sequence, motif).

usage: python tools/bench_sites.py [n_sequences] [L] [K] [M] [ds]
"""
import ctypes
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from crbm_amd import CRBM, _lib  # noqa: E402
from crbm_amd._lib import fptr  # noqa: E402
from crbm_amd.crbm import _RAW_SITE  # noqa: E402


def timed(fn, reps=3):
    fn()
    best = 1e30
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        best = min(best, time.perf_counter() - t)
    return best


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 1000000
    L = int(sys.argv[2]) if len(sys.argv) > 2 else 200
    K = int(sys.argv[3]) if len(sys.argv) > 3 else 10
    M = int(sys.argv[4]) if len(sys.argv) > 4 else 15
    ds = bool(int(sys.argv[5])) if len(sys.argv) > 5 else True
    rng = np.random.default_rng(1234)
    codes = rng.integers(0, 4, size=(n, L), dtype=np.uint8)
    m = CRBM(K, M, doublestranded=ds, batchsize=64, seed=1)
    m.motifs.set_value((np.random.default_rng(42).standard_normal((K, 1, 4, M)) * 0.7).astype(np.float32))
    m.bias.set_value(m.bias.get_value() + 3.0)
    Lh, S = L - M + 1, 2 if ds else 1
    # the threshold of ~1 site per (sequence, motif): the 1 - 1/(S*Lh) quantile of the scores of 2000 rows
    sample = np.eye(4, dtype=np.float32)[codes[:2000]].transpose(0, 2, 1)[:, None]
    P = [m.motifHitProbs(sample)] + ([m._bottomUpProbabilityOfData(sample, flip_motif=True)] if ds else [])
    thr = float(np.quantile(np.stack(P), 1.0 - 1.0 / (S * Lh)))
    out = {"n": n, "L": L, "K": K, "M": M, "ds": ds, "threshold": thr}
    out["upload_s"] = timed(lambda: m._upload(codes, 0), reps=1)
    cap = 4 * n * K
    raw = np.empty(cap, _RAW_SITE)
    count = ctypes.c_int64(0)
    i32 = ctypes.POINTER(ctypes.c_int32)
    bs, bt, bp = np.empty((n, K), np.int32), np.empty((n, K), np.int32), np.empty((n, K), np.float32)
    recp = raw.ctypes.data_as(ctypes.POINTER(_lib.CrbmSite))
    out["sites_and_best_s"] = timed(lambda: m._call("crbm_motif_sites_resident", 0, n, thr, cap, recp, ctypes.byref(count),
                                                    bs.ctypes.data_as(i32), bt.ctypes.data_as(i32), fptr(bp)))
    out["records"] = count.value
    out["records_per_seq_motif"] = count.value / (n * K)
    out["best_only_s"] = timed(lambda: m._call("crbm_motif_sites_resident", 0, n, thr, 0, None, None,
                                               bs.ctypes.data_as(i32), bt.ctypes.data_as(i32), fptr(bp)))
    mx, mean = np.empty((n, K), np.float32), np.empty((n, K), np.float32)
    pos = np.empty((K, Lh), np.float32)
    out["hit_summary_s"] = timed(lambda: m._call("crbm_hit_summary_resident", 0, n, fptr(mx), fptr(mean), fptr(pos)))
    for k in ("sites_and_best_s", "best_only_s", "hit_summary_s"):
        out[k[:-2] + "_ms"] = out[k] * 1e3
        out[k[:-2] + "_seq_per_s"] = n / out[k]
    out["sites_over_summary"] = out["sites_and_best_s"] / out["hit_summary_s"]
    out["best_only_over_summary"] = out["best_only_s"] / out["hit_summary_s"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
