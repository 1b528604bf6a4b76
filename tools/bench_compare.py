"""compareMotifs against the only other route to the same numbers, in one process: K = 300 queries of width 10 against
N = 10^4 synthetic targets (Dirichlet(0.3) columns, widths 6 .. 20), both strands, 100 bins.
  device     compareMotifs end to end (median of 5: quantisation, the C call with its copies, the result object) and the
             device time the library reports (crbm_compare_ms), in total and for the three stages: counts, null,
             placements; and the host time of deriving p-, E- and q-values from the result, which neither side of the
             comparison below includes
  numpy      tests/compare_reference.py in the same process on a stated subset -- the nulls of `ref_queries` queries
             against the whole pool, and the placements of those queries on the first `ref_targets` targets -- whose
             results must have the device's bits.  Its time for the whole problem is EXTRAPOLATED from the subset:
             null time per query * K + placement time per pair * K * N.  The tool fails when the device route is not
             faster than that.
Writes profiles/compare_bench.json and prints the same JSON line.

usage: python tools/bench_compare.py [K] [N]
"""
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from crbm_amd import CRBM, MotifSet, compareMotifs  # noqa: E402
from crbm_amd import motifs  # noqa: E402
from tests import compare_reference as R  # noqa: E402

WIDTH, BINS, REF_QUERIES, REF_TARGETS = 10, 100, 2, 200


def timed(fn, repeats=5):
    ts, out = [], None
    for _ in range(repeats):
        t = time.perf_counter()
        out = fn()
        ts.append((time.perf_counter() - t) * 1e3)
    return out, [round(x, 2) for x in ts], statistics.median(ts)


def main():
    K = int(sys.argv[1]) if len(sys.argv) > 1 else 300
    N = int(sys.argv[2]) if len(sys.argv) > 2 else 10000
    rng = np.random.default_rng(7)
    queries = MotifSet(["q%d" % i for i in range(K)], [R.dirichlet_motif(rng, WIDTH) for _ in range(K)])
    targets = MotifSet(["t%d" % i for i in range(N)], [R.dirichlet_motif(rng, int(w)) for w in rng.integers(6, 21, size=N)])
    m = CRBM(10, 15, doublestranded=True, batchsize=8, seed=1)   # any model: it lends its device
    out = {"K": K, "N": N, "query_width": WIDTH, "target_widths": "6..20", "bins": BINS, "strands": "both",
           "pool_columns": int(2 * targets.widths.sum()), "column_pairs": int(2 * K * WIDTH * targets.widths.sum())}
    compareMotifs(m, queries, targets, bins=BINS)                # warm-up
    c, out["device_ms"], out["device_median_ms"] = timed(lambda: compareMotifs(m, queries, targets, bins=BINS))
    total, stages = motifs.last_device_ms(m)
    t = time.perf_counter()
    c.qvalue                                                     # p-, E- and q-values are derived on the host when first read
    out["derive_host_ms"] = (time.perf_counter() - t) * 1e3
    out["kernels_device_ms"] = total
    out["counts_device_ms"], out["null_device_ms"], out["placements_device_ms"] = stages
    out["column_pairs_per_second_placements"] = out["column_pairs"] / (stages[2] * 1e-3)

    nq, nt = min(REF_QUERIES, K), min(REF_TARGETS, N)
    qq = [R.quantise(mat) for mat in queries.matrices[:nq]]
    tq = [R.quantise(mat) for mat in targets.matrices]
    t0 = time.perf_counter()
    pool = R.pool_of(tq, True)
    tails = [R.tails_of(R.counts_of(q, pool, BINS), 1.0 / len(pool)) for q in qq]
    t1 = time.perf_counter()
    for k, q in enumerate(qq):
        for t in range(nt):
            p, o, s, l, n_off = R.pair(q, tq[t], tails[k], BINS, True, 1)
            assert np.float64(p).view(np.uint64) == c.p_min[k, t].view(np.uint64) and (o, s, l, n_off) == \
                (c.offset[k, t], c.strand[k, t], c.overlap[k, t], c.n_off[k, t]), "the device and the reference differ at %d, %d" % (k, t)
    t2 = time.perf_counter()
    out["numpy_subset"] = {"ref_queries": nq, "ref_targets": nt, "null_ms": (t1 - t0) * 1e3, "placements_ms": (t2 - t1) * 1e3}
    out["numpy_extrapolated_ms"] = (t1 - t0) * 1e3 / nq * K + (t2 - t1) * 1e3 / (nq * nt) * K * N
    out["numpy_is_extrapolated"] = True
    out["numpy_over_device"] = out["numpy_extrapolated_ms"] / out["device_median_ms"]
    out["device_faster_than_numpy"] = out["device_median_ms"] < out["numpy_extrapolated_ms"]
    out["matches_evalue_10"] = int(len(c.matches(evalue=10.0)))

    line = json.dumps(out)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "compare_bench.json"), "w") as f:
        f.write(line + "\n")
    print(line)
    if not out["device_faster_than_numpy"]:
        sys.exit("compareMotifs is not faster than the NumPy reference")


if __name__ == "__main__":
    main()
