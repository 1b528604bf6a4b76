"""Variant effects against the route that exists without them, end to end, in one process: config #2's double-stranded
model (10 x 15), a stream of 10^7 letters with 1 % of them inside gap runs, 10^6 random variants by default.
  variants     CRBM.variantEffects(stream, pos, alt)["dfe"]
  mutagenesis  cut the context of 2M - 1 letters around every variant on the host, CRBM.mutagenesis on the (V, 2M - 1)
               rows, pick entry [M - 1, alt] -- possible only where the whole context holds letters; the variants it
               cannot serve (a gap or a stream end within M - 1 letters) are counted
One warm-up, then the median of 5 repeats of each route, interleaved; the largest difference between the two on the
variants the old route serves is reported against the project's criterion RTOL |want| + RTOL max|want|, RTOL = 1e-4.
The kernels' device time (all kernels of all chunks: CRBM_VARIANT_TIMING) comes from a sixth call.  Writes
profiles/variants_bench.json and prints the same JSON line; exits with status 1 if the new call is not faster.

usage: python tools/bench_variants.py [letters] [variants]
"""
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from crbm_amd import CRBM  # noqa: E402
from tools.bench_calibrate import device_ms  # noqa: E402

RTOL = 1e-4


def gapped_stream(T, seed, share=0.01, run=500):
    rng = np.random.default_rng(seed)
    s = rng.integers(0, 4, size=T, dtype=np.uint8)
    for a in rng.integers(0, T - run, size=max(1, int(T * share / run))):
        s[a:a + run] = 4
    return s


def by_mutagenesis(m, stream, pos, alt):
    """the route without variantEffects: (dfe of the variants it serves, their indices)"""
    M = m.motif_length
    idx = pos[:, None] + np.arange(-(M - 1), M)[None, :]
    inside = (idx[:, 0] >= 0) & (idx[:, -1] < stream.size)
    ctx = np.full(idx.shape, 4, np.uint8)
    ctx[inside] = stream[idx[inside]]
    served = np.flatnonzero((ctx < 4).all(axis=1))
    d = m.mutagenesis(np.ascontiguousarray(ctx[served]))
    return d[np.arange(served.size), M - 1, alt[served]], served


def main():
    T = int(float(sys.argv[1])) if len(sys.argv) > 1 else 10000000
    V = int(float(sys.argv[2])) if len(sys.argv) > 2 else 1000000
    K, M = 10, 15
    stream = gapped_stream(T, 1234)
    rng = np.random.default_rng(99)
    pos, alt = rng.integers(0, T, size=V), rng.integers(0, 4, size=V).astype(np.uint8)
    m = CRBM(K, M, doublestranded=True, batchsize=64, seed=1)
    m.motifs.set_value((np.random.default_rng(42).standard_normal((K, 1, 4, M)) * 0.7).astype(np.float32))
    m.bias.set_value(m.bias.get_value() + 3.0)
    new = m.variantEffects(stream, pos, alt)            # warm-up of both routes, and their agreement
    old, served = by_mutagenesis(m, stream, pos, alt)
    want = old.astype(np.float64)
    err = np.abs(new["dfe"][served].astype(np.float64) - want)
    bound = RTOL * np.abs(want) + RTOL * np.abs(want).max()
    tn, to = [], []
    for _ in range(5):
        t = time.perf_counter()
        m.variantEffects(stream, pos, alt)
        tn.append(time.perf_counter() - t)
        t = time.perf_counter()
        by_mutagenesis(m, stream, pos, alt)
        to.append(time.perf_counter() - t)
    out = {"letters": T, "variants": V, "K": K, "M": M, "ds": True, "gap_share": float((stream > 3).mean()),
           "not_served_by_mutagenesis": int(V - served.size), "on_no_letter": int((stream[pos] > 3).sum()),
           "max_abs_difference": float(err.max()), "max_abs_dfe": float(np.abs(want).max()),
           "worst_difference_over_bound": float((err / bound).max()), "routes_agree": bool(np.all(err <= bound)),
           "variants_ms": [round(x * 1e3, 2) for x in tn], "mutagenesis_ms": [round(x * 1e3, 2) for x in to],
           "variants_median_ms": statistics.median(tn) * 1e3, "mutagenesis_median_ms": statistics.median(to) * 1e3}
    out["variants_over_mutagenesis"] = out["variants_median_ms"] / out["mutagenesis_median_ms"]
    out["variants_kernels_device_ms"] = device_ms(lambda: m.variantEffects(stream, pos, alt), "CRBM_VARIANT_TIMING")
    out["variants_faster"] = out["variants_median_ms"] < out["mutagenesis_median_ms"]
    line = json.dumps(out)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "variants_bench.json"), "w") as f:
        f.write(line + "\n")
    print(line)
    return 0 if out["variants_faster"] and out["routes_agree"] else 1


if __name__ == "__main__":
    sys.exit(main())
