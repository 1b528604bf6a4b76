"""The analytic null against the other routes to a score distribution, in one process, on config #2's double-stranded
model (10 x 15), a Markov background of order 3 and step 2^-10.
  device     scoreDistribution(model, background) end to end (median of 5) and the device time the library reports
             (crbm_null_ms), for both kernel variants (CRBM_NULL_VARIANT = 0 plain gather, 1 sibling tiles through the LDS);
             both give the same bits, which the tool asserts
  numpy      the dynamic programme of tests/null_reference.py on the same inputs: the only other route to the same result.
             The tool fails when the device route is not faster.
  sampled    the empirical route, for context: sampleBackground + scoreHistogram over 10^8 letters by default, its time,
             and the largest standardised difference (count - n p) / sqrt(n p (1 - p)) between its counts and binned()
             over the bins with at least 100 expected counts.  A recorded number, no pass / fail: overlapping windows are
             not independent.
Writes profiles/null_bench.json and prints the same JSON line.

usage: python tools/bench_null.py [letters]
"""
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from crbm_amd import CRBM, fitBackground, sampleBackground, scoreDistribution  # noqa: E402
from crbm_amd import null  # noqa: E402
from tests import null_reference as R  # noqa: E402
from tests import background_reference as B  # noqa: E402

STEP, ORDER, BINS, LO, HI = 2.0 ** -10, 3, 512, -16.0, 16.0


def timed(fn, repeats=5):
    ts, out = [], None
    for _ in range(repeats):
        t = time.perf_counter()
        out = fn()
        ts.append((time.perf_counter() - t) * 1e3)
    return out, [round(x, 2) for x in ts], statistics.median(ts)


def model():
    K, M = 10, 15
    m = CRBM(K, M, doublestranded=True, batchsize=64, seed=1)
    m.motifs.set_value((np.random.default_rng(42).standard_normal((K, 1, 4, M)) * 0.7).astype(np.float32))
    m.bias.set_value(m.bias.get_value() + 3.0)
    return m


def main():
    T = int(float(sys.argv[1])) if len(sys.argv) > 1 else 100000000
    m = model()
    data = sampleBackground(m, min(T, 10000000), B.dirichlet_table(ORDER, 41), 3)     # sequence with third-order structure
    bg = fitBackground(m, data, order=ORDER)
    out = {"K": 10, "M": 15, "ds": True, "order": ORDER, "step": STEP, "letters": T}
    dists = {}
    for variant in (0, 1):
        os.environ["CRBM_NULL_VARIANT"] = str(variant)
        scoreDistribution(m, bg, step=STEP)                      # warm-up
        dists[variant], out["device_v%d_ms" % variant], out["device_v%d_median_ms" % variant] = timed(lambda: scoreDistribution(m, bg, step=STEP))
        out["device_v%d_kernels_device_ms" % variant] = null.last_device_ms(m)
    del os.environ["CRBM_NULL_VARIANT"]
    d = dists[0]
    assert np.array_equal(d.pmf, dists[1].pmf), "the kernel variants differ"
    out["G"] = int(d.G)
    out["cells"] = int(20 * R.contexts(ORDER) * d.G * 15)

    w, c = null.window_pwm(m)
    q, _, _, _ = null.quantise(w, c, STEP)
    P = bg.probabilities(1.0)
    init = null.stationary(P, ORDER)
    t = time.perf_counter()
    want = [R.dp(q[r], P, init, ORDER) for r in range(q.shape[0])]
    out["numpy_dp_ms"] = (time.perf_counter() - t) * 1e3
    bound = (8 * 15 + 128) * 2.0 ** -53
    worst = 0.0
    for r, ref in enumerate(want):
        got = d.pmf.reshape(q.shape[0], -1)[r, :ref.size]
        big = ref > 1e-280
        worst = max(worst, float((np.abs(got[big] - ref[big]) / ref[big]).max()) / bound)
    out["worst_relative_error_over_bound"] = worst
    best = min(out["device_v0_median_ms"], out["device_v1_median_ms"])
    out["numpy_over_device"] = out["numpy_dp_ms"] / best
    out["device_faster_than_numpy"] = best < out["numpy_dp_ms"]

    def sampled():
        return m.scoreHistogram(sampleBackground(m, T, bg, 7), bins=BINS, lo=LO, hi=HI)
    sampled()
    h, out["sampled_ms"], out["sampled_median_ms"] = timed(sampled, repeats=3)
    expect = d.binned(BINS, LO, HI) * h.windows
    ok = expect >= 100.0
    p = expect / h.windows
    z = (h.counts - expect)[ok] / np.sqrt((expect * (1.0 - p))[ok])
    out["windows"] = int(h.windows)
    out["bins_compared"] = int(ok.sum())
    out["largest_standardised_difference"] = float(np.abs(z).max())
    _, resolved = d.thresholds(1e-8)
    out["smallest_positive_tail"] = float(d.tail()[d.tail() > 0].min())
    out["thresholds_fpr_1e-8_resolved_in_float32"] = "%d of %d" % (int(resolved.sum()), resolved.size)

    line = json.dumps(out)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "null_bench.json"), "w") as f:
        f.write(line + "\n")
    print(line)
    if not out["device_faster_than_numpy"]:
        sys.exit("scoreDistribution is not faster than the NumPy dynamic programme")


if __name__ == "__main__":
    main()
