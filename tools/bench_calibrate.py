"""Score histogram against its floor and against the route that exists without it, in one process: config #2's
double-stranded model (10 x 15), 512 bins over [-16, 16), an N-free stream of 10^8 random letters by default.
  hist      CRBM.scoreHistogram(stream, 512), end to end, for each way a wave spreads its LDS adds (CRBM_HIST_VARIANT:
            0 motifs in order, 1 lane-rotated motif order, 2 counter sets per wave), and the device time of its kernels
            (all segments: CRBM_HIST_TIMING)
  floor     CRBM.scanSites(stream, 1.0): the same encode and gather work, next to no records
  records   what a user does without scoreHistogram: scanSites(chunk, 0.0) -> logit -> np.bincount per (motif, strand)
            over chunks of 2^20 letters, measured on 2^22 letters and scaled by letters / 2^22 (the route is linear in
            the letters: every chunk does the same work)
One warm-up of every route, then the median of 5 repeats each, the hist variants and the floor interleaved.  Writes
profiles/calibrate_bench.json (or the path given) and prints the same JSON line; the variants must agree to the bit
(asserted), and the run ends with an error when the histogram does not beat the route through records.

usage: python tools/bench_calibrate.py [letters] [output.json]
"""
import json
import os
import re
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from crbm_amd import CRBM  # noqa: E402

BINS, LO, HI = 512, -16.0, 16.0
VARIANTS = {0: "in_order", 1: "lane_rotated", 2: "per_wave_sets"}


def by_records(m, stream, chunk=1 << 20):
    """the histogram from records: every score leaves the device as a 20-byte record"""
    K, S, M = m.num_motifs, 2, m.motif_length
    counts = np.zeros(K * S * BINS, np.int64)
    for a in range(0, stream.size - M + 1, chunk):
        s = m.scanSites(stream[a:a + chunk + M - 1], 0.0)
        p = s["prob"].astype(np.float64)
        with np.errstate(divide="ignore"):
            x = np.log(p) - np.log1p(-p)
        t = (x - LO) * (BINS / (HI - LO))
        b = np.clip(np.where(t >= 0, t, 0.0), 0, BINS - 1).astype(np.int64)
        counts += np.bincount((s["motif"].astype(np.int64) * S + (s["strand"] == -1)) * BINS + b, minlength=counts.size)
    return counts.reshape(K, S, BINS)


def device_ms(fn, switch="CRBM_HIST_TIMING"):
    """kernel time the library reports on stderr under `switch` (CRBM_HIST_TIMING, or CRBM_SCAN_TIMING for scanSites)"""
    os.environ[switch] = "1"
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile() as f:
        os.dup2(f.fileno(), 2)
        try:
            fn()
        finally:
            os.dup2(saved, 2)
            os.close(saved)
            del os.environ[switch]
        f.seek(0)
        text = f.read().decode()
    return sum(float(x) for x in re.findall(r"kernels ([0-9.]+) ms", text))


def timed(fn):
    t = time.perf_counter()
    fn()
    return time.perf_counter() - t


def main():
    T = int(float(sys.argv[1])) if len(sys.argv) > 1 else 100000000
    path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "calibrate_bench.json")
    K, M = 10, 15
    stream = np.random.default_rng(1234).integers(0, 4, size=T, dtype=np.uint8)
    m = CRBM(K, M, doublestranded=True, batchsize=64, seed=1)
    m.motifs.set_value((np.random.default_rng(42).standard_normal((K, 1, 4, M)) * 0.7).astype(np.float32))
    m.bias.set_value(m.bias.get_value() + 3.0)
    default = os.environ.pop("CRBM_HIST_VARIANT", None)
    hist = lambda: m.scoreHistogram(stream, bins=BINS, lo=LO, hi=HI)
    small = stream[:min(T, 1 << 22)]
    ref = None
    for v in VARIANTS:                                   # warm-up, and the variants must agree to the bit
        os.environ["CRBM_HIST_VARIANT"] = str(v)
        h = hist()
        assert ref is None or np.array_equal(ref.counts, h.counts)
        ref = h
    m.scanSites(stream, 1.0)
    rec = by_records(m, small)
    os.environ["CRBM_HIST_VARIANT"] = "1"
    hs = m.scoreHistogram(small, bins=BINS, lo=LO, hi=HI)
    moved = int(np.abs(rec - hs.counts).sum()) // 2      # scores the logit of the rounded prob puts in a neighbouring bin
    th = {v: [] for v in VARIANTS}
    tf, tr = [], []
    for _ in range(5):
        for v in VARIANTS:
            os.environ["CRBM_HIST_VARIANT"] = str(v)
            th[v].append(timed(hist))
        tf.append(timed(lambda: m.scanSites(stream, 1.0)))
        tr.append(timed(lambda: by_records(m, small)))
    out = {"letters": T, "K": K, "M": M, "ds": True, "bins": BINS, "lo": LO, "hi": HI, "windows": ref.windows,
           "rows_sum_to_windows": bool(np.all(ref.counts.sum(axis=2) == ref.windows)),
           "floor_scan_thr1_ms": [round(x * 1e3, 2) for x in tf], "floor_median_ms": statistics.median(tf) * 1e3,
           "records_letters": int(small.size), "records_ms": [round(x * 1e3, 2) for x in tr],
           "records_scaled_median_ms": statistics.median(tr) * 1e3 * T / small.size,
           "records_rows_sum_equal": bool(np.array_equal(rec.sum(axis=2), hs.counts.sum(axis=2))), "records_scores_in_a_neighbouring_bin": moved}
    for v, name in VARIANTS.items():
        os.environ["CRBM_HIST_VARIANT"] = str(v)
        out["hist_%s_ms" % name] = [round(x * 1e3, 2) for x in th[v]]
        out["hist_%s_median_ms" % name] = statistics.median(th[v]) * 1e3
        out["hist_%s_kernels_device_ms" % name] = device_ms(hist)
        out["hist_%s_over_floor" % name] = out["hist_%s_median_ms" % name] / out["floor_median_ms"]
    os.environ.pop("CRBM_HIST_VARIANT")
    if default is not None:
        os.environ["CRBM_HIST_VARIANT"] = default
    out["floor_kernels_device_ms"] = device_ms(lambda: m.scanSites(stream, 1.0), "CRBM_SCAN_TIMING")
    best = min(VARIANTS, key=lambda v: out["hist_%s_median_ms" % VARIANTS[v]])
    out["fastest_variant"] = VARIANTS[best]
    out["hist_beats_records"] = out["hist_%s_median_ms" % VARIANTS[best]] < out["records_scaled_median_ms"]
    line = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write(line + "\n")
    print(line)
    if not out["hist_beats_records"]:                    # the required outcome
        sys.exit("scoreHistogram (%.1f ms) does not beat the route through records (%.1f ms scaled)"
                 % (out["hist_%s_median_ms" % VARIANTS[best]], out["records_scaled_median_ms"]))


if __name__ == "__main__":
    main()
