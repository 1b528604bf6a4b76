"""Stream scan against the route that exists without it, end to end, in one process: config #2's double-stranded model
(10 x 15) at threshold 0.9 over an N-free stream of 10^8 random letters by default.
  scan      CRBM.scanSites(stream, thr)
  windowed  cut the stream on the host into rows of 200 letters that overlap by M - 1, CRBM.motifSites on the rows,
            map the records back to stream positions and drop the duplicates of the overlaps
One warm-up, then the median of 5 repeats of each route, interleaved; the two record sets must be equal (motif, start,
strand, prob bit for bit).  The scan's device time (all kernels of all segments: CRBM_SCAN_TIMING) comes from a
sixth scan.  Writes profiles/scan_bench.json and prints the same JSON line.

usage: python tools/bench_scan.py [letters] [threshold]
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

L = 200


def windowed(m, stream, thr):
    """the route without scanSites: rows of L letters overlapping by M - 1 -> motifSites -> stream positions"""
    M = m.motif_length
    step = L - M + 1                                    # window starts per row: every start belongs to exactly one row
    T = stream.size
    n = (T - M + 1 + step - 1) // step
    starts = np.arange(n, dtype=np.int64) * step
    starts[-1] = T - L                                  # the last row is moved back to end with the stream ...
    rows = np.lib.stride_tricks.as_strided(stream, shape=(n - 1, L), strides=(step, 1))
    rows = np.concatenate([rows, stream[None, T - L:]])
    s = m.motifSites(np.ascontiguousarray(rows), thr)
    pos = starts[s["seq"]] + s["start"]
    keep = np.ones(s.size, bool)
    if n > 1:
        keep[(s["seq"] == n - 1) & (pos < starts[-2] + step)] = False    # ... and its overlap with the row before dropped
    s, pos = s[keep], pos[keep]
    order = np.lexsort((np.where(s["strand"] == -1, 1, 0), s["motif"], pos))
    out = s[order]
    out["seq"] = 0
    out["start"] = pos[order]
    return out


def device_ms(fn):
    """kernel time the library reports on stderr under CRBM_SCAN_TIMING"""
    os.environ["CRBM_SCAN_TIMING"] = "1"
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile() as f:
        os.dup2(f.fileno(), 2)
        try:
            fn()
        finally:
            os.dup2(saved, 2)
            os.close(saved)
            del os.environ["CRBM_SCAN_TIMING"]
        f.seek(0)
        text = f.read().decode()
    return sum(float(x) for x in re.findall(r"kernels ([0-9.]+) ms", text))


def main():
    T = int(float(sys.argv[1])) if len(sys.argv) > 1 else 100000000
    thr = float(sys.argv[2]) if len(sys.argv) > 2 else 0.9
    K, M = 10, 15
    stream = np.random.default_rng(1234).integers(0, 4, size=T, dtype=np.uint8)
    m = CRBM(K, M, doublestranded=True, batchsize=64, seed=1)
    m.motifs.set_value((np.random.default_rng(42).standard_normal((K, 1, 4, M)) * 0.7).astype(np.float32))
    m.bias.set_value(m.bias.get_value() + 3.0)
    a = m.scanSites(stream, thr)                        # warm-up of both routes, and the check that they agree
    b = windowed(m, stream, thr)
    same = a.size == b.size and all(np.array_equal(a[f], b[f]) for f in ("motif", "start", "strand")) and \
        np.array_equal(a["prob"].view(np.uint32), b["prob"].view(np.uint32))
    ts, tw = [], []
    for _ in range(5):
        t = time.perf_counter()
        m.scanSites(stream, thr)
        ts.append(time.perf_counter() - t)
        t = time.perf_counter()
        windowed(m, stream, thr)
        tw.append(time.perf_counter() - t)
    out = {"letters": T, "K": K, "M": M, "ds": True, "threshold": thr, "records": int(a.size), "routes_agree": bool(same),
           "scan_ms": [round(x * 1e3, 2) for x in ts], "windowed_ms": [round(x * 1e3, 2) for x in tw],
           "scan_median_ms": statistics.median(ts) * 1e3, "windowed_median_ms": statistics.median(tw) * 1e3}
    out["scan_over_windowed"] = out["scan_median_ms"] / out["windowed_median_ms"]
    out["scan_kernels_device_ms"] = device_ms(lambda: m.scanSites(stream, thr))
    out["scan_not_slower"] = out["scan_median_ms"] <= out["windowed_median_ms"]
    line = json.dumps(out)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "scan_bench.json"), "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
