"""Markov backgrounds against the null they replace, end to end, in one process: a stream of 10^8 letters by default,
1 % of it in gap runs of 500, on the device of config #2's double-stranded model (10 x 15).
  fit        fitBackground(model, stream, order=3)
  sample     sampleBackground(model, stream, background, seed) at orders 1 and 3
  shuffle    sequences.shuffleStream(stream, seed): the host's lexsort over all letters
  consumer   model.scoreHistogram(sampled stream)
One warm-up of the device routes, then the median of 5 repeats of each; the device time is what the library reports
for the kernels of the last call (crbm_background_ms; CRBM_HIST_TIMING for the consumer).  The tool fails when
sampleBackground at order 3 is not faster than shuffleStream end to end.  Writes profiles/background_bench.json and
prints the same JSON line.

  --scan     instead: sampleBackground at order 3 for chunk lengths 64 .. 4096 (CRBM_BG_CHUNK), median of 3 each, into
             profiles/background_chunk_scan.json -- what the default of crbm_background.h was chosen from.

usage: python tools/bench_background.py [--scan] [letters]
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
from crbm_amd import CRBM, fitBackground, sampleBackground, shuffleStream  # noqa: E402
from crbm_amd.background import last_device_ms  # noqa: E402

SCAN_CHUNKS = (64, 128, 256, 512, 1024, 2048, 4096)


def gapped(T, seed=1234, share=0.01, run=500):
    rng = np.random.default_rng(seed)
    s = rng.integers(0, 4, size=T, dtype=np.uint8)
    for at in rng.integers(0, max(T - run, 1), size=max(1, int(T * share / run))):
        s[at:at + run] = 4
    return s


def timed(fn, repeats=5):
    ts, out = [], None
    for _ in range(repeats):
        t = time.perf_counter()
        out = fn()
        ts.append((time.perf_counter() - t) * 1e3)
    return out, [round(x, 2) for x in ts], statistics.median(ts)


def hist_device_ms(fn):
    """kernel time the library reports on stderr under CRBM_HIST_TIMING"""
    os.environ["CRBM_HIST_TIMING"] = "1"
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile() as f:
        os.dup2(f.fileno(), 2)
        try:
            fn()
        finally:
            os.dup2(saved, 2)
            os.close(saved)
            del os.environ["CRBM_HIST_TIMING"]
        f.seek(0)
        text = f.read().decode()
    return sum(float(x) for x in re.findall(r"kernels ([0-9.]+) ms", text))


def write(name, out):
    line = json.dumps(out)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", name), "w") as f:
        f.write(line + "\n")
    print(line)


def model():
    K, M = 10, 15
    m = CRBM(K, M, doublestranded=True, batchsize=64, seed=1)
    m.motifs.set_value((np.random.default_rng(42).standard_normal((K, 1, 4, M)) * 0.7).astype(np.float32))
    m.bias.set_value(m.bias.get_value() + 3.0)
    return m


def scan(T):
    m = model()
    stream = gapped(T)
    bg = fitBackground(m, stream, order=3)
    rows, first = [], None
    for chunk in SCAN_CHUNKS:
        os.environ["CRBM_BG_CHUNK"] = str(chunk)
        got = sampleBackground(m, stream, bg, 7)                 # warm-up, and: the chunk length changes no bit
        first = got if first is None else first
        assert np.array_equal(got, first)
        _, ts, med = timed(lambda: sampleBackground(m, stream, bg, 7), repeats=3)
        rows.append({"chunk": chunk, "end_to_end_ms": ts, "end_to_end_median_ms": med, "kernels_device_ms": last_device_ms(m)})
    del os.environ["CRBM_BG_CHUNK"]
    best = min(rows, key=lambda r: r["kernels_device_ms"])
    copies = min(r["end_to_end_median_ms"] - r["kernels_device_ms"] for r in rows)
    write("background_chunk_scan.json", {
        "letters": T, "order": 3, "rows": rows, "fastest_kernels_chunk": best["chunk"],
        "end_to_end_minus_kernels_ms": copies,
        "bound": "the copies of T bytes up and down (and the host's checks)" if copies > best["kernels_device_ms"] else "the kernels"})


def main():
    args = [a for a in sys.argv[1:] if a != "--scan"]
    T = int(float(args[0])) if args else 100000000
    if "--scan" in sys.argv[1:]:
        return scan(T)
    m = model()
    stream = gapped(T)
    bg3 = fitBackground(m, stream, order=3)                      # warm-up of the device routes
    bg1 = fitBackground(m, stream, order=1)
    sampleBackground(m, stream, bg3, 7)
    out = {"letters": T, "gap_share": float((stream == 4).mean()), "K": 10, "M": 15, "ds": True}
    _, out["fit_order3_ms"], out["fit_order3_median_ms"] = timed(lambda: fitBackground(m, stream, order=3))
    out["fit_order3_kernels_device_ms"] = last_device_ms(m)
    for order, bg in ((1, bg1), (3, bg3)):
        null, out["sample_order%d_ms" % order], out["sample_order%d_median_ms" % order] = timed(lambda: sampleBackground(m, stream, bg, 7))
        out["sample_order%d_kernels_device_ms" % order] = last_device_ms(m)
    assert np.array_equal(null == 4, stream == 4)
    _, out["shuffle_ms"], out["shuffle_median_ms"] = timed(lambda: shuffleStream(stream, 7))
    m.scoreHistogram(null)
    _, out["histogram_ms"], out["histogram_median_ms"] = timed(lambda: m.scoreHistogram(null))
    out["histogram_kernels_device_ms"] = hist_device_ms(lambda: m.scoreHistogram(null))
    out["shuffle_over_sample_order3"] = out["shuffle_median_ms"] / out["sample_order3_median_ms"]
    out["sample_faster_than_shuffle"] = out["sample_order3_median_ms"] < out["shuffle_median_ms"]
    write("background_bench.json", out)
    if not out["sample_faster_than_shuffle"]:
        sys.exit("sampleBackground is not faster than shuffleStream end to end")


if __name__ == "__main__":
    main()
