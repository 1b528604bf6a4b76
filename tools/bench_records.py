"""Record summaries against what exists without them, in one process: config #2's double-stranded model (10 x 15) on
two streams of 10^8 letters (by default) with 1 % of them in gap runs of 25 codes.
  (a) many    5 * 10^5 records of 100..300 letters (scaled with the letters): CRBM.recordSummary(stream, offsets) end to
              end and the device time of its kernels (CRBM_RECORDS_TIMING), against the host route: the N-free records
              grouped by length -> freeEnergy(codes, permotif=True) + motifBestSites(codes) per group.  The route cannot
              serve a record that holds an N; their number is reported.
  (b) one     the same number of letters as ONE record, against the floor CRBM.scanSites(stream, 1.0): the same encode
              and gather work, next to no records.  The ratio (b) / floor is what the register-resident sums and the
              flushes cost; it is reported without a bar.
One warm-up of every route, then the median of 5 repeats each.  Writes profiles/records_bench.json (or the path given)
and prints the same JSON line; the run ends with an error when (a) is not faster than the host route.

usage: python tools/bench_records.py [letters] [output.json]
"""
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from crbm_amd import CRBM  # noqa: E402
from bench_calibrate import device_ms, timed  # noqa: E402


def gapped(T, seed, share=0.01, run=25):
    rng = np.random.default_rng(seed)
    s = rng.integers(0, 4, size=T, dtype=np.uint8)
    for a in rng.integers(0, T - run, size=max(1, int(T * share / run))):
        s[a:a + run] = 4
    return s


def many_records(T, seed):
    """(stream, offsets): records of 100..300 letters until T codes are used up, one code 4 between them"""
    rng = np.random.default_rng(seed)
    lengths = rng.integers(100, 301, size=T // 100 + 1)
    ends = np.cumsum(lengths + 1)
    R = int(np.searchsorted(ends, T + 1, side="right"))
    offsets = np.concatenate(([0], ends[:R])).astype(np.int64)
    stream = gapped(int(offsets[-1]) - 1, seed + 1)
    stream[offsets[1:-1] - 1] = 4
    return stream, offsets


def host_route(m, stream, offsets):
    """what a user does today: drop the records with an N, group the rest by length, one freeEnergy + motifBestSites
    call per group.  Returns (records served, groups)."""
    lengths = np.diff(offsets) - 1
    bad = np.concatenate(([0], np.cumsum(stream > 3)))
    clean = (bad[offsets[1:] - 1] - bad[offsets[:-1]]) == 0
    served = groups = 0
    for L in np.unique(lengths[clean]):
        if L < m.motif_length:
            continue
        rows = np.flatnonzero(clean & (lengths == L))
        codes = stream[offsets[rows][:, None] + np.arange(L)[None, :]]
        m.freeEnergy(codes, permotif=True)
        m.motifBestSites(codes)
        served += rows.size
        groups += 1
    return served, groups


def median5(fn):
    fn()
    return statistics.median(timed(fn) for _ in range(5))


def main():
    T = int(float(sys.argv[1])) if len(sys.argv) > 1 else 100000000
    path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "records_bench.json")
    K, M = 10, 15
    m = CRBM(K, M, doublestranded=True, batchsize=64, seed=1)
    m.motifs.set_value((np.random.default_rng(42).standard_normal((K, 1, 4, M)) * 0.7).astype(np.float32))
    m.bias.set_value(m.bias.get_value() + 3.0)
    stream_a, offsets = many_records(T, 77)
    stream_b = gapped(T, 78)
    one = np.array([0, T + 1], np.int64)
    R = offsets.size - 1
    served, groups = host_route(m, stream_a, offsets)
    res = {"model": "10x15 ds", "letters": T, "records": R, "host_route_records_served": served,
           "host_route_records_not_served": R - served, "host_route_groups": groups}
    res["many_s"] = median5(lambda: m.recordSummary(stream_a, offsets))
    res["many_device_ms"] = device_ms(lambda: m.recordSummary(stream_a, offsets), "CRBM_RECORDS_TIMING")
    res["host_route_s"] = median5(lambda: host_route(m, stream_a, offsets))
    res["one_s"] = median5(lambda: m.recordSummary(stream_b, one))
    res["one_device_ms"] = device_ms(lambda: m.recordSummary(stream_b, one), "CRBM_RECORDS_TIMING")
    res["floor_s"] = median5(lambda: m.scanSites(stream_b, 1.0))
    res["floor_device_ms"] = device_ms(lambda: m.scanSites(stream_b, 1.0), "CRBM_SCAN_TIMING")
    res["many_speedup_over_host_route"] = res["host_route_s"] / res["many_s"]
    res["one_over_floor"] = res["one_s"] / res["floor_s"]
    res["one_over_floor_device"] = res["one_device_ms"] / res["floor_device_ms"] if res["floor_device_ms"] else None
    line = json.dumps(res)
    with open(path, "w") as f:
        f.write(line + "\n")
    print(line)
    if not res["many_s"] < res["host_route_s"]:
        sys.exit("recordSummary (%.3f s) is not faster than the host route (%.3f s)" % (res["many_s"], res["host_route_s"]))


if __name__ == "__main__":
    main()
