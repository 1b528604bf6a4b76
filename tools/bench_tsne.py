"""t-SNE of motif abundances, stage by stage, in one process: the features are motifHitSummary(...)["max"] of config #2's
model (10 x 15, double-stranded) on random 200-letter codes with instances of three of its motifs planted in thirds of the
rows; n = 4 000 (the tutorial's size), 20 000 and 100 000 rows by default.
  per n   neighbours, affinities, symmetrisation (host) and 1000 iterations of the descent, each the median of 5 after one
          warm-up; the device time per iteration from HIP events around the iterations of crbm_tsne_descend
          (crbm_tsne_descend_ms); the repulsion's pair terms per second, n^2 per iteration over that device time -- a lower
          bound, the time holds the attraction and the sums too -- beside the fp32 vector peak (157.3 TFLOP/s = 78.6 T
          fused multiply-adds per second; a pair is nine vector instructions).
  against where scikit-learn imports: TSNE(method="barnes_hut", n_jobs=16) on the same features at n = 4 000 and 20 000,
          once each; the run ends with an error when tsneEmbed (all four stages, its defaults) is not faster.  Where it
          does not import, that is recorded and nothing is compared.
The shader clock is warmed up first, as bench.py does: 3000 Gibbs steps of the model's chains.  Writes
profiles/tsne_bench.json (or the path given) and prints the same JSON line.

usage: python tools/bench_tsne.py [sizes, comma-separated] [output.json]
"""
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from crbm_amd import CRBM, tsne, tsneEmbed  # noqa: E402

PEAK_FMA_PER_S = 157.3e12 / 2
REPEATS = 5


def features(model, n, seed):
    """(n, K) float32: the largest hit probability per row and motif; rows of third t carry an instance of motif t"""
    rng = np.random.default_rng(seed)
    codes = rng.integers(0, 4, size=(n, 200), dtype=np.uint8)
    W = model.motifs.get_value()[:, 0]                          # (K, 4, M)
    M = W.shape[2]
    for t in range(3):
        rows = np.arange(t, n, 3)
        at = rng.integers(0, 200 - M, size=rows.size)
        codes[rows[:, None], at[:, None] + np.arange(M)[None, :]] = W[t].argmax(axis=0)[None, :]
    return model.motifHitSummary(codes, position_mean=False)["max"]


def median_s(fn):
    fn()
    times = []
    for _ in range(REPEATS):
        t = time.perf_counter()
        out = fn()
        times.append(time.perf_counter() - t)
    return statistics.median(times), out


def one_size(model, n, seed):
    X = features(model, n, seed)
    perplexity, ee = 30.0, 12.0
    k = min(n - 1, 90)
    lr = max(n / ee / 4.0, 50.0)
    row = {"n": n, "D": int(X.shape[1]), "k": k}
    row["neighbors_s"], (idx, d2) = median_s(lambda: tsne.neighbors(model, X, k))
    row["affinities_s"], (p, beta) = median_s(lambda: tsne.affinities(model, d2, perplexity))
    row["symmetrize_host_s"], P = median_s(lambda: tsne.symmetrize(idx, p))
    row["nnz"] = int(P[2].size)
    y0 = (1e-4 * np.random.default_rng(seed).standard_normal((n, 2))).astype(np.float32)
    ms = ctypes.c_float(0.0)
    device = []

    def run():
        y, v, g = y0.copy(), np.zeros((n, 2), np.float32), np.ones((n, 2), np.float32)
        total = 0.0
        for count, ex, mom in ((250, ee, 0.5), (750, 1.0, 0.8)):
            tsne.descend(model, P, y, v, g, count, ex, lr, mom)
            model._call("crbm_tsne_descend_ms", ctypes.byref(ms))
            total += ms.value
        device.append(total)
        return y
    row["descend_1000_s"], y = median_s(run)
    row["device_ms_per_iteration"] = statistics.median(device[1:]) / 1000.0
    row["pair_terms_per_s"] = float(n) * n / (row["device_ms_per_iteration"] * 1e-3)
    row["fp32_peak_fma_per_s"] = PEAK_FMA_PER_S
    row["share_of_peak_at_9_instructions_per_pair"] = row["pair_terms_per_s"] * 9 / PEAK_FMA_PER_S
    row["finite"] = bool(np.isfinite(y).all())
    return row, X


def main():
    sizes = [int(s) for s in sys.argv[1].split(",")] if len(sys.argv) > 1 else [4000, 20000, 100000]
    path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "tsne_bench.json")
    model = CRBM(num_motifs=10, motif_length=15, seed=7)             # double-stranded, the shape of config #2
    model.motifs.set_value(np.random.default_rng(5).standard_normal((10, 1, 4, 15)).astype(np.float32))
    model.bias.set_value(np.full((1, 10), -6.0, np.float32))
    model.gibbsSteps(3000)                                       # the clock is up before anything is timed
    out = {"workload": "t-SNE of motifHitSummary max, config #2's model double-stranded, perplexity 30, 1000 iterations",
           "repeats": REPEATS, "sizes": []}
    try:
        from sklearn.manifold import TSNE
        import sklearn
        out["sklearn"] = sklearn.__version__
    except Exception as e:                                       # recorded, nothing compared
        TSNE = None
        out["sklearn"] = "does not import: %s" % type(e).__name__
    slower = []
    for n in sizes:
        row, X = one_size(model, n, seed=n)
        if n <= 20000:
            row["tsneEmbed_s"], _ = median_s(lambda: tsneEmbed(model, X))
            if TSNE is not None:
                t = time.perf_counter()
                TSNE(method="barnes_hut", n_jobs=16).fit_transform(X)
                row["sklearn_barnes_hut_s"] = time.perf_counter() - t
                row["ratio"] = row["tsneEmbed_s"] / row["sklearn_barnes_hut_s"]
                if row["ratio"] >= 1.0:
                    slower.append(n)
        out["sizes"].append(row)
        print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))
    if slower:
        raise SystemExit("tsneEmbed is not faster than scikit-learn's Barnes-Hut at n = %s" % slower)


if __name__ == "__main__":
    main()
