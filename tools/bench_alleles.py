"""Allele effects against the route that exists without them, end to end, in one process: config #2's double-stranded
model (10 x 15), a stream of 10^7 letters with 1 % of them inside gap runs, 10^6 variants by default, 85 % SNPs and 15 %
indels of 1-20 letters (insertions and deletions in equal parts).
  alleles      CRBM.alleleEffects(stream, pos, ref, alt)["dfe"]
  free energy  both haplotype rows (M - 1 letters on either side of the allele) built on the host, grouped by length,
               CRBM.freeEnergy on each group, L_alt * fe_alt - L_ref * fe_ref -- possible only where both rows hold
               letters alone; the variants it cannot serve (a gap or a stream end within M - 1 letters) are counted
One warm-up, then the median of 5 repeats of each route, interleaved; the largest difference between the two on the
variants the old route serves is reported against RTOL |want| + RTOL max|want| + RTOL mass, RTOL = 1e-4, with mass the
two free energies that are subtracted.  The kernels' device time (all kernels of all chunks: CRBM_ALLELE_TIMING) comes
from a sixth call.  Also reported, with no bar set: alleleEffects / variantEffects on the SNP subset (the SNP kernel
looks up one other table row per window where this one scores both haplotypes in full).  Writes
profiles/alleles_bench.json and prints the same JSON line; exits with status 1 if the new call is not faster.

usage: python tools/bench_alleles.py [letters] [variants]
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
from tools.bench_variants import gapped_stream  # noqa: E402

RTOL = 1e-4
LETTERS = np.frombuffer(b"ACGTN", np.uint8)


def by_free_energy(m, stream, pos, R, alt_off, alt_codes):
    """the route without alleleEffects: (dfe of the variants it serves, the sum of the two |F|, their indices)"""
    M = m.motif_length
    A = np.diff(alt_off)
    lo, hi = pos - (M - 1), pos + R + (M - 1)
    inside = np.flatnonzero((lo >= 0) & (hi <= stream.size))
    gaps = np.concatenate([[0], np.cumsum(stream > 3)])
    served = inside[gaps[hi[inside]] == gaps[lo[inside]]]
    F = np.zeros((2, pos.size))
    for r in np.unique(R[served]):
        idx = served[R[served] == r]
        rows = stream[lo[idx, None] + np.arange(r + 2 * (M - 1))[None, :]]
        F[0, idx] = rows.shape[1] * m.freeEnergy(np.ascontiguousarray(rows)).astype(np.float64)
    for a in np.unique(A[served]):
        idx = served[A[served] == a]
        left = stream[lo[idx, None] + np.arange(M - 1)[None, :]]
        mid = alt_codes[alt_off[idx, None] + np.arange(a)[None, :]]
        right = stream[(pos[idx] + R[idx])[:, None] + np.arange(M - 1)[None, :]]
        rows = np.ascontiguousarray(np.concatenate([left, mid, right], axis=1))
        F[1, idx] = rows.shape[1] * m.freeEnergy(rows).astype(np.float64)
    return (F[1] - F[0])[served], (np.abs(F[0]) + np.abs(F[1]))[served], served


def main():
    T = int(float(sys.argv[1])) if len(sys.argv) > 1 else 10000000
    V = int(float(sys.argv[2])) if len(sys.argv) > 2 else 1000000
    K, M = 10, 15
    stream = gapped_stream(T, 1234)
    rng = np.random.default_rng(99)
    kind = rng.random(V)                                   # < 0.85 SNP, then insertions and deletions in equal parts
    length = rng.integers(1, 21, size=V)
    R = np.where(kind < 0.85, 1, np.where(kind < 0.925, 0, length)).astype(np.int64)
    A = np.where(kind < 0.85, 1, np.where(kind < 0.925, length, 0)).astype(np.int64)
    pos = rng.integers(0, T - 20, size=V)
    alt_off = np.concatenate([[0], np.cumsum(A)]).astype(np.int64)
    alt_codes = rng.integers(0, 4, size=int(alt_off[-1])).astype(np.uint8)
    snp = np.flatnonzero(kind < 0.85)
    alt_codes[alt_off[snp]] = (np.minimum(stream[pos[snp]], 3) + rng.integers(1, 4, size=snp.size)) % 4      # never the reference letter
    text = LETTERS[alt_codes].tobytes().decode()
    alt = [text[a:b] for a, b in zip(alt_off[:-1].tolist(), alt_off[1:].tolist())]
    rtext = LETTERS[stream].tobytes().decode()
    ref = [rtext[p:p + r] for p, r in zip(pos.tolist(), R.tolist())]
    m = CRBM(K, M, doublestranded=True, batchsize=64, seed=1)
    m.motifs.set_value((np.random.default_rng(42).standard_normal((K, 1, 4, M)) * 0.7).astype(np.float32))
    m.bias.set_value(m.bias.get_value() + 3.0)
    new = m.alleleEffects(stream, pos, ref, alt)           # warm-up of both routes, and their agreement
    old, mass, served = by_free_energy(m, stream, pos, R, alt_off, alt_codes)
    err = np.abs(new["dfe"][served].astype(np.float64) - old)
    bound = RTOL * np.abs(old) + RTOL * np.abs(old).max() + RTOL * mass
    snp_alt = alt_codes[alt_off[snp]]
    m.variantEffects(stream, pos[snp], snp_alt)
    snp_ref, snp_alts = [ref[i] for i in snp], [alt[i] for i in snp]
    tn, to, ts, tv = [], [], [], []
    for _ in range(5):
        for times, fn in ((tn, lambda: m.alleleEffects(stream, pos, ref, alt)),
                          (to, lambda: by_free_energy(m, stream, pos, R, alt_off, alt_codes)),
                          (ts, lambda: m.alleleEffects(stream, pos[snp], snp_ref, snp_alts)),
                          (tv, lambda: m.variantEffects(stream, pos[snp], snp_alt))):
            t = time.perf_counter()
            fn()
            times.append(time.perf_counter() - t)
    med = lambda x: statistics.median(x) * 1e3
    out = {"letters": T, "variants": V, "snps": int(snp.size), "K": K, "M": M, "ds": True, "gap_share": float((stream > 3).mean()),
           "not_served_by_free_energy": int(V - served.size), "zeros_by_definition": int((new["windows"].sum(axis=1) == 0).sum()),
           "max_abs_difference": float(err.max()), "max_abs_dfe": float(np.abs(old).max()),
           "worst_difference_over_bound": float((err / bound).max()), "routes_agree": bool(np.all(err <= bound)),
           "alleles_ms": [round(x * 1e3, 2) for x in tn], "free_energy_ms": [round(x * 1e3, 2) for x in to],
           "alleles_median_ms": med(tn), "free_energy_median_ms": med(to),
           "alleles_on_snps_median_ms": med(ts), "variants_on_snps_median_ms": med(tv)}
    out["alleles_over_free_energy"] = out["alleles_median_ms"] / out["free_energy_median_ms"]
    out["alleles_over_variants_on_snps"] = out["alleles_on_snps_median_ms"] / out["variants_on_snps_median_ms"]
    out["alleles_kernels_device_ms"] = device_ms(lambda: m.alleleEffects(stream, pos, ref, alt), "CRBM_ALLELE_TIMING")
    out["alleles_on_snps_kernels_device_ms"] = device_ms(lambda: m.alleleEffects(stream, pos[snp], snp_ref, snp_alts), "CRBM_ALLELE_TIMING")
    out["variants_on_snps_kernels_device_ms"] = device_ms(lambda: m.variantEffects(stream, pos[snp], snp_alt), "CRBM_VARIANT_TIMING")
    out["alleles_faster"] = out["alleles_median_ms"] < out["free_energy_median_ms"]
    line = json.dumps(out)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "alleles_bench.json"), "w") as f:
        f.write(line + "\n")
    print(line)
    return 0 if out["alleles_faster"] and out["routes_agree"] else 1


if __name__ == "__main__":
    sys.exit(main())
