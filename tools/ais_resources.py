"""VGPR / SGPR / scratch / static LDS of the annealed-importance-sampling kernel (crbm_ais) in the code object of every
model of __graft_entry__.PRECOMPILE: each model is compiled alone into an empty cache (CRBM_JIT_CACHE) and the kernel's
metadata read with llvm-readelf --notes.  Pooled models have an empty body (crbm_ais refuses them); models on the
generic path compile the modules of their slab models, which carry the kernel although crbm_ais refuses those models
too.  The dynamic LDS of a launch (gather table, set-bit top-down tables, one slice per wave) is printed for four waves
at L = 200.  Needs no GPU.

usage: python tools/ais_resources.py [> profiles/ais_resources.txt]
"""
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from sites_resources import kernel_meta   # noqa: E402


def lds_bytes(K, M, ds, G, L, waves=4):
    """crbm_layout.h: ais_layout / ais_lds_bytes"""
    cdiv = lambda a, b: (a + b - 1) // b
    KP, NW = 4 * cdiv(K, 4), cdiv(K, 32)
    tables = cdiv(M, G) * 4 ** G * KP + (M + 7) * K * 4 * (1 + ds) + 4
    nvb = cdiv(L, 4)
    Lrow = 4 * cdiv(4 * nvb + M - 1 + 3, 4)
    run_words = ((1 + ds) * Lrow * NW + cdiv(4 * nvb, 16) + 2 + 3) & ~3
    return 4 * (tables + waves * run_words)


def main():
    from __graft_entry__ import PRECOMPILE
    from crbm_amd.csrc import build as hip_build
    print("model (K x M, ds, pooling, Lf, batch) | module | body | VGPRs | SGPRs | scratch B/lane | static LDS B")
    worst = 0
    for c in PRECOMPILE:
        with tempfile.TemporaryDirectory() as d:
            os.environ["CRBM_JIT_CACHE"] = d
            hip_build.precompile([c], verbose=False)
            for f in sorted(os.listdir(d)):
                v, s, p, g = kernel_meta(os.path.join(d, f), "crbm_ais")
                worst = max(worst, p)
                print("%d x %d, ds=%d, pool=%d, Lf=%s, B=%s | %s | %s | %d | %d | %d | %d" % (
                    c["num_motifs"], c["motif_length"], c.get("doublestranded", 0), c.get("pooling", 1),
                    c.get("fantasy_hidden_len", 200), c.get("batchsize", 20), f[:22],
                    "empty (refused)" if c.get("pooling", 1) > 1 else "ais_body", v, s, p, g))
    print("dynamic LDS per block, four waves, L = 200: config #2's model (10 x 15, ss, G = 3) %d B; 10 x 15 ds %d B"
          % (lds_bytes(10, 15, 0, 3, 200), lds_bytes(10, 15, 1, 3, 200)))
    print("largest scratch of crbm_ais: %d bytes per lane" % worst)


if __name__ == "__main__":
    main()
