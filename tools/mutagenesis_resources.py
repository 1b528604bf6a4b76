"""VGPR / SGPR / scratch / static LDS of the mutagenesis kernel (crbm_mutagenesis) in the code object of every model of
__graft_entry__.PRECOMPILE plus 256 x 4 double-stranded and 100 x 15: each model is compiled alone into an empty
cache (CRBM_JIT_CACHE) and the kernel's metadata read with llvm-readelf --notes.  Pooled models have an empty body
(they take the general path: expand, the model's free-energy pass, combine); models on the generic path compile the
modules of their slab models, which carry the kernel too although the general path never launches it.  The dynamic
LDS of a launch (gather table + 3 planes of L rounded up to 64 floats per wave) is printed for L = 200.
Needs no GPU.

usage: python tools/mutagenesis_resources.py [> profiles/mutagenesis_resources.txt]
"""
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from sites_resources import kernel_meta   # noqa: E402


def main():
    from __graft_entry__ import PRECOMPILE
    from crbm_amd.csrc import build as hip_build
    models = list(PRECOMPILE) + [dict(num_motifs=256, motif_length=4, doublestranded=1),
                                 dict(num_motifs=100, motif_length=15, doublestranded=0)]
    print("model (K x M, ds, pooling, Lf, batch) | module | body | VGPRs | SGPRs | scratch B/lane | static LDS B")
    worst = 0
    for c in models:
        with tempfile.TemporaryDirectory() as d:
            os.environ["CRBM_JIT_CACHE"] = d
            hip_build.precompile([c], verbose=False)
            for f in sorted(os.listdir(d)):
                v, s, p, g = kernel_meta(os.path.join(d, f), "crbm_mutagenesis")
                worst = max(worst, p)
                print("%d x %d, ds=%d, pool=%d, Lf=%s, B=%s | %s | %s | %d | %d | %d | %d" % (
                    c["num_motifs"], c["motif_length"], c.get("doublestranded", 0), c.get("pooling", 1),
                    c.get("fantasy_hidden_len", 200), c.get("batchsize", 20), f[:22],
                    "empty (general path)" if c.get("pooling", 1) > 1 else "fused", v, s, p, g))
    print("dynamic LDS per block at L = 200: gather table + waves x 3 x 256 x 4 B (4 waves: 12288 B beside the table)")
    print("largest scratch of crbm_mutagenesis: %d bytes per lane" % worst)


if __name__ == "__main__":
    main()
