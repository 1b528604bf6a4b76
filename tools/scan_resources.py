"""VGPR / SGPR / scratch / static LDS of the named kernels (default: the stream-scan kernel, crbm_scan_sites) in the
code object of every model of __graft_entry__.PRECOMPILE plus 256 x 4 double-stranded and 100 x 15: each model is
compiled alone into an empty cache (CRBM_JIT_CACHE) and the kernels' metadata read with llvm-readelf --notes.  Models
on the generic path compile the modules of their slab models, whose kernels are the ones that run (blockIdx.y = slab).
Pooled models carry an empty body of the stream kernels (refused on the host).  The gather table is dynamic LDS
(ModelShape.TAB * 4 bytes).  Scratch must be 0 everywhere: the script exits with an error otherwise.  Needs no GPU.

usage: python tools/scan_resources.py [kernel ...] [> profiles/scan_resources.txt]
"""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
READELF = "/opt/rocm/llvm/bin/llvm-readelf"


def kernel_meta(notes, name):
    for block in notes.split("  - .agpr_count")[1:]:
        if re.search(r"\.name:\s+%s\n" % name, block):
            get = lambda key: int(re.search(r"\.%s:\s+(\d+)" % key, block).group(1))
            return get("vgpr_count"), get("sgpr_count"), get("private_segment_fixed_size"), get("group_segment_fixed_size")
    raise KeyError(name)


def main():
    from __graft_entry__ import PRECOMPILE
    from crbm_amd.csrc import build as hip_build
    kernels = sys.argv[1:] or ["crbm_scan_sites"]
    models = list(PRECOMPILE) + [dict(num_motifs=256, motif_length=4, doublestranded=1),
                                 dict(num_motifs=100, motif_length=15, doublestranded=0)]
    print("model (K x M, ds, pooling, Lf, batch) | module | kernel | VGPRs | SGPRs | scratch B/lane | static LDS B")
    worst = {k: 0 for k in kernels}
    for c in models:
        with tempfile.TemporaryDirectory() as d:
            os.environ["CRBM_JIT_CACHE"] = d
            hip_build.precompile([c], verbose=False)
            for f in sorted(os.listdir(d)):
                notes = subprocess.run([READELF, "--notes", os.path.join(d, f)], capture_output=True, text=True, check=True).stdout
                for k in kernels:
                    try:
                        v, s, p, g = kernel_meta(notes, k)
                    except KeyError:     # the module of the geometry-specialised chain kernels carries no other kernel
                        continue
                    worst[k] = max(worst[k], p)
                    print("%d x %d, ds=%d, pool=%d, Lf=%s, B=%s | %s | %s | %d | %d | %d | %d" % (
                        c["num_motifs"], c["motif_length"], c.get("doublestranded", 0), c.get("pooling", 1),
                        c.get("fantasy_hidden_len", 200), c.get("batchsize", 20), f[:22], k, v, s, p, g))
    for k in kernels:
        print("largest scratch of %s: %d bytes per lane" % (k, worst[k]))
    if any(worst.values()):
        sys.exit("scratch in use: %s" % ", ".join(k for k in kernels if worst[k]))


if __name__ == "__main__":
    main()
