"""VGPR / SGPR / scratch / static LDS of the stream-scan kernel (crbm_scan_sites) in the code object of every model
of __graft_entry__.PRECOMPILE plus 256 x 4 double-stranded and 100 x 15: each model is compiled alone into an empty
cache (CRBM_JIT_CACHE) and the kernel's metadata read with llvm-readelf --notes.  Models on the generic path compile
the modules of their slab models, whose crbm_scan_sites is the one that runs (blockIdx.y = slab).  Pooled models carry
an empty body (refused on the host).  The gather table is dynamic LDS (ModelShape.TAB * 4 bytes, printed beside).
Scratch must be 0 everywhere: the script exits with an error otherwise.  Needs no GPU.

usage: python tools/scan_resources.py [> profiles/scan_resources.txt]
"""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
READELF = "/opt/rocm/llvm/bin/llvm-readelf"


def kernel_meta(hsaco, name):
    notes = subprocess.run([READELF, "--notes", hsaco], capture_output=True, text=True, check=True).stdout
    for block in notes.split("  - .agpr_count")[1:]:
        if re.search(r"\.name:\s+%s\n" % name, block):
            get = lambda key: int(re.search(r"\.%s:\s+(\d+)" % key, block).group(1))
            return get("vgpr_count"), get("sgpr_count"), get("private_segment_fixed_size"), get("group_segment_fixed_size")
    raise KeyError(name)


def main():
    from __graft_entry__ import PRECOMPILE
    from crbm_amd.csrc import build as hip_build
    models = list(PRECOMPILE) + [dict(num_motifs=256, motif_length=4, doublestranded=1),
                                 dict(num_motifs=100, motif_length=15, doublestranded=0)]
    print("model (K x M, ds, pooling, Lf, batch) | module | VGPRs | SGPRs | scratch B/lane | static LDS B")
    worst = 0
    for c in models:
        with tempfile.TemporaryDirectory() as d:
            os.environ["CRBM_JIT_CACHE"] = d
            hip_build.precompile([c], verbose=False)
            for f in sorted(os.listdir(d)):
                v, s, p, g = kernel_meta(os.path.join(d, f), "crbm_scan_sites")
                worst = max(worst, p)
                print("%d x %d, ds=%d, pool=%d, Lf=%s, B=%s | %s | %d | %d | %d | %d" % (
                    c["num_motifs"], c["motif_length"], c.get("doublestranded", 0), c.get("pooling", 1),
                    c.get("fantasy_hidden_len", 200), c.get("batchsize", 20), f[:22], v, s, p, g))
    print("largest scratch of crbm_scan_sites: %d bytes per lane" % worst)
    if worst:
        sys.exit("crbm_scan_sites uses scratch")


if __name__ == "__main__":
    main()
