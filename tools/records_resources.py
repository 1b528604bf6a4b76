"""VGPR / SGPR / scratch / static LDS of the record-summary kernel (crbm_scan_records) in the code object of every model
of __graft_entry__.PRECOMPILE: each model is compiled alone into an empty cache (CRBM_JIT_CACHE) and the kernel's
metadata read with llvm-readelf --notes.  Pooled models have an empty body (crbm_scan_records_codes refuses them);
models on the generic path compile the modules of their slab models; the modules of the geometry-specialised chain
kernels carry no stream kernel and are skipped.  The dynamic LDS of a launch is the model's gather
table alone.  Needs no GPU.

usage: python tools/records_resources.py [> profiles/records_resources.txt]
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
    print("model (K x M, ds, pooling, Lf, batch) | module | body | VGPRs | SGPRs | scratch B/lane | static LDS B")
    worst = 0
    for c in PRECOMPILE:
        with tempfile.TemporaryDirectory() as d:
            os.environ["CRBM_JIT_CACHE"] = d
            hip_build.precompile([c], verbose=False)
            for f in sorted(os.listdir(d)):
                try:
                    v, s, p, g = kernel_meta(os.path.join(d, f), "crbm_scan_records")
                except KeyError:             # the module of the geometry-specialised chain kernels: no stream kernels
                    continue
                worst = max(worst, p)
                print("%d x %d, ds=%d, pool=%d, Lf=%s, B=%s | %s | %s | %d | %d | %d | %d" % (
                    c["num_motifs"], c["motif_length"], c.get("doublestranded", 0), c.get("pooling", 1),
                    c.get("fantasy_hidden_len", 200), c.get("batchsize", 20), f[:22],
                    "empty (refused)" if c.get("pooling", 1) > 1 else "scan_records_body", v, s, p, g))
    print("largest scratch of crbm_scan_records: %d bytes per lane" % worst)


if __name__ == "__main__":
    main()
