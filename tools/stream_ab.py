"""Digests of what the stream features return, for comparing two revisions bit for bit: run this script on a checkout of
each and diff the outputs.  Models: CLASSES[0..3] of tests/test_gpu_sweeps.py (10 x 15 and 20 x 15 double-stranded,
300 x 10 and 257 x 1 as slabs of 60 motifs); stream: gapped_stream(5003, 2031) of tests/test_gpu_scan.py, at the
threshold its _threshold picks; CRBM_SLAB_BYTES unset (one segment) and set for 7 segments.  One line per model, budget
and call with the number of records (or valid windows) and a SHA-256 over every field:
  scanSites(stream, thr) | motifSites of a (64, 200) block of random letters at thr | scoreHistogram(bins=64, lo=-8, hi=8)
Needs a GPU.

usage: python tools/stream_ab.py [> digests.txt]
"""
import hashlib
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests.test_gpu_sweeps import CLASSES, _model, _codes  # noqa: E402
from tests.test_gpu_scan import gapped_stream, per_start, _threshold  # noqa: E402

T, SEED = 5003, 2031


def records_digest(r):
    h = hashlib.sha256()
    for f in ("seq", "motif", "start", "strand"):
        h.update(np.ascontiguousarray(r[f]).astype(np.int64).tobytes())
    h.update(np.ascontiguousarray(r["prob"]).astype(np.float32).view(np.uint32).tobytes())
    return "%d %s" % (r.size, h.hexdigest())


def main():
    stream = gapped_stream(T, SEED)
    block = _codes(64, 200, 4, seed=SEED)
    with pytest.MonkeyPatch.context() as mp:
        for cls in CLASSES[:4]:
            name, M = cls[0], cls[2]
            m, o = _model(cls, mp)
            thr = _threshold(o, stream)[2]
            starts = T - M + 1
            for budget in (None, per_start(cls) * (starts // 7 + 1)):
                if budget is None:
                    mp.delenv("CRBM_SLAB_BYTES", raising=False)
                else:
                    mp.setenv("CRBM_SLAB_BYTES", str(budget))
                tag = "%s %s" % (name, "default" if budget is None else "7-segments")
                print(tag, "scanSites", records_digest(m.scanSites(stream, thr)))
                print(tag, "motifSites", records_digest(m.motifSites(block, thr)))
                hist = m.scoreHistogram(stream, bins=64, lo=-8.0, hi=8.0)
                print(tag, "scoreHistogram", hist.windows,
                      hashlib.sha256(np.ascontiguousarray(hist.counts).astype(np.int64).tobytes()).hexdigest())
                sys.stdout.flush()


if __name__ == "__main__":
    main()
