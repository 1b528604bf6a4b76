"""Digests of what the stream features return, for comparing two revisions bit for bit: run this script on a checkout of
each and diff the outputs.  Models: CLASSES[0..3] of tests/test_gpu_sweeps.py (10 x 15 and 20 x 15 double-stranded,
300 x 10 and 257 x 1 as slabs of 60 motifs); stream: gapped_stream(5003, 2031) of tests/test_gpu_scan.py, at the
threshold its _threshold picks; CRBM_SLAB_BYTES unset (one segment or chunk) and set for 7 of them, by each call's own
cost per window start, per variant or per allele.  One line per model, budget and call with the number of records (or
valid windows, or variants) and a SHA-256 over every field, floats by their bit pattern:
  scanSites(stream, thr) | motifSites of a (64, 200) block of random letters at thr | scoreHistogram(bins=64, lo=-8, hi=8)
  recordSummary(stream, offsets) with the stream cut into six records at codes 4
  variantEffects of variant_list(stream, M, 300, 77) (tests/variant_reference.py)
  alleleEffects of allele_list(stream, M, 300, 77) (tests/allele_reference.py: SNPs, insertions, deletions, block
  substitutions, alleles of 70 and 130 letters), untrimmed
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
from tests.test_gpu_variants import per_variant  # noqa: E402
from tests.test_gpu_alleles import costs  # noqa: E402
from tests.variant_reference import variant_list  # noqa: E402
from tests.allele_reference import allele_list, strings  # noqa: E402

T, SEED = 5003, 2031


def records_digest(r):
    h = hashlib.sha256()
    for f in ("seq", "motif", "start", "strand"):
        h.update(np.ascontiguousarray(r[f]).astype(np.int64).tobytes())
    h.update(np.ascontiguousarray(r["prob"]).astype(np.float32).view(np.uint32).tobytes())
    return "%d %s" % (r.size, h.hexdigest())


def dict_digest(d):
    """every field of a returned dict in the order of its names: arrays by their bytes (floats by their bit pattern,
    integers widened to 64 bits), scalars by their repr"""
    h = hashlib.sha256()
    for key in sorted(d):
        v = d[key]
        h.update(key.encode())
        if isinstance(v, np.ndarray):
            v = np.ascontiguousarray(v)
            h.update(repr(v.shape).encode())
            h.update((v if v.dtype.kind == "f" else v.astype(np.int64)).tobytes())
        else:
            h.update(repr(v).encode())
    return h.hexdigest()


def record_offsets(stream):
    """the stream as six records, cut behind five of its codes 4 spread over them: its two gap runs give long records
    of letters and short ones of codes 4 alone (no valid window)"""
    gaps = np.flatnonzero(stream[1:-1] == 4) + 1
    cuts = gaps[np.linspace(0, gaps.size - 1, 5).astype(np.int64)]
    return np.concatenate([[0], np.unique(cuts) + 1, [stream.size + 1]]).astype(np.int64)


def main():
    stream = gapped_stream(T, SEED)
    block = _codes(64, 200, 4, seed=SEED)
    offsets = record_offsets(stream)
    with pytest.MonkeyPatch.context() as mp:
        for cls in CLASSES[:4]:
            name, M = cls[0], cls[2]
            m, o = _model(cls, mp)
            thr = _threshold(o, stream)[2]
            starts = T - M + 1
            vpos, valt = variant_list(stream, M, 300, 77)
            apos, aR, aalts = allele_list(stream, M, 300, 77)
            aref, aalt = strings(stream, apos, aR, aalts)
            budgets = {"segments": per_start(cls) * (starts // 7 + 1), "variants": per_variant(cls) * (vpos.size // 7 + 1),
                       "alleles": int(costs(cls, aR, aalts).sum()) // 7}
            for seven in (False, True):
                def budget(unit):
                    if seven:
                        mp.setenv("CRBM_SLAB_BYTES", str(budgets[unit]))
                    else:
                        mp.delenv("CRBM_SLAB_BYTES", raising=False)
                tag = "%s %s" % (name, "7-segments" if seven else "default")
                budget("segments")
                print(tag, "scanSites", records_digest(m.scanSites(stream, thr)))
                print(tag, "motifSites", records_digest(m.motifSites(block, thr)))
                hist = m.scoreHistogram(stream, bins=64, lo=-8.0, hi=8.0)
                print(tag, "scoreHistogram", hist.windows,
                      hashlib.sha256(np.ascontiguousarray(hist.counts).astype(np.int64).tobytes()).hexdigest())
                rec = m.recordSummary(stream, offsets)
                print(tag, "recordSummary", int(rec["windows"].sum()), dict_digest(rec))
                budget("variants")
                print(tag, "variantEffects", vpos.size, dict_digest(m.variantEffects(stream, vpos, valt)))
                budget("alleles")
                print(tag, "alleleEffects", apos.size, dict_digest(m.alleleEffects(stream, apos, aref, aalt, trim=False)))
                sys.stdout.flush()


if __name__ == "__main__":
    main()
