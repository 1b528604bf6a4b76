"""CPU-only checks of CRBM.alleleEffects (crbm_amd/crbm.py) and sequences.readVcf: everything alleleEffects refuses is
refused before the library is reached -- ref and alt by form and letters, the ref check against the stream, spans
outside their record or the stream, lengths beyond the C call's; trimming removes the common prefix, then the common
suffix, and advances pos; variants that are empty or whose span holds a code 4 get zeros on the host and are not sent;
`seq` / `offsets` map record positions to stream positions; a long stream is cut at record boundaries and the outputs
come back in the caller's order.  readVcf on a file written here: multi-allelic, symbolic, breakend and unknown-contig
lines, gz, lower case.  The entry point is declared, documented, bound and exported."""
import ctypes
import gzip
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _model(monkeypatch, K=3, M=4):
    from crbm_amd import CRBM
    m = CRBM(K, M)
    monkeypatch.setattr(m, "_h", lambda: None)           # no GPU here: the checks must fire before any call
    monkeypatch.setattr(m, "_call", lambda *a: (_ for _ in ()).throw(AssertionError("reached the library")))
    return m


def _recording(m, monkeypatch, K=3):
    """m._call replaced by a stand-in that records (piece, pos, ref_len, alts) and writes recognisable outputs"""
    calls = []

    def fake(name, codes, T, nvar, pos, ref_len, alt_off, alt_codes, dfe, pm, win):
        assert name == "crbm_allele_effects_codes"
        piece = np.ctypeslib.as_array(codes, (T,)).copy()
        p, r = np.ctypeslib.as_array(pos, (nvar,)).copy(), np.ctypeslib.as_array(ref_len, (nvar,)).copy()
        off = np.ctypeslib.as_array(alt_off, (nvar + 1,)).copy()
        ac = np.ctypeslib.as_array(alt_codes, (int(off[-1]),)).copy() if off[-1] else np.zeros(0, np.uint8)
        assert off[0] == 0 and np.all(np.diff(off) >= 0)
        alts = ["".join("ACGT"[c] for c in ac[off[i]:off[i + 1]]) for i in range(nvar)]
        calls.append((piece, p.tolist(), r.tolist(), alts))
        np.ctypeslib.as_array(dfe, (nvar,))[:] = 100 * len(calls) + p
        np.ctypeslib.as_array(pm, (nvar, K))[:] = r[:, None] + np.arange(K)[None, :]
        np.ctypeslib.as_array(win, (nvar, 2))[:] = np.stack([r, np.diff(off)], axis=1)
    monkeypatch.setattr(m, "_call", fake)
    return calls


def test_entry_point_is_declared_documented_bound_and_exported():
    import crbm_amd
    from crbm_amd import _lib
    header = open(os.path.join(ROOT, "include", "crbm_amd.h")).read()
    assert re.search(r"int crbm_allele_effects_codes\(crbm_handle\* h, const uint8_t\* codes, int64_t T, int64_t nvar,\s+"
                     r"const int64_t\* pos, const int32_t\* ref_len,\s+const int64_t\* alt_off /\* nvar\+1, ascending from 0 \*/, "
                     r"const uint8_t\* alt_codes,\s+float\* dfe, float\* dfe_per_motif, int32_t\* windows\);", header)
    res, args = _lib.SIGNATURES["crbm_allele_effects_codes"]
    assert res is ctypes.c_int32 and len(args) == 11 and args[2] is ctypes.c_int64 and args[3] is ctypes.c_int64
    assert args[4] is _lib._I64P and args[5] is _lib._I32P and args[6] is _lib._I64P and args[7] is _lib._U8P and args[10] is _lib._I32P
    assert hasattr(_lib.load(), "crbm_allele_effects_codes")
    assert crbm_amd.readVcf is crbm_amd.sequences.readVcf
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        assert "alleleEffects" in open(os.path.join(ROOT, doc)).read(), doc


def test_allele_effects_refuses_bad_arguments_before_the_c_side(monkeypatch):
    m = _model(monkeypatch)
    s = np.array([0, 1, 2, 3, 4, 0, 1, 2, 3, 0], np.uint8)           # ACGT N ACGTA
    with pytest.raises(ValueError, match="uint8"):
        m.alleleEffects(s.astype(np.int32), [1], ["C"], ["G"])
    with pytest.raises(ValueError, match="pos must be a 1-D integer"):
        m.alleleEffects(s, np.array([1.0]), ["C"], ["G"])
    with pytest.raises(ValueError, match="ref must be a sequence of strings"):
        m.alleleEffects(s, [1, 2], "CG", ["G", "A"])
    with pytest.raises(ValueError, match="alt must be a sequence of strings"):
        m.alleleEffects(s, [1], ["C"], [np.uint8(2)])
    with pytest.raises(ValueError, match="alt must hold one entry per variant"):
        m.alleleEffects(s, [1, 2], ["C", "G"], ["G"])
    with pytest.raises(ValueError, match="alt must hold letters"):
        m.alleleEffects(s, [1], ["C"], ["GN"])
    with pytest.raises(ValueError, match="alt must hold letters"):
        m.alleleEffects(s, [1], ["C"], ["<DEL>"])
    with pytest.raises(ValueError, match="ref must hold letters"):
        m.alleleEffects(s, [1], ["CX"], ["G"])
    with pytest.raises(ValueError, match=r"outside the stream at variants \[1\]"):
        m.alleleEffects(s, [1, 9], ["C", "AC"], ["G", "A"])
    with pytest.raises(ValueError, match=r"outside the stream at variants \[0\]"):
        m.alleleEffects(s, [-1, 7], ["C", "G"], ["G", "A"])
    with pytest.raises(ValueError, match=r"outside the stream at variants \[0\]"):
        m.alleleEffects(s, [11], [""], ["G"])                        # pos = T + 1; pos = T is an insertion behind the last code
    with pytest.raises(ValueError, match=r"ref does not match the stream at 2 of 4 variants, the first at indices \[0, 2\] \(another assembly\?\)"):
        m.alleleEffects(s, [1, 5, 3, 3], ["CC", "acg", "TA", "TN"], ["G", "A", "", "C"])
    with pytest.raises(ValueError, match="seq needs the offsets"):
        m.alleleEffects(s, [1], ["C"], ["G"], seq=[0])
    off = np.array([0, 5, 11])                                       # records [0, 4) and [5, 10)
    with pytest.raises(ValueError, match=r"seq must lie in \[0, 2\)"):
        m.alleleEffects(s, [1], ["C"], ["G"], offsets=off, seq=[2])
    with pytest.raises(ValueError, match="one record index per variant"):
        m.alleleEffects(s, [1, 2], ["C", "G"], ["G", "A"], offsets=off, seq=[0])
    with pytest.raises(ValueError, match=r"pos outside its record at variants \[1\]"):
        m.alleleEffects(s, [1, 3], ["C", "TN"], ["G", "A"], offsets=off, seq=[0, 0])      # the separator is not part of record 0
    monkeypatch.setattr(type(m), "_ALLELE_MAX", 2)
    with pytest.raises(ValueError, match=r"at most 2 letters each; longer at variants \[1\]"):
        m.alleleEffects(s, [1, 5], ["C", "A"], ["GG", "CTT"])


def test_trimming_zeros_and_what_reaches_the_library(monkeypatch):
    from crbm_amd import CRBM
    m = CRBM(3, 4)
    monkeypatch.setattr(m, "_h", lambda: None)
    calls = _recording(m, monkeypatch)
    s = np.array([0, 1, 2, 3, 4, 0, 1, 2, 3, 0], np.uint8)           # ACGT N ACGTA
    pos = [0, 0, 5, 1, 3, 2, 10, 6, 0]
    ref = ["AC", "ACG", "ACGT", "C", "TN", "g", "", "CG", "."]
    alt = ["A", "ATG", "AT", "c", "T", "GA", "-", "CGCG", "T"]
    out = m.alleleEffects(s, pos, ref, alt)
    # AC>A: the anchor goes, a deletion of C at 1.  ACG>ATG: prefix A and suffix G go, C>T at 1.  ACGT>AT: prefix A, then
    # suffix T: CG deleted at 6.  C>c and the empty pair trim to nothing: zeros, not sent.  TN>T: N is left, a span on a
    # code 4: zeros.  g>GA: an insertion of A at 3.  CG>CGCG: the prefix is taken first, CG inserted at 8.  .>T at 0.
    assert len(calls) == 1 and calls[0][0].tolist() == s.tolist()
    assert calls[0][1:] == ([1, 1, 6, 3, 8, 0], [1, 1, 2, 0, 0, 0], ["", "T", "", "A", "CG", "T"])
    assert out["dfe"].tolist() == [101, 101, 106, 0, 0, 103, 0, 108, 100] and out["dfe"].dtype == np.float32
    assert out["windows"].tolist() == [[1, 0], [1, 1], [2, 0], [0, 0], [0, 0], [0, 1], [0, 0], [0, 2], [0, 1]]
    assert out["windows"].dtype == np.int32 and out["per_motif"].shape == (9, 3) and np.all(out["per_motif"][[3, 4, 6]] == 0)
    calls.clear()
    out = m.alleleEffects(s, pos, ref, alt, trim=False)              # as given: only the empty pair and the span on N stay behind
    assert calls[0][1:] == ([0, 0, 5, 1, 2, 6, 0], [2, 3, 4, 1, 1, 2, 0], ["A", "ATG", "AT", "C", "GA", "CGCG", "T"])
    assert out["dfe"].tolist() == [100, 100, 105, 101, 0, 102, 0, 106, 100]
    calls.clear()
    out = m.alleleEffects(s, [10], [""], ["acgt"])                   # pos = T: behind the last code
    assert calls[0][1:] == ([10], [0], ["ACGT"])
    empty = m.alleleEffects(s, np.zeros(0, np.int64), [], [])
    assert empty["dfe"].shape == (0,) and empty["per_motif"].shape == (0, 3) and empty["windows"].shape == (0, 2)


def test_allele_effects_maps_records_cuts_long_streams_and_restores_the_order(monkeypatch):
    from crbm_amd import CRBM
    m = CRBM(3, 4)
    monkeypatch.setattr(m, "_h", lambda: None)
    monkeypatch.setattr(CRBM, "_SCAN_MAX", 12)
    recs = ["ACGTAC", "TTNG", "CAGGTCA"]
    from crbm_amd import seqsToStream
    stream, off, _ = seqsToStream(recs)
    assert off.tolist() == [0, 7, 12, 20]
    calls = _recording(m, monkeypatch)
    seq, pos = np.array([2, 0, 1, 2, 0, 1, 0]), np.array([5, 4, 0, 0, 0, 3, 6])
    out = m.alleleEffects(stream, pos, ["CA", "AC", "T", "", "A", "G", ""], ["C", "A", "TA", "GG", "T", "", "T"], offsets=off, seq=seq)
    # pieces of at most 12 letters, cut at record boundaries: records 0 and 1 (stream [0, 11)), then record 2 ([12, 19))
    assert [c[0].tolist() for c in calls] == [stream[:11].tolist(), stream[12:].tolist()]
    assert calls[0][1:] == ([5, 8, 0, 10, 6], [1, 0, 1, 1, 0], ["", "A", "T", "", "T"])      # the insertion at the end of record 0: pos = its length
    assert calls[1][1:] == ([6, 0], [1, 0], ["", "GG"])
    assert out["dfe"].tolist() == [206, 105, 108, 200, 100, 110, 106]
    with pytest.raises(ValueError, match=r"pos outside its record at variants \[0\]"):
        m.alleleEffects(stream, [7], [""], ["T"], offsets=off, seq=[0])
    calls.clear()
    out = m.alleleEffects(stream, [11, 3], ["N", "T"], ["T", "g"], offsets=off)      # on the separator between the pieces: zeros
    assert len(calls) == 1 and calls[0][1:] == ([3], [1], ["G"]) and out["dfe"].tolist() == [0, 103]


VCF = """##fileformat=VCFv4.2
##contig=<ID=chr1>
#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO
chr1\t2\t.\tC\tT\t.\tPASS\tDP=9
chr1\t3\trs1\tGT\tG,GTT,<DEL>\t50\tPASS\t.
chr2\t1\t.\ta\tc,*\t.\t.\t.\tGT\t0/1
chrUn\t5\t.\tA\tG,C\t.\t.\t.
chr2\t4\t.\tG\tG]chr1:5]\t.\t.\t.
chr2\t4\t.\tG\t.\t.\t.\t.

chr1\t7\t.\tN\tA\t.\t.\t.
"""


@pytest.mark.parametrize("gz", [False, True])
def test_read_vcf(tmp_path, gz):
    from crbm_amd import readVcf
    path = str(tmp_path / ("v.vcf.gz" if gz else "v.vcf"))
    with (gzip.open(path, "wt") if gz else open(path, "w")) as f:
        f.write(VCF)
    v = readVcf(path, ["chr1", "chr2"])
    assert v["seq"].tolist() == [0, 0, 0, 1, 0] and v["seq"].dtype == np.int64
    assert v["pos"].tolist() == [1, 2, 2, 0, 6] and v["pos"].dtype == np.int64
    assert v["ref"] == ["C", "GT", "GT", "a", "N"] and v["alt"] == ["T", "G", "GTT", "c", "A"]
    assert v["line"].tolist() == [4, 5, 5, 6, 11]
    assert v["skipped"] == {"symbolic": 3, "breakend": 1, "unknown_contig": 2}
    with open(str(tmp_path / "bad.vcf"), "w") as f:
        f.write("chr1\tx\t.\tA\tC\n")
    with pytest.raises(ValueError, match="line 1: POS is not an integer"):
        readVcf(str(tmp_path / "bad.vcf"), ["chr1"])


def test_read_vcf_feeds_allele_effects(tmp_path, monkeypatch):
    from crbm_amd import CRBM, readVcf, seqsToStream
    stream, off, names = seqsToStream(["ACGTACNA", "ATTG"], ["chr1", "chr2"])
    path = str(tmp_path / "v.vcf")
    with open(path, "w") as f:
        f.write(VCF)
    v = readVcf(path, names)
    m = CRBM(3, 4)
    monkeypatch.setattr(m, "_h", lambda: None)
    calls = _recording(m, monkeypatch)
    out = m.alleleEffects(stream, v["pos"], v["ref"], v["alt"], offsets=off, seq=v["seq"])
    # C>T at 1; GT>G: T deleted at 3; GT>GTT: T inserted at 4 (prefix GT goes first); a>c at 9 + 0; N>A: a span on a code 4
    assert calls[0][1:] == ([1, 3, 4, 9], [1, 1, 0, 1], ["T", "", "T", "C"])
    assert out["dfe"].tolist() == [101, 103, 104, 109, 0]
