"""CPU-only tests of the record-summary surface: the declaration of crbm_scan_records_codes and its refusal of a null
handle, CRBM.recordSummary's argument checks (all before the C side) and its cutting of a stream into pieces: at
record boundaries, within _SCAN_MAX letters and within the accumulator budget, rows concatenated in order."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_abi_declares_the_record_entry_point():
    import crbm_amd
    from crbm_amd import _lib
    header = open(os.path.join(ROOT, "include", "crbm_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    decl = re.search(r"\bint crbm_scan_records_codes\((.*?)\);", code, flags=re.S)
    assert decl, "crbm_scan_records_codes is not declared"
    assert [a.strip() for a in decl.group(1).split(",")] == [
        "crbm_handle* h", "const uint8_t* codes", "int64_t T", "const int64_t* rec_start", "int64_t nrec", "int64_t* windows",
        "int64_t* letters", "float* fe", "float* fe_per_motif", "int32_t* best_start", "int32_t* best_strand", "float* best_prob",
        "double* unit"]
    doc = header[header.index("record summaries"):header.index("int crbm_scan_records_codes(")]
    for word in ("rec_start", "T + 1", "fixed point", "2^62", "NOT added", "smaller start", "CRBM_ERR_INVALID", "same bits"):
        assert word in doc, word
    assert re.search(r"#define\s+CRBM_AMD_ABI_VERSION\s+5\b", header)          # additive: the version stays
    lib = _lib.load()
    assert lib.crbm_scan_records_codes.argtypes == _lib.SIGNATURES["crbm_scan_records_codes"][1]
    codes = np.zeros(8, np.uint8)
    rec = np.array([0, 9], np.int64)
    windows = np.zeros(1, np.int64)
    assert lib.crbm_scan_records_codes(None, codes.ctypes.data_as(_lib._U8P), 8, rec.ctypes.data_as(_lib._I64P), 1,
                                       windows.ctypes.data_as(_lib._I64P), None, None, None, None, None, None, None) == _lib.ERR_INVALID
    assert hasattr(crbm_amd.CRBM, "recordSummary")
    assert "NOT added" in crbm_amd.CRBM.recordSummary.__doc__


def _model(monkeypatch):
    """the stub of tests/test_scan_host.py: no GPU here, the checks must fire before any call"""
    from crbm_amd import CRBM
    m = CRBM(3, 4, batchsize=8, fantasy_hidden_len=10, seed=1)
    monkeypatch.setattr(m, "_h", lambda: None)
    monkeypatch.setattr(m, "_call", lambda *a: (_ for _ in ()).throw(AssertionError("reached the library")))
    return m


def test_record_summary_refuses_bad_arguments_before_the_c_side(monkeypatch):
    m = _model(monkeypatch)
    good = np.array([0, 1, 2, 3, 4, 0, 1, 2, 3], np.uint8)
    with pytest.raises(ValueError, match="offsets is required"):
        m.recordSummary(good, None)
    with pytest.raises(TypeError):
        m.recordSummary(good)
    with pytest.raises(ValueError, match="uint8"):
        m.recordSummary(good.astype(np.int32), [0, 10])
    with pytest.raises(ValueError, match="one-dimensional"):
        m.recordSummary(good.reshape(3, 3), [0, 10])
    with pytest.raises(ValueError, match="0..4"):
        m.recordSummary(np.array([0, 1, 5, 2], np.uint8), [0, 5])
    with pytest.raises(ValueError, match="start at 0 and ascend"):
        m.recordSummary(good, [1, 5, 10])
    with pytest.raises(ValueError, match="start at 0 and ascend"):
        m.recordSummary(good, [0, 5, 5, 10])
    with pytest.raises(ValueError, match="last entry"):
        m.recordSummary(good, [0, 5, 9])
    with pytest.raises(ValueError, match="separated by a code 4"):
        m.recordSummary(good, [0, 4, 10])
    with pytest.raises(ValueError, match="no records, but letters"):
        m.recordSummary(good, [0])
    with pytest.raises(ValueError, match="1-D integer"):
        m.recordSummary(good, [0.0, 10.0])
    with pytest.raises(AssertionError, match="reached the library"):      # and a good call gets that far
        m.recordSummary(good, [0, 5, 10])
    with pytest.raises(AssertionError, match="reached the library"):
        m.recordSummary(good, [0, 10])


def _fake(calls):
    def fake(piece, rec_start):                                # letters as "windows", the piece's first code as fe
        assert rec_start[0] == 0 and rec_start[-1] == (piece.size + 1 if rec_start.size > 1 else 0) and rec_start.dtype == np.int64 and rec_start.flags.c_contiguous
        R = rec_start.size - 1
        calls.append((piece.size, R))
        rows = [piece[rec_start[r]:rec_start[r + 1] - 1] for r in range(R)]
        return {"windows": np.array([(x < 4).sum() for x in rows], np.int64), "letters": np.zeros((R, 4), np.int64),
                "per_motif": np.zeros((R, 3), np.float32), "fe": np.array([x[0] if x.size else -1 for x in rows], np.float32),
                "start": np.zeros((R, 3), np.int32), "strand": np.ones((R, 3), np.int32), "prob": np.zeros((R, 3), np.float32),
                "unit": 0.25}
    return fake


def test_record_summary_cuts_at_record_boundaries_and_concatenates(monkeypatch):
    from crbm_amd import CRBM, seqsToStream
    m = CRBM(3, 4, batchsize=8, fantasy_hidden_len=10, seed=1)
    seqs = ["ACGTA", "CCCCC", "GG", "", "TTTTNTTT", "ACGTACGTACG"]
    stream, offsets, _ = seqsToStream(seqs)
    calls = []
    monkeypatch.setattr(m, "_records_call", _fake(calls))
    monkeypatch.delenv("CRBM_SLAB_BYTES", raising=False)
    out = m.recordSummary(stream, offsets)
    assert calls == [(stream.size, 6)]
    assert out["windows"].tolist() == [5, 5, 2, 0, 7, 11] and out["fe"].tolist() == [0, 1, 2, -1, 3, 0]
    assert out["strand"].dtype == np.int8 and out["unit"] == 0.25 and out["per_motif"].shape == (6, 3)
    monkeypatch.setattr(CRBM, "_SCAN_MAX", 12)                 # letters: pieces of at most 12, whole records
    del calls[:]
    cut = m.recordSummary(stream, offsets)
    assert calls == [(11, 2), (12, 3), (11, 1)]
    for k in ("windows", "fe", "strand"):
        assert np.array_equal(cut[k], out[k])
    monkeypatch.setattr(CRBM, "_SCAN_MAX", 10)
    with pytest.raises(ValueError, match="cannot be scanned"):
        m.recordSummary(stream, offsets)


def test_record_summary_keeps_the_accumulators_within_the_slab_budget(monkeypatch):
    """a piece's device accumulators take records * (16 K + 40) bytes: K = 3 gives 88 per record"""
    from crbm_amd import CRBM, seqsToStream
    m = CRBM(3, 4, batchsize=8, fantasy_hidden_len=10, seed=1)
    stream, offsets, _ = seqsToStream(["ACGTA", "CCCCC", "GG", "", "TTTTNTTT", "ACGTACGTACG", "A"])
    calls = []
    monkeypatch.setattr(m, "_records_call", _fake(calls))
    monkeypatch.setenv("CRBM_SLAB_BYTES", str(88 * 3 + 87))    # three records a piece
    out = m.recordSummary(stream, offsets)
    assert [r for _, r in calls] == [3, 3, 1] and sum(t for t, _ in calls) + 2 == stream.size
    assert out["windows"].tolist() == [5, 5, 2, 0, 7, 11, 1]
    del calls[:]
    monkeypatch.setenv("CRBM_SLAB_BYTES", "1")                 # never fewer than one record
    assert m.recordSummary(stream, offsets)["windows"].tolist() == [5, 5, 2, 0, 7, 11, 1] and [r for _, r in calls] == [1] * 7
    del calls[:]
    monkeypatch.setenv("CRBM_SLAB_BYTES", str(88 * 2))         # both limits at once
    monkeypatch.setattr(CRBM, "_SCAN_MAX", 12)
    assert m.recordSummary(stream, offsets)["windows"].tolist() == [5, 5, 2, 0, 7, 11, 1]
    assert calls == [(11, 2), (3, 2), (8, 1), (11, 1), (1, 1)]     # 12 letters cut [2 | 3 | 1 | 1] records, 2 records cut the 3
    del calls[:]
    empty = m.recordSummary(np.zeros(0, np.uint8), [0])        # no records: one call for the unit, no rows
    assert empty["windows"].shape == (0,) and empty["per_motif"].shape == (0, 3) and calls == [(0, 0)]
