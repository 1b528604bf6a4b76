"""CPU-only tests of the stream-scan surface: the readers sequences.seqsToStream / fastaToStream, crbm_scan_sites_codes
in the header, the ctypes table and the built library (ABI still 5), and the host-side argument checks of
CRBM.scanSites, which fire before any C call."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_readers_keep_gaps_lengths_and_names(tmp_path):
    from crbm_amd import seqsToStream, fastaToStream, readSeqsFromFasta
    seqs = ["ACGTNNACgt", "", "acRYgtSWKMBDHVnT", "AC", "TTTTTTTTTTTTTTTTTTTTT"]       # N runs, an empty record, lower
    stream, offsets, names = seqsToStream(seqs)                                       # case, IUPAC codes, a short record
    assert stream.dtype == np.uint8 and stream.ndim == 1 and offsets.dtype == np.int64
    assert names == ["seq0", "seq1", "seq2", "seq3", "seq4"]
    assert offsets.tolist() == [0, 11, 12, 29, 32, 54]
    assert stream.size == sum(map(len, seqs)) + len(seqs) - 1 == offsets[-1] - 1
    want = {"A": 0, "C": 1, "G": 2, "T": 3}
    for i, s in enumerate(seqs):
        got = stream[offsets[i]:offsets[i + 1] - 1]
        assert got.tolist() == [want.get(ch.upper(), 4) for ch in s]
    assert np.all(stream[offsets[1:-1] - 1] == 4)                                     # exactly one separator between records
    for bad in (["ACGT", "AC-T"], ["ACXT"], ["AC GT"], ["AC\nGT"], ["ACGé"]):
        with pytest.raises(ValueError, match="may only contain"):
            seqsToStream(bad)
    s0, o0, n0 = seqsToStream([])
    assert s0.size == 0 and o0.tolist() == [0] and n0 == []
    s1, o1, _ = seqsToStream(["", ""])
    assert s1.tolist() == [4] and o1.tolist() == [0, 1, 2]
    fa = tmp_path / "x.fa"
    fa.write_text(">chr1 first\nACGTNN\nACgt\n>empty\n>chr2\nacRYgtSWKMBDHVnT\n>short\nAC\n")
    stream2, offsets2, names2 = fastaToStream(str(fa))
    assert names2 == ["chr1", "empty", "chr2", "short"]
    assert np.array_equal(stream2, stream[:offsets[4] - 1]) and offsets2.tolist() == offsets[:5].tolist()
    assert [r.id for r in readSeqsFromFasta(str(fa))] == ["empty", "short"]            # that reader is as it was


def test_entry_point_is_declared_documented_bound_and_exported():
    import ctypes
    import crbm_amd
    from crbm_amd import _lib
    header = open(os.path.join(ROOT, "include", "crbm_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    decl = re.search(r"\bint crbm_scan_sites_codes\((.*?)\);", code, flags=re.S)
    assert decl, "crbm_scan_sites_codes is not declared"
    args = [" ".join(a.split()) for a in decl.group(1).split(",")]
    assert args == ["crbm_handle* h", "const uint8_t* codes", "int64_t T", "float threshold", "int64_t capacity",
                    "crbm_site* sites", "int64_t* count"]
    doc = header[header.index("stream scan"):header.index("int crbm_scan_sites_codes(")]
    for word in ("no letter", "valid", "same bits", "(start, motif, strand)", "exact total", "CRBM_SLAB_BYTES", "2^31 - 1",
                 "CRBM_ERR_INVALID", "pooling", "generic", "alphabet", "stays usable"):
        assert word in doc, word
    assert int(re.search(r"#define CRBM_AMD_ABI_VERSION (\d+)", header).group(1)) == _lib.ABI_VERSION == 5
    assert _lib.SIGNATURES["crbm_scan_sites_codes"] == (
        _lib._I32, [_lib._H, _lib._U8P, _lib._I64, ctypes.c_float, _lib._I64, _lib._SITEP, _lib._I64P])
    lib = _lib.load()
    assert lib.crbm_abi_version() == 5
    assert lib.crbm_scan_sites_codes.argtypes == _lib.SIGNATURES["crbm_scan_sites_codes"][1]
    assert _lib.CrbmLaunchInfo._fields_[-1][0] == "mutagenesis_route" and ctypes.sizeof(_lib.CrbmLaunchInfo) == 4 * 15
    # a null handle is refused without touching a device
    codes = np.zeros(8, np.uint8)
    count = ctypes.c_int64(-1)
    assert lib.crbm_scan_sites_codes(None, codes.ctypes.data_as(_lib._U8P), 8, 0.5, 0, None, ctypes.byref(count)) == _lib.ERR_INVALID
    for name in ("seqsToStream", "fastaToStream"):
        assert hasattr(crbm_amd, name)
    assert hasattr(crbm_amd.CRBM, "scanSites")


def _model(monkeypatch):
    from crbm_amd import CRBM
    m = CRBM(3, 4, batchsize=8, fantasy_hidden_len=10, seed=1)
    monkeypatch.setattr(m, "_h", lambda: None)           # no GPU here: the checks must fire before any call
    monkeypatch.setattr(m, "_call", lambda *a: (_ for _ in ()).throw(AssertionError("reached the library")))
    return m


def test_scan_sites_refuses_bad_arguments_before_the_c_side(monkeypatch):
    m = _model(monkeypatch)
    good = np.array([0, 1, 2, 3, 4, 0, 1, 2, 3], np.uint8)
    with pytest.raises(ValueError, match="uint8"):
        m.scanSites(good.astype(np.int32))
    with pytest.raises(ValueError, match="uint8"):
        m.scanSites("ACGT")
    with pytest.raises(ValueError, match="one-dimensional"):
        m.scanSites(good.reshape(3, 3))
    with pytest.raises(ValueError, match="0..4"):
        m.scanSites(np.array([0, 1, 5, 2], np.uint8))
    for t in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="threshold must lie"):
            m.scanSites(good, t)
    with pytest.raises(ValueError, match="start at 0 and ascend"):
        m.scanSites(good, offsets=[1, 5, 10])
    with pytest.raises(ValueError, match="start at 0 and ascend"):
        m.scanSites(good, offsets=[0, 5, 5, 10])
    with pytest.raises(ValueError, match="do not fit the stream"):
        m.scanSites(good, offsets=[0, 5, 9])
    with pytest.raises(ValueError, match="separated by a code 4"):
        m.scanSites(good, offsets=[0, 4, 10])
    with pytest.raises(ValueError, match="1-D integer"):
        m.scanSites(good, offsets=[0.0, 5.0, 10.0])
    with pytest.raises(AssertionError, match="reached the library"):      # and a good call gets that far
        m.scanSites(good, 0.5, offsets=[0, 5, 10])
    with pytest.raises(AssertionError, match="reached the library"):
        m.scanSites(good)


def test_scan_sites_cuts_long_streams_at_record_boundaries_and_maps_records(monkeypatch):
    """scanSites over a C limit of 12 letters per call: pieces end at record boundaries, records come back with the
    record index and record-relative starts, in (seq, start, motif, strand) order"""
    from crbm_amd import CRBM, seqsToStream
    from crbm_amd.crbm import _RAW_SITE
    m = CRBM(3, 4, batchsize=8, fantasy_hidden_len=10, seed=1)
    stream, offsets, _ = seqsToStream(["ACGTA", "CCCCC", "GG", "TTTTTTTT", "ACGTACGTACG"])
    monkeypatch.setattr(CRBM, "_SCAN_MAX", 12)
    pieces = []

    def fake(piece, t):                                   # a "site" at every letter: motif 0, start = position in the piece
        assert piece.size <= 12
        pieces.append(piece.copy())
        pos = np.flatnonzero(piece < 4)
        raw = np.zeros(pos.size, _RAW_SITE)
        raw["start"], raw["strand"], raw["prob"] = pos, 1, 0.75
        return raw
    monkeypatch.setattr(m, "_scan_call", fake)
    sites = m.scanSites(stream, 0.5, offsets=offsets)
    assert [p.size for p in pieces] == [11, 11, 11]       # records 0+1, 2+3, 4: no piece ends inside a record
    assert sites.size == int((stream < 4).sum())
    want = [(i, p) for i, n in enumerate((5, 5, 2, 8, 11)) for p in range(n)]
    assert list(zip(sites["seq"].tolist(), sites["start"].tolist())) == want
    flat = m.scanSites(stream[:11], 0.5)                  # without offsets: stream positions, seq 0
    assert np.all(flat["seq"] == 0) and flat["start"].tolist() == [0, 1, 2, 3, 4, 6, 7, 8, 9, 10]
    with pytest.raises(ValueError, match="needs offsets"):
        m.scanSites(stream, 0.5)
    with pytest.raises(ValueError, match="cannot be scanned"):
        m.scanSites(seqsToStream(["A" * 13])[0], 0.5, offsets=[0, 14])
