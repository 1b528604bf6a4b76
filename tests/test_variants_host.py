"""CPU-only checks of CRBM.variantEffects (crbm_amd/crbm.py): everything it refuses is refused before the library is
reached -- stream and offsets as scanSites, pos, alt and ref by dtype, shape and range, the ref check with the indices
of the first mismatches, positions outside their record; `seq` / `offsets` map record positions to stream positions;
a long stream is cut at record boundaries, every variant goes to its piece with a position relative to it, and the
outputs come back in the caller's order.  The entry point is declared, documented, bound and exported.  (Chunk
planning lives in crbm_sweep.h: tests/test_emu_variants.py.)"""
import ctypes
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


def test_entry_point_is_declared_documented_bound_and_exported():
    from crbm_amd import _lib
    header = open(os.path.join(ROOT, "include", "crbm_amd.h")).read()
    assert re.search(r"int crbm_variant_effects_codes\(crbm_handle\* h, const uint8_t\* codes, int64_t T, int64_t nvar, "
                     r"const int64_t\* pos,\s+const uint8_t\* alt, float\* dfe, float\* dfe_per_motif, int32_t\* windows\);", header)
    assert "#define CRBM_AMD_ABI_VERSION 5" in header    # additive: the version stays
    res, args = _lib.SIGNATURES["crbm_variant_effects_codes"]
    assert res is ctypes.c_int32 and len(args) == 9 and args[2] is ctypes.c_int64 and args[3] is ctypes.c_int64
    assert args[4] is _lib._I64P and args[5] is _lib._U8P and args[8] is _lib._I32P
    assert hasattr(_lib.load(), "crbm_variant_effects_codes")
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        assert "variantEffects" in open(os.path.join(ROOT, doc)).read(), doc


def test_variant_effects_refuses_bad_arguments_before_the_c_side(monkeypatch):
    m = _model(monkeypatch)
    s = np.array([0, 1, 2, 3, 4, 0, 1, 2, 3, 0], np.uint8)
    ok_pos, ok_alt = np.array([1, 7]), np.array([2, 0], np.uint8)
    with pytest.raises(ValueError, match="uint8"):
        m.variantEffects(s.astype(np.int32), ok_pos, ok_alt)
    with pytest.raises(ValueError, match="0..4"):
        m.variantEffects(np.array([0, 5], np.uint8), [0], np.array([1], np.uint8))
    with pytest.raises(ValueError, match="pos must be a 1-D integer"):
        m.variantEffects(s, np.array([1.0, 7.0]), ok_alt)
    with pytest.raises(ValueError, match="pos must be a 1-D integer"):
        m.variantEffects(s, np.array([[1, 7]]), ok_alt)
    with pytest.raises(ValueError, match=r"outside the stream at variants \[1\]"):
        m.variantEffects(s, [1, 10], ok_alt)
    with pytest.raises(ValueError, match=r"outside the stream at variants \[0\]"):
        m.variantEffects(s, [-1, 7], ok_alt)
    with pytest.raises(ValueError, match="alt must hold letters"):
        m.variantEffects(s, ok_pos, np.array([2, 4], np.uint8))
    with pytest.raises(ValueError, match="alt must hold letters"):
        m.variantEffects(s, ok_pos, "AN")
    with pytest.raises(ValueError, match="one entry per variant"):
        m.variantEffects(s, ok_pos, "ACG")
    with pytest.raises(ValueError, match="alt must be a uint8 array"):
        m.variantEffects(s, ok_pos, np.array([2, 0], np.int64))
    with pytest.raises(ValueError, match="seq needs the offsets"):
        m.variantEffects(s, ok_pos, ok_alt, seq=[0, 1])
    off = np.array([0, 5, 11])                           # records [0, 4) and [5, 10)
    with pytest.raises(ValueError, match=r"seq must lie in \[0, 2\)"):
        m.variantEffects(s, ok_pos, ok_alt, offsets=off, seq=[0, 2])
    with pytest.raises(ValueError, match="one record index per variant"):
        m.variantEffects(s, ok_pos, ok_alt, offsets=off, seq=[0])
    with pytest.raises(ValueError, match=r"pos outside its record at variants \[0\]"):
        m.variantEffects(s, [4, 1], ok_alt, offsets=off, seq=[0, 1])       # the separator is not part of record 0
    with pytest.raises(ValueError, match=r"ref does not match the stream at 2 of 3 variants, the first at indices \[0, 2\]"):
        m.variantEffects(s, [1, 7, 4], "GAC", ref="AGA")                   # stream: C, G, no letter
    with pytest.raises(ValueError, match="ref must hold one entry"):
        m.variantEffects(s, ok_pos, ok_alt, ref="C")


def test_variant_effects_maps_records_cuts_long_streams_and_restores_the_order(monkeypatch):
    from crbm_amd import CRBM, _lib
    m = CRBM(3, 4)
    monkeypatch.setattr(m, "_h", lambda: None)
    monkeypatch.setattr(CRBM, "_SCAN_MAX", 12)
    recs = [np.array([0, 1, 2, 3, 0, 1], np.uint8), np.array([3, 3, 4, 2], np.uint8), np.array([1, 0, 2, 2, 3, 1, 0], np.uint8)]
    stream = np.concatenate([recs[0], [4], recs[1], [4], recs[2]]).astype(np.uint8)
    off = np.array([0, 7, 12, 20])
    calls = []

    def fake(name, codes, T, nvar, pos, alt, dfe, pm, win):
        assert name == "crbm_variant_effects_codes"
        piece = np.ctypeslib.as_array(codes, (T,)).copy()
        p, a = np.ctypeslib.as_array(pos, (nvar,)).copy(), np.ctypeslib.as_array(alt, (nvar,)).copy()
        calls.append((piece, p, a))
        np.ctypeslib.as_array(dfe, (nvar,))[:] = 100 * len(calls) + p              # the piece and the position inside it
        np.ctypeslib.as_array(pm, (nvar, 3))[:] = a[:, None] + np.arange(3)[None, :]
        np.ctypeslib.as_array(win, (nvar,))[:] = piece[p]
    monkeypatch.setattr(m, "_call", fake)
    seq, pos = np.array([2, 0, 1, 2, 0, 1]), np.array([6, 5, 2, 0, 0, 3])
    out = m.variantEffects(stream, pos, "ACGTAC", offsets=off, seq=seq, ref=np.array([0, 1, 4, 1, 0, 2], np.uint8))
    # pieces of at most 12 letters, cut at record boundaries: records 0 and 1 (stream [0, 11)), then record 2 ([12, 19))
    assert [c[0].tolist() for c in calls] == [stream[:11].tolist(), stream[12:].tolist()]
    assert calls[0][1].tolist() == [5, 9, 0, 10] and calls[1][1].tolist() == [6, 0]
    assert calls[0][2].tolist() == [1, 2, 0, 1] and calls[1][2].tolist() == [0, 3]
    assert out["dfe"].tolist() == [206, 105, 109, 200, 100, 110] and out["dfe"].dtype == np.float32
    assert out["windows"].tolist() == [0, 1, 4, 1, 0, 2] and out["windows"].dtype == np.int32      # the codes under the variants
    assert out["per_motif"].shape == (6, 3) and out["per_motif"][:, 0].tolist() == [0, 1, 2, 3, 0, 1]
    # without seq: stream positions; letters as an array; a variant on the separator between the pieces reaches no piece: zeros
    calls.clear()
    out = m.variantEffects(stream, [11, 3], np.array(["T", "g"]), offsets=off)
    assert len(calls) == 1 and calls[0][1].tolist() == [3] and calls[0][2].tolist() == [2]
    assert out["dfe"].tolist() == [0, 103] and out["windows"].tolist() == [0, 3]
    empty = m.variantEffects(stream, np.zeros(0, np.int64), np.zeros(0, np.uint8), offsets=off)
    assert empty["dfe"].shape == (0,) and empty["per_motif"].shape == (0, 3) and empty["windows"].shape == (0,)
