"""CPU-only tests of the mutagenesis surface: the three crbm_mutagenesis* entry points in the header, the ctypes table
and the built library (ABI 5 in all three), and the host-side argument checks of CRBM.mutagenesis /
CRBM.pseudoLogLikelihood, which fire before any C call."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("crbm_mutagenesis", "crbm_mutagenesis_codes", "crbm_mutagenesis_resident")


def test_mutagenesis_entry_points_are_declared_bound_and_exported():
    import ctypes
    from crbm_amd import _lib
    header = open(os.path.join(ROOT, "include", "crbm_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in ENTRIES:
        assert re.search(r"\bint %s\(" % name, code), name
        assert name in _lib.SIGNATURES
    assert "convRBM.py:657-676" in header[header.index("in-silico mutagenesis"):header.index("int crbm_mutagenesis(")]
    assert int(re.search(r"#define CRBM_AMD_ABI_VERSION (\d+)", header).group(1)) == _lib.ABI_VERSION == 5
    F, U8P, I32, H = _lib._F, _lib._U8P, _lib._I32, _lib._H
    assert _lib.SIGNATURES["crbm_mutagenesis"] == (I32, [H, F, I32, I32, F, F])
    assert _lib.SIGNATURES["crbm_mutagenesis_codes"] == (I32, [H, U8P, I32, I32, F, F])
    assert _lib.SIGNATURES["crbm_mutagenesis_resident"] == (I32, [H, I32, I32, F, F])
    lib = _lib.load()
    assert lib.crbm_abi_version() == 5
    for name in ENTRIES:
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    # the route of the last call is the last field of crbm_launch_info on both sides
    assert _lib.CrbmLaunchInfo._fields_[-1][0] == "mutagenesis_route"
    fields = re.search(r"typedef struct crbm_launch_info \{(.*?)\} crbm_launch_info;", code, flags=re.S).group(1)
    assert len(re.findall(r"\b\w+\s*[,;]", fields)) == len(_lib.CrbmLaunchInfo._fields_)
    assert ctypes.sizeof(_lib.CrbmLaunchInfo) == 4 * len(_lib.CrbmLaunchInfo._fields_)


def test_null_handle_is_refused_by_the_library():
    """(dfe == pll == NULL and L < motif_length need a handle: tests/test_gpu_mutagenesis.py)"""
    from crbm_amd import _lib
    lib = _lib.load()
    out = np.zeros(4, np.float32)
    assert lib.crbm_mutagenesis_resident(None, 0, 1, _lib.fptr(out), None) == _lib.ERR_INVALID


@pytest.mark.parametrize("method", ["mutagenesis", "pseudoLogLikelihood"])
def test_mutagenesis_calls_refuse_bad_arguments_before_the_c_side(monkeypatch, method):
    from crbm_amd import CRBM
    m = CRBM(3, 4, batchsize=8, fantasy_hidden_len=10)
    monkeypatch.setattr(m, "_h", lambda: None)           # no GPU here: the checks must fire before any call
    monkeypatch.setattr(m, "_call", lambda *a: (_ for _ in ()).throw(AssertionError("reached the library")))
    f = getattr(m, method)
    with pytest.raises(Exception, match="expected a one-hot array"):
        f(np.zeros((2, 4, 20), dtype=np.float32))           # wrong rank
    with pytest.raises(Exception, match="expected a one-hot array"):
        f(np.zeros((2, 1, 3, 20), dtype=np.float32))        # wrong alphabet
    with pytest.raises(ValueError, match="shorter than motif_length"):
        f(np.zeros((2, 3), dtype=np.uint8))
    with pytest.raises(ValueError, match="shorter than motif_length"):
        f(np.zeros((2, 1, 4, 3), dtype=np.float32))
