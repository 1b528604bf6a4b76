"""CPU-only tests of the annealed-importance-sampling surface: crbm_ais in the header, the ctypes table and the built
library (ABI still 5, crbm_launch_info unchanged), the sampler kinds on both sides, and the host-side argument checks
of CRBM.logPartition / CRBM.logLikelihood, which fire before any C call."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entry_point_is_declared_documented_bound_and_exported():
    import ctypes
    from crbm_amd import _lib
    header = open(os.path.join(ROOT, "include", "crbm_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    decl = re.search(r"\bint crbm_ais\((.*?)\);", code, flags=re.S)
    assert decl, "crbm_ais is not declared"
    args = [" ".join(a.split()) for a in decl.group(1).split(",")]
    assert args == ["crbm_handle* h", "int32_t L", "int32_t runs", "uint32_t run_offset", "const float* betas", "int32_t nbetas",
                    "int32_t t0", "int32_t t1", "const float* base_c", "uint64_t seed", "uint8_t* state", "float* logw"]
    doc = header[header.index("annealed importance sampling"):header.index("int crbm_ais(")]
    for word in ("log p*_beta", "run_offset", "CRBM_AIS_STEPS", "same bits", "CRBM_ERR_INVALID", "pooling", "generic", "alphabet"):
        assert word in doc, word
    assert int(re.search(r"#define CRBM_AMD_ABI_VERSION (\d+)", header).group(1)) == _lib.ABI_VERSION == 5
    H, F, I32, U32, U64, U8P = _lib._H, _lib._F, _lib._I32, _lib._U32, _lib._U64, _lib._U8P
    assert _lib.SIGNATURES["crbm_ais"] == (I32, [H, I32, I32, U32, F, I32, I32, I32, F, U64, U8P, F])
    lib = _lib.load()
    assert lib.crbm_abi_version() == 5
    assert lib.crbm_ais.argtypes == _lib.SIGNATURES["crbm_ais"][1]
    # crbm_launch_info keeps its layout
    assert _lib.CrbmLaunchInfo._fields_[-1][0] == "mutagenesis_route" and ctypes.sizeof(_lib.CrbmLaunchInfo) == 4 * 15
    # a null handle is refused without touching a device
    lw = np.zeros(2, np.float32)
    b = np.array([0, 1], np.float32)
    assert lib.crbm_ais(None, 8, 2, 0, _lib.fptr(b), 2, 0, 1, None, 0, None, _lib.fptr(lw)) == _lib.ERR_INVALID


def test_sampler_kinds_agree_between_kernels_and_yardstick():
    from tests import ais_reference as ref
    layout = open(os.path.join(ROOT, "crbm_amd", "csrc", "crbm_layout.h")).read()
    assert int(re.search(r"KIND_AIS_H = (\d+)", layout).group(1)) == ref.KIND_AIS_H == 6
    assert int(re.search(r"KIND_AIS_V = (\d+)", layout).group(1)) == ref.KIND_AIS_V == 7


def _model(monkeypatch):
    from crbm_amd import CRBM
    m = CRBM(3, 4, batchsize=8, fantasy_hidden_len=10, seed=1)
    monkeypatch.setattr(m, "_h", lambda: None)           # no GPU here: the checks must fire before any call
    monkeypatch.setattr(m, "_call", lambda *a: (_ for _ in ()).throw(AssertionError("reached the library")))
    return m


def test_log_partition_refuses_bad_arguments_before_the_c_side(monkeypatch):
    m = _model(monkeypatch)
    with pytest.raises(ValueError, match="runs must be at least 1"):
        m.logPartition(20, runs=0)
    with pytest.raises(ValueError, match="shorter than motif_length"):
        m.logPartition(3)
    with pytest.raises(ValueError, match="at least 1 temperature"):
        m.logPartition(20, betas=0)
    with pytest.raises(ValueError, match="start at 0 and end at 1"):
        m.logPartition(20, betas=[0.1, 0.5, 1.0])
    with pytest.raises(ValueError, match="start at 0 and end at 1"):
        m.logPartition(20, betas=[0.0, 0.5, 0.9])
    with pytest.raises(ValueError, match="start at 0 and end at 1"):
        m.logPartition(20, betas=[0.0, np.nan, 1.0])
    with pytest.raises(ValueError, match="must not decrease"):
        m.logPartition(20, betas=[0.0, 0.6, 0.5, 1.0])
    with pytest.raises(ValueError, match="at least two values"):
        m.logPartition(20, betas=[1.0])
    with pytest.raises(ValueError, match="base must be None"):
        m.logPartition(20, base=np.zeros(3))
    with pytest.raises(ValueError, match="base must be None"):
        m.logPartition(20, base=np.zeros((2, 1, 5, 9), np.float32))
    with pytest.raises(ValueError, match="base must be finite"):
        m.logPartition(20, base=[0.0, np.inf, 0.0, 0.0])
    with pytest.raises(ValueError, match="letter code outside"):
        m.logPartition(20, base=np.full((2, 9), 4, np.uint8))
    with pytest.raises(AssertionError, match="reached the library"):      # and a good call gets that far
        m.logPartition(20, runs=4, betas=[0.0, 0.5, 1.0], base=np.zeros((1, 4)))


def test_log_likelihood_refuses_bad_arguments_before_the_c_side(monkeypatch):
    m = _model(monkeypatch)
    with pytest.raises(Exception, match="expected a one-hot array"):
        m.logLikelihood(np.zeros((2, 4, 20), dtype=np.float32), logZ=1.0)
    with pytest.raises(ValueError, match="shorter than motif_length"):
        m.logLikelihood(np.zeros((2, 3), dtype=np.uint8), logZ=1.0)
    with pytest.raises(TypeError, match="unexpected keyword"):
        m.logLikelihood(np.zeros((2, 9), dtype=np.uint8), logZ=1.0, runs=5)
    with pytest.raises(ValueError, match="runs must be at least 1"):
        m.logLikelihood(np.zeros((2, 9), dtype=np.uint8), runs=0)


def test_base_rate_bias_from_data():
    from crbm_amd import CRBM
    m = CRBM(3, 4, batchsize=8, fantasy_hidden_len=10, seed=1)
    codes = np.array([[0, 0, 1, 3], [0, 2, 0, 0]], np.uint8)
    want = np.log((np.array([5, 1, 1, 1]) + 1.0) / (8 + 4)).astype(np.float32)
    np.testing.assert_array_equal(m._ais_base(codes), want)
    onehot = np.ascontiguousarray(np.eye(4, dtype=np.float32)[codes].transpose(0, 2, 1)[:, None])
    np.testing.assert_array_equal(m._ais_base(onehot), want)
    np.testing.assert_array_equal(m._ais_base(np.array([[0.1, 0.2, 0.3, 0.4]])), np.array([0.1, 0.2, 0.3, 0.4], np.float32))
    assert m._ais_base(None) is None
    np.testing.assert_array_equal(m._ais_ladder(4), np.array([0, 0.25, 0.5, 0.75, 1], np.float32))
