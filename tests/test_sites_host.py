"""CPU-only tests of the motif-site surface: utils.saveSites (BED6 and tab), the host-side argument checks of
CRBM.motifSites / motifBestSites (before any C call), and the three crbm_motif_sites* entry points in the header, the
ctypes table and the built library."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("crbm_motif_sites", "crbm_motif_sites_codes", "crbm_motif_sites_resident")


def _sites():
    from crbm_amd import CRBM
    s = np.zeros(3, dtype=CRBM.SITE_DTYPE)
    s["seq"], s["motif"], s["start"], s["strand"] = [0, 0, 2], [0, 2, 1], [5, 0, 17], [1, -1, 0]
    s["prob"] = [0.9, 0.5, 0.75]
    return s


def test_site_dtype():
    from crbm_amd import CRBM
    assert CRBM.SITE_DTYPE.names == ("seq", "motif", "start", "strand", "prob")
    assert [CRBM.SITE_DTYPE[f].str for f in CRBM.SITE_DTYPE.names] == ["<i4", "<i4", "<i4", "|i1", "<f4"]


def test_save_sites_bed_and_tab(tmp_path):
    from crbm_amd import CRBM, saveSites
    from crbm_amd.utils import saveSites as saveSites2
    assert saveSites is saveSites2
    m = CRBM(3, 6, doublestranded=True)
    fn = str(tmp_path / "s.bed")
    saveSites(m, _sites(), fn)
    assert open(fn).read() == ("seq0\t5\t11\tmot1\t0.9\t+\n"
                               "seq0\t0\t6\tmot3\t0.5\t-\n"
                               "seq2\t17\t23\tmot2\t0.75\t.\n")
    saveSites(m, _sites(), fn, names=["chr1:100-300", "b", "peak_7"])
    assert open(fn).read().splitlines()[2] == "peak_7\t17\t23\tmot2\t0.75\t."
    fn = str(tmp_path / "s.tab")
    saveSites(m, _sites(), fn, names=["x", "y", "z"], fformat="tab")
    lines = open(fn).read().splitlines()
    assert lines[0] == "chrom\tstart\tend\tmotif\tprob\tstrand"
    assert lines[1:] == ["x\t5\t11\tmot1\t0.9\t+", "x\t0\t6\tmot3\t0.5\t-", "z\t17\t23\tmot2\t0.75\t."]
    saveSites(m, _sites()[:0], fn)
    assert open(fn).read() == ""
    with pytest.raises(ValueError):
        saveSites(m, _sites(), fn, fformat="gff")


def test_site_calls_refuse_bad_arguments_before_the_c_side(monkeypatch):
    from crbm_amd import CRBM
    m = CRBM(3, 4, batchsize=8, fantasy_hidden_len=10)
    monkeypatch.setattr(m, "_h", lambda: None)           # no GPU here: the checks must fire before any call
    monkeypatch.setattr(m, "_call", lambda *a: (_ for _ in ()).throw(AssertionError("reached the library")))
    codes = np.zeros((2, 20), dtype=np.uint8)
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="threshold"):
            m.motifSites(codes, bad)
    with pytest.raises(Exception, match="expected a one-hot array"):
        m.motifSites(np.zeros((2, 4, 20), dtype=np.float32), 0.5)
    with pytest.raises(Exception, match="expected a one-hot array"):
        m.motifBestSites(np.zeros((2, 1, 3, 20), dtype=np.float32))
    with pytest.raises(ValueError, match="shorter than motif_length"):
        m.motifSites(np.zeros((2, 3), dtype=np.uint8), 0.5)
    with pytest.raises(ValueError, match="shorter than motif_length"):
        m.motifBestSites(np.zeros((2, 1, 4, 3), dtype=np.float32))


def test_site_entry_points_are_declared_bound_and_exported():
    from crbm_amd import _lib
    header = open(os.path.join(ROOT, "include", "crbm_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in ENTRIES:
        assert re.search(r"\bint %s\(" % name, code), name
        assert name in _lib.SIGNATURES
    assert re.search(r"typedef struct crbm_site \{", code)
    assert int(re.search(r"#define CRBM_AMD_ABI_VERSION (\d+)", header).group(1)) == _lib.ABI_VERSION >= 4
    import ctypes
    assert ctypes.sizeof(_lib.CrbmSite) == 20
    lib = _lib.load()
    for name in ENTRIES:
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
