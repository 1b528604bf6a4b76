"""CPU-only tests of the motif comparison's host side (crbm_amd/motifs.py, utils.saveMatches): header, SIGNATURES and
exported symbols agree and the ABI version stays 5; readMotifs on every format it takes, written here into tmp_path; the
saveMotifs -> readMotifs round trip within the two decimals of the text; malformed files with the file and line in the
message; quantised() against tests/compare_reference.py; Benjamini-Hochberg against a hand computation; matches, best,
save / load and saveMatches on a hand-made comparison; every ValueError."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import compare_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_abi_declares_the_entry_points():
    import crbm_amd
    from crbm_amd import _lib, motifs
    header = open(os.path.join(ROOT, "include", "crbm_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    want = {
        "crbm_motif_compare": ["crbm_handle* h", "const uint16_t* qcols", "const int32_t* qstart", "int32_t K", "const uint16_t* tcols",
                               "const int32_t* tstart", "int32_t N", "int32_t bins", "int32_t both", "int32_t min_overlap", "double invC",
                               "double* p_min", "int32_t* offset", "int8_t* strand", "int32_t* overlap", "int32_t* n_off"],
        "crbm_motif_compare_null": ["crbm_handle* h", "const uint16_t* qcols", "int32_t m", "const uint16_t* tcols", "const int32_t* tstart",
                                    "int32_t N", "int32_t bins", "int32_t both", "double invC", "uint32_t* counts", "double* tail"],
        "crbm_compare_ms": ["crbm_handle* h", "float* ms", "float* stage_ms"],
    }
    lib = _lib.load()
    for name, args in want.items():
        decl = re.search(r"\bint %s\((.*?)\);" % name, code, flags=re.S)
        assert decl, name + " is not declared"
        assert [" ".join(a.split()) for a in decl.group(1).split(",")] == args
        res, argtypes = _lib.SIGNATURES[name]
        assert res is ctypes.c_int32 and len(argtypes) == len(args) and getattr(lib, name).argtypes == argtypes
    assert re.search(r"#define\s+CRBM_AMD_ABI_VERSION\s+5\b", header) and _lib.ABI_VERSION == 5      # additive: the version stays
    doc = header[header.index("Motif comparison"):header.index("int crbm_motif_compare(")]
    for word in ("CRBM_COMPARE_TILE", "CRBM_COMPARE_BYTES", "CRBM_ERR_INVALID", "2^31 - 1", "ascending y", "strand +1", "4096"):
        assert word in doc, word
    assert lib.crbm_motif_compare(None, *([None] * 2), 1, None, None, 1, 100, 1, 1, 0.5, *([None] * 5)) == _lib.ERR_INVALID
    assert lib.crbm_compare_ms(None, None, None) == _lib.ERR_INVALID
    for name in ("MotifSet", "MotifComparison", "readMotifs", "compareMotifs", "saveMatches", "motifs"):
        assert hasattr(crbm_amd, name), name
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in want:
        assert name in integration
    assert '"crbm_compare.h"' in open(os.path.join(ROOT, "crbm_amd", "csrc", "build.py")).read()
    assert "crbm_compare.h" not in open(os.path.join(ROOT, "crbm_amd", "csrc", "crbm_jit.h")).read()    # not part of the per-model source
    source = open(os.path.join(ROOT, "crbm_amd", "csrc", "crbm_compare.h")).read()
    assert re.search(r"TILE_DEFAULT\s*=\s*%d\b" % motifs.TARGET_TILE, source) and re.search(r"MAX_WIDTH\s*=\s*%d\b" % motifs.MAX_WIDTH, source)


JASPAR = """>MA0001.1 AGL3
A  [ 0  3 79 40 ]
C  [94 75  4  3 ]
G  [ 1  0  3  4 ]
T  [ 2 19 11 50 ]
>MA0002.1
A [0.25 0.5]
C [0.25 0.0]
G [0.25 0.0]
T [0.25 0.5]
"""
MEME = """MEME version 4

ALPHABET= ACGT

strands: + -

Background letter frequencies
A 0.25 C 0.25 G 0.25 T 0.25

MOTIF first alt
letter-probability matrix: alength= 4 w= 3 nsites= 20 E= 0
 0.1 0.2 0.3 0.4
 1.0 0.0 0.0 0.0
 0.25 0.25 0.25 0.25
URL http://somewhere

MOTIF second
letter-probability matrix: alength= 4 w= 1
0 0 2 2
"""


def test_read_every_format(tmp_path):
    from crbm_amd import readMotifs, MotifSet
    (tmp_path / "a.jaspar").write_text(JASPAR)
    (tmp_path / "b.meme").write_text(MEME)
    (tmp_path / "c.pfm").write_text("  0.50   0.10\n  0.25   0.20\n  0.25   0.30\n  0.00   0.40\n")
    s = readMotifs(str(tmp_path / "a.jaspar"))
    assert isinstance(s, MotifSet) and len(s) == 2 and s.names == ["AGL3", "MA0002.1"]
    assert np.allclose(s.matrices[0][:, 0], np.array([0, 94, 1, 2]) / 97.0) and s.matrices[0].shape == (4, 4)
    assert np.array_equal(s.matrices[1], [[0.25, 0.5], [0.25, 0], [0.25, 0], [0.25, 0.5]])
    m = readMotifs(str(tmp_path / "b.meme"))
    assert m.names == ["first", "second"] and m.matrices[0].shape == (4, 3) and m.matrices[1].shape == (4, 1)
    assert np.array_equal(m.matrices[0][:, 0], [0.1, 0.2, 0.3, 0.4]) and np.array_equal(m.matrices[1][:, 0], [0, 0, 0.5, 0.5])
    p = readMotifs(str(tmp_path / "c.pfm"))
    assert p.names == ["c"] and np.allclose(p.matrices[0], [[0.5, 0.1], [0.25, 0.2], [0.25, 0.3], [0.0, 0.4]])
    every = readMotifs(str(tmp_path))                            # a directory: its files in sorted order
    assert every.names == ["AGL3", "MA0002.1", "first", "second", "c"]
    assert readMotifs([str(tmp_path / "c.pfm"), str(tmp_path / "a.jaspar")]).names == ["c", "AGL3", "MA0002.1"]
    ps = readMotifs(str(tmp_path / "a.jaspar"), pseudocount=1.0)
    assert np.allclose(ps.matrices[0][:, 0], (np.array([0, 94, 1, 2]) + 0.25) / 98.0) and np.allclose(ps.matrices[0].sum(axis=0), 1.0)
    name, matrix = every[2]
    assert name == "first" and matrix.shape == (4, 3) and len(every[1:3]) == 2 and every[[4, 0]].names == ["c", "AGL3"]


@pytest.mark.parametrize("fformat", ["jaspar", "pfm"])
def test_save_motifs_round_trip(tmp_path, fformat):
    from crbm_amd import readMotifs, saveMotifs, MotifSet

    class Model(object):
        def getPFMs(self):
            rng = np.random.default_rng(4)
            return [R.dirichlet_motif(rng, w, alpha=1.0) for w in (5, 9, 12)]

    model = Model()
    saveMotifs(model, str(tmp_path / "out"), name="mot", fformat=fformat)
    back = readMotifs(str(tmp_path / "out"))
    own = MotifSet.from_model(model)
    assert own.names == ["mot1", "mot2", "mot3"]
    assert back.names == (own.names if fformat == "jaspar" else ["mot0", "mot1", "mot2"])     # a bare pfm is named after its file
    for a, b in zip(back.matrices, own.matrices):
        assert a.shape == b.shape and np.abs(a - b).max() <= 0.005 * 5 + 1e-12       # two decimals, renormalised over four letters


@pytest.mark.parametrize("text,line,why", [
    (">m\nA [1 2]\nC [1 2]\nG [1 2]\n", 1, "rows, not four"),
    (">m\nA [1 2]\nC [1 2]\nG [1 2]\nT [1 2]\nA [1 2]\n", 6, "four per record"),
    (">m\nA [1 2]\nC [1 2 3]\nG [1 2]\nT [1 2]\n", 1, "ragged"),
    (">m\nA [1 0]\nC [1 0]\nG [1 0]\nT [1 0]\n", 1, "sums to 0"),
    (">m\nA [1 x]\nC [1 0]\nG [1 0]\nT [1 0]\n", 2, "not a number"),
    ("1 2\n1 2\n1 2\n1 2\n1 2\n", 5, "more than four rows"),
    ("MOTIF m\nletter-probability matrix: alength= 4 w= 2\n0.5 0.5 0 0\n0.5 0.5 0\n", 4, "ragged"),
    ("MOTIF m\nletter-probability matrix: alength= 4 w= 3\n0.5 0.5 0 0\n0.5 0.5 0 0\n", 1, "w= 3"),
    ("MOTIF m\nletter-probability matrix: alength= 4 w= 1\n0 0 0 0\n", 1, "sums to 0"),
    ("MOTIF m\nletter-probability matrix: alength= 20 w= 1\n" + "0.05 " * 20 + "\n", 2, "alength"),
    ("", 1, "no motif"),
])
def test_malformed_files_name_the_file_and_line(tmp_path, text, line, why):
    from crbm_amd import readMotifs
    path = tmp_path / "bad.txt"
    path.write_text(text)
    with pytest.raises(ValueError) as e:
        readMotifs(str(path))
    assert "bad.txt, line %d:" % line in str(e.value) and why in str(e.value), str(e.value)


def test_quantised_is_the_references():
    from crbm_amd import MotifSet
    rng = np.random.default_rng(2)
    mats = [R.dirichlet_motif(rng, w) for w in (1, 7, 64)]
    s = MotifSet(["a", "b", "c"], mats)
    cols, start = s.quantised()
    assert cols.dtype == np.uint16 and start.dtype == np.int32 and start.tolist() == [0, 1, 8, 72] and cols.shape == (72, 4)
    assert cols.flags["C_CONTIGUOUS"] and s.widths.tolist() == [1, 7, 64] and len(s) == 3
    for k, m in enumerate(mats):
        assert np.array_equal(cols[start[k]:start[k + 1]], R.quantise(m))
    rc, _ = s.reverse_complement().quantised()
    for k, m in enumerate(mats):
        assert np.array_equal(rc[start[k]:start[k + 1]], R.reverse_complement(R.quantise(m)))
    edge = MotifSet(["e"], [np.array([[1.0, 0.5 / 4096], [0.0, 1.49 / 4096], [0.0, 0.0], [0.0, 1.0 - 1.99 / 4096]])])
    assert edge.quantised()[0].tolist() == [[4096, 0, 0, 0], [1, 1, 0, 4094]]


def test_benjamini_hochberg_and_derive():
    from crbm_amd import motifs
    p = np.array([[0.01, 0.04, 0.03, 0.5], [0.9, 0.9, 0.2, 1.0]])
    want = [[0.04, 0.04 * 4 / 3, 0.04 * 4 / 3, 0.5], [1.0, 1.0, 0.8, 1.0]]      # row 2: 0.8, 1.2 -> 1, 1.2 -> 1, 1
    assert np.allclose(motifs.benjamini_hochberg(p), want, rtol=1e-15)
    rng = np.random.default_rng(0)
    p_min, n_off = rng.uniform(size=(3, 17)) ** 8, rng.integers(1, 200, size=(3, 17))
    p_min[0, 0], p_min[1, 1] = 1.0, 0.0
    pv, ev, qv = motifs.derive(p_min, n_off)
    rpv, rev, rqv = R.derive(p_min, n_off)
    assert np.array_equal(pv, rpv) and np.array_equal(ev, rev) and np.allclose(qv, np.minimum(rqv, 1.0), rtol=1e-15)
    assert pv[0, 0] == 1.0 and pv[1, 1] == 0.0


def comparison():
    from crbm_amd import MotifComparison
    p_min = np.array([[1e-9, 0.5, 1e-4], [0.2, 1e-12, 1.0]])
    return MotifComparison(["q1", "q2"], ["t1", "t2", "t3"], p_min, [[0, -2, 3], [1, 0, 0]], [[1, -1, 1], [1, 1, -1]],
                           [[6, 4, 5], [7, 8, 2]], [[20, 20, 20], [10, 10, 10]], bins=50, strands="both", min_overlap=2)


def test_matches_best_save_load_and_save_matches(tmp_path):
    from crbm_amd import MotifComparison, saveMatches, motifs
    c = comparison()
    assert c.pvalue.shape == (2, 3) and np.allclose(c.evalue, c.pvalue * 3) and np.all(c.qvalue >= c.pvalue)
    m = c.matches(evalue=1.0)
    assert m.dtype == motifs.MATCH_DTYPE and m["query"].tolist() == [0, 0, 1] and m["target"].tolist() == [0, 2, 1]
    assert m["offset"].tolist() == [0, 3, 0] and m["strand"].tolist() == [1, 1, 1] and m["overlap"].tolist() == [6, 5, 8]
    assert len(c.matches(evalue=10.0)) == 6 and len(c.matches(evalue=0.0)) == 0
    b = c.best()
    assert b["query"].tolist() == [0, 1] and b["target"].tolist() == [0, 1]
    b2 = c.best(n=2)
    assert b2["query"].tolist() == [0, 0, 1, 1] and b2["target"].tolist() == [0, 2, 1, 0] and len(c.best(n=9)) == 6
    c.save(str(tmp_path / "cmp"))
    back = MotifComparison.load(str(tmp_path / "cmp.npz"))
    for f in MotifComparison.FIELDS:
        assert np.array_equal(getattr(back, f), getattr(c, f)) and getattr(back, f).dtype == getattr(c, f).dtype
    assert back.queries == c.queries and back.targets == c.targets and (back.bins, back.strands, back.min_overlap) == (50, "both", 2)
    saveMatches(c, str(tmp_path / "m.tsv"), evalue=1.0)
    lines = (tmp_path / "m.tsv").read_text().splitlines()
    assert lines[0].split("\t") == ["query", "target", "offset", "strand", "overlap", "pvalue", "evalue", "qvalue"]
    assert [l.split("\t")[:5] for l in lines[1:]] == [["q1", "t1", "0", "+", "6"], ["q1", "t3", "3", "+", "5"], ["q2", "t2", "0", "+", "8"]]
    assert float(lines[1].split("\t")[5]) == pytest.approx(c.pvalue[0, 0], rel=1e-5)
    saveMatches(c, str(tmp_path / "all.tsv"))
    assert "-" in [l.split("\t")[3] for l in (tmp_path / "all.tsv").read_text().splitlines()[1:]]


def test_value_errors():
    from crbm_amd import MotifSet, MotifComparison, compareMotifs, readMotifs
    good = np.full((4, 3), 0.25)
    for names, mats in ((["a"], [np.full((4, 65), 0.25)]), ([], []), (["a"], [np.full((3, 4), 1 / 3.0)]), (["a"], [good * 1.1]),
                        (["a"], [np.full((4, 0), 0.25)]), (["a", "b"], [good]), (["a"], [np.where(np.eye(4, 3) > 0, -0.5, 0.5)]),
                        (["a"], [np.full((4, 3), np.nan)]), (["a"], [np.full(4, 0.25)])):
        with pytest.raises(ValueError):
            MotifSet(names, mats)
    s = MotifSet(["a"], [good])
    for kw in (dict(bins=1), dict(bins=257), dict(bins=10.0), dict(bins=True), dict(strands="minus"), dict(strands=None),
               dict(min_overlap=0), dict(min_overlap=1.5), dict(targets=[good]), dict(queries=[good])):
        args = dict(queries=s, targets=s)
        args.update(kw)
        with pytest.raises(ValueError):
            compareMotifs(None, **args)                          # refused before the model is touched
    with pytest.raises(ValueError):
        readMotifs("x", pseudocount=-1.0)
    with pytest.raises(ValueError):
        MotifComparison(["q"], ["t"], np.zeros((1, 2)), np.zeros((1, 1)), np.ones((1, 1)), np.ones((1, 1)), np.ones((1, 1)))
    with pytest.raises(ValueError):
        MotifComparison(["q"], ["t"], *([np.ones((1, 1))] * 5), strands="minus")
