"""The geometry the host picks for the generic kernels (crbm_plan.h: big_hgv_geom, big_vgh_geom, big_stats_geom,
big_eval_lds, vgh_dense_lds -- the functions crbm_api.hip launches by), read on the CPU through tests/emu/plan_driver.cpp.

  * every case of tests/test_gpu_generic_geometry.py (tests/generic_geom_cases.py) lies in the regime its id names, and
    its launches fit the 160 KB of LDS or are refused as the case expects: a later change to a budget cannot move a case
    out of its regime unnoticed;
  * the regime boundaries sit where the kernels' budgets put them, at 256 compute units: h|v slabs of 32 / 16 / 8 motifs
    at A M = 682 | 683 and 1228 | 1229 (DNA: 170 | 171 and 307 | 308 letters), column slabs of the chain v|h at 128 | 129
    letters (DNA; 8 | 9 for 64 letters, 25 | 26 for 20, 170 | 171 for 3), its chunks at 2048 | 2049 visible positions
    (DNA) and 256 | 257 (other alphabets), statistics chunks at 4096 | 4097 hidden positions, its row stride (8 x 256 / K, at least
    1: one row after the other from 1025 motifs on, the quotient itself gone from 2049), its per-thread slots on DNA at
    256 | 257 letters up to 512 = eight slots exactly;
  * every model the constructor accepts has a dense v|h launch within the LDS.

The driver is host code alone: compiled here as it stands and loaded into this process."""
import ctypes
import os
import subprocess

import pytest

from tests import generic_geom_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LDS = 160 * 1024
FIELDS = ["KS", "TS", "split", "hgv_lds", "JS", "vgh_CH", "vgh_lds", "R", "stats_CH", "stats_lds", "eval_lds", "dense_lds",
          "dense_KS", "LW", "NW"]
KNOBS = ["CRBM_FORCE_BIG", "CRBM_SLAB_STATS", "CRBM_SLAB_MOTIFS", "CRBM_SLAB_GROUP", "CRBM_SLAB_TABLE_BUDGET", "CRBM_GROUP",
         "CRBM_TABLE_BUDGET"]


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("generic_geom") / "libplan_driver.so")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-fPIC", "-shared", "-I", os.path.join(ROOT, "crbm_amd", "csrc"),
                           os.path.join(ROOT, "tests", "emu", "plan_driver.cpp"), "-o", path])
    return ctypes.CDLL(path)


@pytest.fixture(autouse=True)
def default_knobs(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


def geom(lib, A, K, M, pool=1, n=3, L=None, Lf=None, num_cu=cases.NUM_CU):
    L = M + 28 if L is None else L
    out = (ctypes.c_long * 32)()
    cnt = lib.big_geom_ints(K, M, A, pool, n, L, (L - M + 1) if Lf is None else Lf, num_cu, out)
    assert cnt == len(FIELDS)
    return dict(zip(FIELDS, out[:cnt]))


def slab_count(lib, c):
    """slabs of the slab model the plan gives the case (0: off the slab route)"""
    out = (ctypes.c_int * 64)()
    lib.plan_ints(c["K"], c["M"], int(c["ds"]), c["A"], c["pool"], c["Lf"], c["B"], cases.NUM_CU, out)
    big, slab_K = out[0], out[8]
    assert big == 1, "the case is not on the generic path"
    return 0 if slab_K == 0 else -(-c["K"] // slab_K)


def check_regime(lib, c, Lf=None):
    g = geom(lib, c["A"], c["K"], c["M"], c["pool"], c["n"], c["L"], c["Lf"] if Lf is None else Lf)
    A, M, L = c["A"], c["M"], c["L"]
    Lv = (c["Lf"] if Lf is None else Lf) + M - 1
    got = dict(KS=g["KS"], TS=g["TS"], split=g["split"], hgv_fits=g["hgv_lds"] <= LDS, col_slabs=-(-M // g["JS"]),
               vgh_chunks=-(-Lv // g["vgh_CH"]), stats_chunks=-(-(L - M + 1) // g["stats_CH"]), stats_CH=g["stats_CH"], R=g["R"],
               slots=-(-A * M // 256), NW=g["NW"])
    want = dict(c["regime"])
    if "slab_n" in want:
        assert slab_count(lib, c) == want.pop("slab_n"), c["id"]
    for key, v in want.items():
        assert got[key] == v, (c["id"], key, got[key], v)
    # what every case launches fits: the chain kernels at the chains' length, statistics and evaluation at both lengths
    assert g["vgh_lds"] <= LDS and g["stats_lds"] <= LDS and g["eval_lds"] <= LDS and A * M <= 8 * 256, c["id"]
    if want.get("hgv_fits", True):
        assert g["hgv_lds"] <= LDS, c["id"]
        chain = geom(lib, A, c["K"], M, c["pool"], c["B"], Lv, Lv - M + 1)
        assert chain["hgv_lds"] <= LDS and chain["stats_lds"] <= LDS, c["id"]
    return g


@pytest.mark.parametrize("c", cases.FULL + cases.LONG + [cases.REFUSED], ids=lambda c: c["id"])
def test_case_lies_in_its_regime(lib, c):
    check_regime(lib, c)


@pytest.mark.parametrize("c,lengths", cases.CHAINS, ids=[c["id"] for c, _ in cases.CHAINS])
def test_chain_cases_take_their_chunks(lib, c, lengths):
    for Lf, chunks in lengths:
        c2 = dict(c, regime=dict(c["regime"], vgh_chunks=chunks))
        g = check_regime(lib, c2, Lf=Lf)
        assert g["vgh_CH"] == (2048 if c["A"] == 4 else 256)
    # the chunk loop's own boundary: a chain of exactly one chunk, one position more, and three chunks with a remainder
    Lvs = [Lf + c["M"] - 1 for Lf, _ in lengths]
    CH = 2048 if c["A"] == 4 else 256
    assert Lvs[0] == CH and Lvs[1] == CH + 1 and 2 * CH < Lvs[2] < 3 * CH


def test_forced_chain_case(lib, monkeypatch):
    c, lengths = cases.FORCED_CHAIN
    monkeypatch.setenv("CRBM_FORCE_BIG", "1")
    for Lf, chunks in lengths:
        check_regime(lib, dict(c, regime=dict(vgh_chunks=chunks)), Lf=Lf)
        assert Lf + c["M"] - 1 == 2049
        assert slab_count(lib, dict(c, Lf=Lf)) == 1          # one slab of its ten motifs


def test_boundaries(lib):
    ks = lambda A, M: geom(lib, A, 3, M)["KS"]
    assert [ks(4, 170), ks(4, 171), ks(4, 307), ks(4, 308), ks(4, 512)] == [32, 16, 16, 8, 8]
    assert [ks(1, 682), ks(1, 683), ks(1, 1228), ks(1, 1229), ks(1, 2048)] == [32, 16, 16, 8, 8]
    assert [ks(64, 10), ks(64, 11), ks(64, 19), ks(64, 20), ks(64, 32)] == [32, 16, 16, 8, 8]
    assert geom(lib, 5, 3, 300, pool=2, L=327)["KS"] == 8 and geom(lib, 4, 3, 10, pool=2, L=37)["KS"] == 8    # pooled: starts at 8 and stays
    js = lambda A, M: geom(lib, A, 3, M)["JS"]
    assert [js(4, 128), js(4, 129), js(64, 8), js(64, 9), js(20, 25), js(20, 26), js(3, 170), js(3, 171)] == [128, 128, 8, 8, 25, 25, 170, 170]
    ch = lambda A, Lv: -(-Lv // geom(lib, A, 3, 5, Lf=Lv - 4)["vgh_CH"])
    assert [ch(4, 2048), ch(4, 2049), ch(3, 256), ch(3, 257), ch(20, 256), ch(20, 257)] == [1, 2, 1, 2, 1, 2]
    sc = lambda Lh, pool=1: geom(lib, 4, 3, 5, pool=pool, L=Lh + 4)
    assert [-(-Lh // sc(Lh)["stats_CH"]) for Lh in (4096, 4097)] == [1, 2]
    assert sc(4098, 3)["stats_CH"] == 4095 and sc(40)["stats_CH"] == 64 and sc(30, 3)["stats_CH"] == 63
    r = lambda K, n: geom(lib, 4, K, 5, n=n)["R"]
    assert [r(2048, 3), r(2049, 3), r(1024, 3), r(1024, 2), r(300, 10)] == [1, 1, 2, 2, 6]
    # split: several mask words and fewer tiles than four per compute unit
    sp = lambda K, n: geom(lib, 4, K, 5, n=n)["split"]
    assert [sp(32, 3), sp(33, 3), sp(33, 1023), sp(33, 1024)] == [0, 1, 1, 0]
    # rows per tile on long rows: the letters' share of the LDS gives none, the clamp gives one
    assert geom(lib, 3, 3, 4, n=5000, L=32769)["TS"] == 1 and geom(lib, 3, 3, 4, n=5000, L=40)["TS"] == 5
    # beside 96 KB of filters a row of 64-letter bytes fits up to 65 400 letters or so: the launch is refused beyond
    assert geom(lib, 64, 3, 32, L=65000)["hgv_lds"] <= LDS < geom(lib, 64, 3, 32, L=66000)["hgv_lds"]


def test_the_row_stride_of_one_needs_more_motifs_than_eight_per_compute_unit(lib):
    assert geom(lib, 3, 2100, 2, n=3)["R"] == 1 and geom(lib, 3, 2048, 2, n=3)["R"] == 1 and geom(lib, 3, 1000, 2, n=3)["R"] == 2


@pytest.mark.parametrize("d", cases.DENSE, ids=lambda d: d[0])
def test_dense_vgh_cases(lib, d):
    _, A, K, M, ds, n, Lh, slabs = d
    g = geom(lib, A, K, M, n=n, L=Lh + M - 1)
    assert g["dense_lds"] <= 64 * 1024 and -(-K // g["dense_KS"]) == slabs
    if d[0].endswith("second_round"):
        assert n * (Lh + M - 1) > 8 * cases.NUM_CU * 256            # the grid-stride loop of vgh_dense_any_kernel runs a second round


def test_every_accepted_model_has_a_dense_vgh_launch(lib):
    """motif_length <= 512 (DNA), num_motifs <= 65536, K A M <= 2^26: the slab of the dense v|h pass holds at least 8 motifs
    and stays within its budget, where the whole filter set took M K 16 bytes (300 x 40: 192 000)"""
    for K, M in [(1, 1), (10, 15), (300, 40), (256, 64), (65536, 1), (32768, 512), (8, 512), (7, 512), (4096, 1), (4097, 1), (102, 40), (103, 40)]:
        g = geom(lib, 4, K, M)
        assert 1 <= g["dense_KS"] <= K and g["dense_KS"] * M * 16 == g["dense_lds"] <= 64 * 1024, (K, M)
        assert g["dense_KS"] == K or g["dense_KS"] >= 8, (K, M)
    assert geom(lib, 4, 4096, 1)["dense_KS"] == 4096 and geom(lib, 4, 4097, 1)["dense_KS"] == 4096
    assert geom(lib, 4, 102, 40)["dense_KS"] == 102 and geom(lib, 4, 103, 40)["dense_KS"] == 102
