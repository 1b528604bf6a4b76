"""The chain kernel body (crbm_kernels.h: gibbs_body, set-bit walk) in both geometry forms on CPU threads under
AddressSanitizer + UBSan: tests/emu/geom_main.cpp, a stand-alone program built here and run directly.  GeomCT (the launch
geometry compiled in) must leave exactly the words GeomRT (the geometry in the arguments) leaves -- hidden masks of both
strands, letters of the last visible sample, activity counts -- from the same state and seeds, with one and with three
steps per launch:

  ss_186_aligned      (K, M, ds, Lf, chains, S) = (10, 15, ss, 186, 8, 4): 16-byte state loads, one tile per block
  ss_185              (10, 15, ss, 185, 8, 4): 185 words per chain (a tile of four is still 16-byte aligned)
  ss_185_word_path    (10, 15, ss, 185, 6, 2): 370 words per tile, the 4-byte load path compiled in
  ds_50               (10, 15, ds, 50, 6, 2): both strands, three tiles on two blocks (the tile loop)
  two_mask_words      (40, 6, ss, 30, 4, 4): two mask words per position
  ragged_falls_back   (10, 15, ss, 186, 9, 4): a ragged last tile -- geo_spec (crbm_plan.h) must refuse it, the launch
                      stays in the run-time form
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = {"ss_186_aligned": "ct", "ss_185": "ct", "ss_185_word_path": "ct", "ds_50": "ct", "two_mask_words": "ct",
         "ragged_falls_back": "rt"}


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("emu_geom") / "geom_main")
    emu = os.path.join(ROOT, "tests", "emu")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g1", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                           "-fno-sanitize-recover=undefined", "-mf16c", "-I", os.path.join(emu, "shim"), "-I", emu,
                           "-I", os.path.join(ROOT, "crbm_amd", "csrc"), os.path.join(emu, "geom_main.cpp"), "-o", path,
                           "-lpthread"])
    return path


@pytest.mark.parametrize("steps", [1, 3])
@pytest.mark.parametrize("which", sorted(CASES))
def test_geometry_forms_leave_the_same_words(exe, which, steps):
    r = subprocess.run([exe, which, str(steps)], capture_output=True, text=True, timeout=900)   # the inherited environment, as it is
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "GEOM OK %s %d form=%s " % (which, steps, CASES[which]) in r.stdout, r.stdout[-2000:]
