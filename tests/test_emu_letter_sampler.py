"""The visible-letter sampler of the chain kernel (crbm_kernels.h: push_letter, sample_letter, letter_byte) and the 32-bit
packing of its mask window (pack_masks) on the CPU under AddressSanitizer + UBSan: tests/emu/letter_main.cpp, a stand-alone
program built here and run directly.  The letter is read off the SIGNS of t - threshold (t == threshold gives +0: reached)
and shifted into the byte two bits per position; the program holds this against the expressions it replaced -- three
comparisons added up, a select per position -- written out in the test itself:

  2^22 random (y0..y3, u) over every scale of activation, u on the 24-bit grid of u01
  all four activations equal, pairs of equal activations, differences beyond 150 (e = 0), u = 0 and u = 1 - 2^-24
  constructed ties t == threshold (activations a whole number apart: every e a power of two) and u one step to either side
  the letter byte of every four positions for every remainder of Lv % 4
  the window word of every mask width that packs several masks (straddling bit 32 or not) against the 64-bit shifts

Not one disagreement is tolerated.
"""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("emu_letter") / "letter_main")
    emu = os.path.join(ROOT, "tests", "emu")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g1", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                           "-fno-sanitize-recover=undefined", "-ffp-contract=off", "-mf16c", "-I", os.path.join(emu, "shim"),
                           "-I", emu, "-I", os.path.join(ROOT, "crbm_amd", "csrc"), os.path.join(emu, "letter_main.cpp"),
                           "-o", path, "-lpthread"])
    return path


def test_letters_bytes_and_window_words_are_what_they_were(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)   # the inherited environment, as it is
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    m = re.search(r"LETTER OK cases=(\d+) ties=(\d+)", r.stdout)
    assert m, r.stdout[-2000:]
    assert int(m.group(1)) > (1 << 22) and int(m.group(2)) >= 100
