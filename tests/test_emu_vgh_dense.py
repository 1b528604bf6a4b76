"""The dense v|h kernel of DNA models (crbm_kernels.h: vgh_dense_kernel) on CPU threads under AddressSanitizer + UBSan:
tests/emu/vgh_dense_main.cpp, a stand-alone program built here and run directly.  The kernel stages its filters a slab
of motifs at a time within a fixed LDS budget (crbm_layout.h, vgh_dense_ks); the emulation of tests/emu/run_emu.py only
reaches models of one slab.  Here: 10 x 15 (one slab), 300 x 40 on both strands (three slabs of 102, 102 and 96 motifs),
256 x 64 (four slabs, four rows per tile), 4099 x 1 (a last slab of three motifs) and 9 x 512 (slabs of 8 and 1), each with
the LDS the host gives the launch, against a double-precision loop; every probability column sums to one and every
position holds one sampled letter."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dense_vgh_slabs(tmp_path):
    exe = str(tmp_path / "vgh_dense_main")
    emu = os.path.join(ROOT, "tests", "emu")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g1", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                           "-fno-sanitize-recover=undefined", "-mf16c", "-I", os.path.join(emu, "shim"), "-I", emu,
                           "-I", os.path.join(ROOT, "crbm_amd", "csrc"), os.path.join(emu, "vgh_dense_main.cpp"), "-o", exe,
                           "-lpthread"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=900)      # the inherited environment, as it is
    assert r.returncode == 0 and "DENSE OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    for want in ("K=10 M=15 ds=1 ks=10 slabs=1 ", "K=300 M=40 ds=1 ks=102 slabs=3 ", "K=256 M=64 ds=0 ks=64 slabs=4 ",
                 "K=4099 M=1 ds=0 ks=4096 slabs=2 ", "K=9 M=512 ds=1 ks=8 slabs=2 "):
        assert want in r.stdout, r.stdout[-2000:]
