"""The chain v|h kernels of the generic path (crbm_kernels_generic.h: big_vgh_kernel, big_vgh_any_kernel) on CPU threads
under AddressSanitizer + UBSan, at the geometry no other emulation reaches: tests/emu/big_vgh_main.cpp, a stand-alone
program built here and run directly, with its inputs and outputs in files.  With 64-thread blocks a chunk holds 512
visible positions (DNA) or 64 (any other alphabet), and the LDS of a block is what the host's formula gives (crbm_plan.h,
big_vgh_geom), to the byte.

Cases, each on one strand and on both, K = 37 (two mask words, the second of five motifs), three chains on two blocks:
  chunks       Lv = CH (one chunk exactly), CH + 1 (a second chunk of one position) and 2 CH + 3 (three chunks); from
               the second chunk on the staged mask words start at hidden position c0 - (M - 1), and M - 1 >= 16 puts
               that off the letter-word boundary the chunk itself starts on
  col slabs    JS < M with M = 2 JS + 1 (two full slabs and one of a single column; the mask words are loaded with the
               first slab only): DNA 17 letters in slabs of 8, and 257 in the host's slabs of 128; 3 letters: 17 in
               slabs of 8; 20 letters: 51 in the host's slabs of 25
The letters must be the oracle's (OracleCRBM._computeVgivenH on the same uniforms); where one differs, a threshold of its
position lies within 1e-6 of the uniform (float32 against float64), and that at no more than 1e-4 of the positions + 2.
"""
import os
import subprocess

import numpy as np
import pytest

from oracle.crbm_oracle import OracleCRBM, visible_uniforms, KIND_CHAIN_V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TIE = 1e-6
K, CHAINS, GRID, THREADS = 37, 3, 2, 64
SEED, STEP, OFFSET = 0x1234567890, 7, 5

# (A, M, JS or 0 for the host's, JS expected, [Lv ...])
SHAPES = [
    (4, 17, 8, 8, [512, 513, 1027]),
    (4, 257, 0, 128, [1027]),
    (3, 17, 8, 8, [64, 65, 131]),
    (20, 51, 0, 25, [64, 65, 131]),
]
CASES = [(A, M, JS, JSx, Lv, ds) for (A, M, JS, JSx, Lvs) in SHAPES for Lv in Lvs for ds in (False, True)]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("emu_big_vgh") / "big_vgh_main")
    emu = os.path.join(ROOT, "tests", "emu")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g1", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                           "-fno-sanitize-recover=undefined", "-mf16c", "-I", os.path.join(emu, "shim"), "-I", emu,
                           "-I", os.path.join(ROOT, "crbm_amd", "csrc"), os.path.join(emu, "big_vgh_main.cpp"), "-o", path,
                           "-lpthread"])
    return path


def pack_masks(h):
    """(B, K, 1, Lf) of 0/1 -> uint32 [B][Lf][NW]"""
    B, K_, _, Lf = h.shape
    NW = (K_ + 31) // 32
    bits = np.zeros((B, Lf, NW * 32), dtype=np.uint64)
    bits[:, :, :K_] = h[:, :, 0, :].transpose(0, 2, 1)
    w = (bits.reshape(B, Lf, NW, 32) << np.arange(32, dtype=np.uint64)).sum(axis=3)
    return np.ascontiguousarray(w.astype(np.uint32))


def unpack_letters(vout, A, Lv):
    """rows of packed letters -> (B, Lv) letter codes, and the words behind the letters (which must be zero)"""
    if A == 4:
        p = np.arange(Lv)
        letters = (vout[:, p >> 4] >> (2 * (p & 15)).astype(np.uint32)) & 3
        used = (Lv + 15) // 16
        tail = vout[:, used - 1] >> np.uint32(2 * (Lv % 16)) if Lv % 16 else np.zeros(len(vout), np.uint32)
    else:
        by = np.ascontiguousarray(vout).view(np.uint8).reshape(len(vout), -1)
        letters = by[:, :Lv]
        used = (Lv + 3) // 4
        tail = by[:, Lv:4 * used].sum(axis=1)
    return letters.astype(np.int64), vout[:, used:], tail


@pytest.mark.parametrize("A,M,JS,JSx,Lv,ds", CASES, ids=["A%d_M%d_Lv%d_%s" % (c[0], c[1], c[4], "ds" if c[5] else "ss") for c in CASES])
def test_chain_vgh_chunks_and_column_slabs(exe, tmp_path, A, M, JS, JSx, Lv, ds):
    Lf = Lv - M + 1
    rng = np.random.default_rng(100 * A + M + Lv)
    W = (rng.standard_normal((K, 1, A, M)) * 0.7 * np.sqrt(15.0 / M)).astype(np.float32)
    c = (rng.standard_normal((1, A)) * 0.3).astype(np.float32)
    h = rng.binomial(1, 0.1, size=(CHAINS, K, 1, Lf)).astype(np.float64)
    hp = rng.binomial(1, 0.1, size=h.shape).astype(np.float64) if ds else None
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        np.array([A, K, M, int(ds), CHAINS, Lf, JS, THREADS, GRID, SEED & 0xFFFFFFFF, SEED >> 32, STEP, OFFSET], dtype=np.int32).tofile(f)
        W.tofile(f)
        c.tofile(f)
        pack_masks(h).tofile(f)
        if ds:
            pack_masks(hp).tofile(f)
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=900)      # the inherited environment, as it is
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    CH = 512 if A == 4 else 64
    assert "BIG_VGH OK chunks=%d col_slabs=%d " % (-(-Lv // CH), -(-M // JSx)) in r.stdout, r.stdout[-2000:]
    assert M - 1 >= 16 and JSx < M and M == 2 * JSx + 1
    raw = np.fromfile(fout, dtype=np.uint32)
    LWs, JSgot, CHgot = (int(x) for x in raw[:3].view(np.int32))
    assert (JSgot, CHgot) == (JSx, CH) and raw.size == 3 + CHAINS * LWs
    got, pad, tail = unpack_letters(raw[3:].reshape(CHAINS, LWs), A, Lv)
    assert pad.shape[1] >= 2 and not pad.any() and not np.any(tail), "the words behind the letters are not zero"
    assert got.max() < A
    # the oracle, on the kernel's uniforms
    o = OracleCRBM(K, M, doublestranded=ds, input_dims=A, batchsize=CHAINS, fantasy_hidden_len=Lf, seed=SEED, W=W)
    o.c = c.astype(np.float64)
    u = visible_uniforms(SEED, STEP, np.arange(CHAINS) + OFFSET, Lv, KIND_CHAIN_V)
    Pv, v = o._computeVgivenH(h, hp, u)
    want = v[:, 0].argmax(axis=1)                                        # (B, Lv)
    bad = got != want
    gap = np.min(np.abs(np.cumsum(Pv[:, 0], axis=1)[:, :max(A - 1, 1)] - u[:, None, :]), axis=1)
    assert np.all(gap[bad] < TIE), "letters differ away from a tie at %s" % (np.argwhere(bad & (gap >= TIE))[:8].tolist(),)
    assert bad.sum() <= 1e-4 * CHAINS * Lv + 2
    assert len(np.unique(want)) == A or A > 4                            # the sample is not degenerate
