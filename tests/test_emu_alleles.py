"""The allele-effect kernels (crbm_kernels.h: scan_encode_kernel, allele_effects_body, allele_combine_kernel) on CPU
threads under AddressSanitizer + UBSan: tests/emu/alleles_main.cpp, a stand-alone program built here and run directly,
all blocks of a grid at once.  Its outputs are held to the float64 reference of tests/allele_reference.py by that
module's criterion at the emulation's RTOL (dfe and per_motif separately, windows and the exact zeros exactly): single-
and double-stranded models, M = 1 (an insertion has no ref windows), motifs in two and three groups of quads, a
40-letter motif, a slabbed model whose last slab overlaps its neighbour, on streams with gaps at tile and word edges;
about 200 random alleles plus the forced ones of allele_list; V = 1, V = 65 and T = M; two grid and block sizes and the
reversed list with the same bits; allele_plan through the program's `plan` sub-command.  Guard words around every
output must be intact."""
import os
import subprocess

import numpy as np
import pytest

from tests.emu import harness
from tests.test_emu_scan import gapped_stream
from tests.allele_reference import allele_effects, allele_list, check, pack

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL = 2e-5
GUARD, GUARD_WORD = 8, 0xDEADBEEF
CFG = {0: (10, 15, True), 1: (10, 5, False), 2: (6, 1, True), 3: (20, 15, True), 4: (36, 6, False), 5: (5, 40, True)}
# (configuration, motifs, model seed, T, stream seed, list seed) of every list below: tests/test_allele_reference.py
# checks that each meets full, partial and zero window counts on both haplotypes
LISTS = {"ds_10x15": (0, 10, 25, 611, 3, 1), "ss_10x5": (1, 10, 15, 590, 4, 1), "m1": (2, 6, 7, 330, 5, 1),
         "two_groups": (3, 20, 35, 600, 6, 1), "three_groups": (4, 36, 42, 597, 7, 1), "m40": (5, 5, 45, 627, 8, 1),
         "slabs": (0, 23, 51, 603, 13, 1), "geometries": (3, 20, 35, 611, 12, 2)}
N_RANDOM = 200


def case(name):
    """(cid, oracle, stream, pos, R, alts) of LISTS[name]"""
    cid, K, mseed, T, sseed, lseed = LISTS[name]
    _, M, ds = CFG[cid]
    stream = gapped_stream(T, sseed, M)
    return (cid, harness.random_model(K, M, ds, mseed, draw_c=True), stream) + allele_list(stream, M, N_RANDOM, lseed)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("emu_alleles") / "alleles_main")
    emu = os.path.join(ROOT, "tests", "emu")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g1", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                           "-fno-sanitize-recover=undefined", "-mf16c", "-I", os.path.join(emu, "shim"), "-I", emu,
                           "-I", os.path.join(ROOT, "crbm_amd", "csrc"), os.path.join(emu, "alleles_main.cpp"), "-o", path,
                           "-lpthread"])
    return path


def _run(exe, tmp_path, cid, o, stream, pos, R, alts, grid=2, threads=128):
    """dict of dfe (V,), per_motif (V, K), windows (V, 2) of one run of the program"""
    K, M = o.num_motifs, o.motif_length
    assert CFG[cid][1:] == (M, bool(o.doublestranded)) and K >= CFG[cid][0]
    V = len(pos)
    off, codes = pack(alts)
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(np.array([cid, K, stream.size, V, grid, threads], np.int32).tobytes())
        f.write(np.ascontiguousarray(o.W.reshape(K, 4, M), np.float32).tobytes())
        f.write(np.ascontiguousarray(o.b.ravel(), np.float32).tobytes())
        f.write(np.ascontiguousarray(o.c.ravel(), np.float32).tobytes())
        f.write(np.ascontiguousarray(stream, np.uint8).tobytes())
        f.write(np.ascontiguousarray(pos, np.int64).tobytes())
        f.write(np.ascontiguousarray(R, np.int32).tobytes())
        f.write(off.tobytes())
        f.write(codes.tobytes())
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=900)      # the inherited environment, as it is
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    out = np.fromfile(fout, np.uint32)
    assert out.size == 4 * GUARD + V * (K + 3)
    a = GUARD
    dfe = out[a:a + V].view(np.float32)
    b = a + V + GUARD
    pm = out[b:b + V * K].view(np.float32).reshape(V, K)
    c = b + V * K + GUARD
    win = out[c:c + 2 * V].view(np.int32).reshape(V, 2)
    guards = np.concatenate([out[:a], out[a + V:b], out[b + V * K:c], out[c + 2 * V:]])
    assert guards.size == 4 * GUARD and np.all(guards == GUARD_WORD), "a guard word was written"
    return {"dfe": dfe.copy(), "per_motif": pm.copy(), "windows": win.copy()}


def _same(a, b):
    for key in ("dfe", "per_motif", "windows"):
        assert np.array_equal(a[key].view(np.uint32), b[key].view(np.uint32)), key


def _check(exe, tmp_path, name, **kw):
    cid, o, stream, pos, R, alts = case(name)
    got = _run(exe, tmp_path, cid, o, stream, pos, R, alts, **kw)
    check(got, allele_effects(o, stream, pos, R, alts), RTOL, name)
    return pos, R, alts, got


def test_ds_10x15(exe, tmp_path):
    pos, R, alts, got = _check(exe, tmp_path, "ds_10x15")
    dup = int(np.flatnonzero((R[:-1] == 2) & (np.array([len(a) for a in alts[:-1]]) == 5) & (pos[:-1] == pos[-1]))[0])
    assert got["dfe"][dup].tobytes() == got["dfe"][-1].tobytes() and got["per_motif"][dup].tobytes() == got["per_motif"][-1].tobytes()
    assert np.abs(got["dfe"][-1]) > 0


def test_ss_10x5(exe, tmp_path):
    _check(exe, tmp_path, "ss_10x5")


def test_m1_an_insertion_has_no_ref_windows(exe, tmp_path):
    pos, R, alts, got = _check(exe, tmp_path, "m1")
    ins = (R == 0) & (np.array([len(a) for a in alts]) > 0)
    assert ins.any() and np.all(got["windows"][ins, 0] == 0) and np.all(got["windows"][ins, 1] == np.array([len(a) for a in alts])[ins])


def test_two_and_three_quad_groups(exe, tmp_path):
    _check(exe, tmp_path, "two_groups")
    _check(exe, tmp_path, "three_groups")


def test_m40(exe, tmp_path):
    _check(exe, tmp_path, "m40")


def test_slabs_with_an_overlapping_last_slab(exe, tmp_path):
    """23 motifs as slabs of 10: the last slab is moved back to motifs 13..22 and leaves the seven its neighbour writes
    alone.  dfe adds all columns in ascending k."""
    _check(exe, tmp_path, "slabs")


def test_one_variant_65_variants_and_t_eq_m(exe, tmp_path):
    cid, o, stream, pos, R, alts = case("ds_10x15")
    full = _run(exe, tmp_path, cid, o, stream, pos, R, alts)
    one = _run(exe, tmp_path, cid, o, stream, pos[7:8], R[7:8], alts[7:8])                  # V = 1: three idle waves
    _same(one, {k: v[7:8] for k, v in full.items()})
    some = _run(exe, tmp_path, cid, o, stream, pos[:65], R[:65], alts[:65])                  # V = 65: one wave takes a second variant
    _same(some, {k: v[:65] for k, v in full.items()})
    check(some, allele_effects(o, stream, pos[:65], R[:65], alts[:65]), RTOL, "V = 65")
    tm = np.random.default_rng(9).integers(0, 4, size=15, dtype=np.uint8)                     # T = M: one window of the stream
    p, r, a = allele_list(tm, 15, 40, 3)
    got = _run(exe, tmp_path, cid, o, tm, p, r, a)
    check(got, allele_effects(o, tm, p, r, a), RTOL, "T = M")
    snp = (r == 1) & (np.array([len(x) for x in a]) == 1)
    assert snp.any() and np.all(got["windows"][snp] == 1)
    none = _run(exe, tmp_path, cid, o, stream, pos[:0], R[:0], alts[:0])                      # V = 0: nothing written
    assert none["dfe"].size == 0


def test_geometries_and_a_reversed_list_give_the_same_bits(exe, tmp_path):
    cid, o, stream, pos, R, alts = case("geometries")
    got = _run(exe, tmp_path, cid, o, stream, pos, R, alts)
    check(got, allele_effects(o, stream, pos, R, alts), RTOL, "geometries")
    for grid, threads in ((1, 256), (3, 64)):
        _same(got, _run(exe, tmp_path, cid, o, stream, pos, R, alts, grid=grid, threads=threads))
    rev = _run(exe, tmp_path, cid, o, stream, pos[::-1], R[::-1], alts[::-1], grid=3, threads=64)
    _same(got, {k: v[::-1] for k, v in rev.items()})


def test_allele_plan_budget_chunks_and_layout(exe, tmp_path):
    """allele_plan (crbm_sweep.h) is what the driver cuts the list by.  A variant costs its n = R + A + 4M - 4 staged
    codes, three bits per code, its 16-byte table entry and 4 (K + 3) output bytes; a chunk is the longest prefix of
    what is left within the budget and within 2^30 staged codes, at least one variant, within 32 MB unless the budget
    was set by hand; two buffer sets exactly when there is more than one chunk; the sets are sized for the longest
    chunk and for the most staged codes."""
    def plan(R, A, M, K, budget, was_set):
        R, A = np.asarray(R, np.int32), np.asarray(A, np.int32)
        path = str(tmp_path / "lengths.bin")
        with open(path, "wb") as f:
            f.write(np.array([R.size], np.int32).tobytes() + R.tobytes() + A.tobytes())
        out = subprocess.run([exe, "plan"] + [str(x) for x in (M, K, budget, was_set, path)], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stderr
        v = [int(x) for x in out.stdout.split()]
        nsets, max_cnt, max_codes, valid_words, cuts = v[0], v[1], v[2], v[3], np.array(v[4:])
        n = R.astype(np.int64) + A + 4 * M - 4
        cost = n + (3 * n + 7) // 8 + 16 + 4 * (K + 3)
        limit = budget if was_set else min(budget, 32 << 20)
        assert cuts[0] == 0 and cuts[-1] == R.size and np.all(np.diff(cuts) >= 1)
        assert nsets == (2 if cuts.size > 2 else 1) and max_cnt == np.diff(cuts).max()
        codes = [int(n[a:b].sum()) for a, b in zip(cuts[:-1], cuts[1:])]
        assert max_codes == max(codes) <= 1 << 30 and valid_words == (max_codes + 63) // 64 + 2
        for a, b in zip(cuts[:-1], cuts[1:]):
            assert b - a == 1 or cost[a:b].sum() <= limit                                   # within the budget, or a single variant
            assert b == R.size or cost[a:b + 1].sum() > limit or n[a:b + 1].sum() > 1 << 30     # and no longer prefix is
        return cuts, cost
    snp = np.ones(2022, np.int32)
    cuts, cost = plan(snp, snp, 15, 10, 256 << 20, 0)
    assert cost[0] == 58 + 22 + 16 + 52 and cuts.tolist() == [0, 2022]                       # config #2: 148 bytes a SNP, one chunk
    big = np.ones(10 ** 6, np.int32)
    assert plan(big, big, 15, 10, 256 << 20, 0)[0][1] == (32 << 20) // 148                   # the 32 MB clamp of the default budget
    assert plan(big, big, 15, 10, 256 << 20, 1)[0].tolist() == [0, 10 ** 6]                  # ... which a hand-set budget lifts
    assert plan(snp, snp, 15, 10, 1, 1)[0].size == 2023                                      # CRBM_SLAB_BYTES=1: one variant a chunk
    assert plan(snp, snp, 15, 10, 148 * 300, 1)[0].size == 8                                 # 7 chunks
    rng = np.random.default_rng(4)
    R, A = rng.integers(0, 200, size=3000), rng.integers(0, 200, size=3000)
    R[17], A[1800] = 65535, 65535
    cuts, _ = plan(R, A, 6, 36, 50000, 1)                                                    # chunks of different lengths, two single-variant ones
    assert np.unique(np.diff(cuts)).size > 3
    long = np.full(9000, 65535, np.int32)
    cuts, _ = plan(long, long, 64, 1, 1 << 40, 1)                                            # the 32-bit window starts of a chunk
    assert cuts[1] == (1 << 30) // (2 * 65535 + 252)
