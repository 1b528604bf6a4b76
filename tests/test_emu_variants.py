"""The variant-effect kernels (crbm_kernels.h: scan_encode_kernel, variant_effects_body, variant_combine_kernel) on CPU
threads under AddressSanitizer + UBSan: tests/emu/variants_main.cpp, a stand-alone program built here and run directly,
all blocks of a grid at once.  Its outputs are held to the float64 reference of tests/variant_reference.py by the
project's mutagenesis criterion at the emulation's RTOL (dfe and per_motif separately, windows and the exact zeros
exactly): single- and double-stranded models, M = 1 (a context of one code), motifs in two and three groups of quads, a
40-letter motif, a slabbed model whose last slab overlaps its neighbour, on streams with gaps at tile and word edges;
about 300 random variants plus positions 0, 1, M-2, M-1, T-M, T-2, T-1, both neighbours of every gap edge, a position
inside a gap, a duplicate and an alt == ref; V = 1, V = 65 and T = M; two grid and block sizes and the reversed list
with the same bits.  Guard words around every output must be intact."""
import os
import subprocess

import numpy as np
import pytest

from tests.emu import harness
from tests.test_emu_scan import gapped_stream
from tests.variant_reference import variant_effects, variant_list, check

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL = 2e-5
GUARD, GUARD_WORD = 8, 0xDEADBEEF
CFG = {0: (10, 15, True), 1: (10, 5, False), 2: (6, 1, True), 3: (20, 15, True), 4: (36, 6, False), 5: (5, 40, True)}


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("emu_variants") / "variants_main")
    emu = os.path.join(ROOT, "tests", "emu")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g1", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                           "-fno-sanitize-recover=undefined", "-mf16c", "-I", os.path.join(emu, "shim"), "-I", emu,
                           "-I", os.path.join(ROOT, "crbm_amd", "csrc"), os.path.join(emu, "variants_main.cpp"), "-o", path,
                           "-lpthread"])
    return path


def _run(exe, tmp_path, cid, o, stream, pos, alt, grid=2, threads=128):
    """dict of dfe (V,), per_motif (V, K), windows (V,) of one run of the program"""
    K, M = o.num_motifs, o.motif_length
    assert CFG[cid][1:] == (M, bool(o.doublestranded)) and K >= CFG[cid][0]
    V = len(pos)
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(np.array([cid, K, stream.size, V, grid, threads], np.int32).tobytes())
        f.write(np.ascontiguousarray(o.W.reshape(K, 4, M), np.float32).tobytes())
        f.write(np.ascontiguousarray(o.b.ravel(), np.float32).tobytes())
        f.write(np.ascontiguousarray(o.c.ravel(), np.float32).tobytes())
        f.write(np.ascontiguousarray(stream, np.uint8).tobytes())
        f.write(np.ascontiguousarray(pos, np.int64).tobytes())
        f.write(np.ascontiguousarray(alt, np.uint8).tobytes())
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=900)      # the inherited environment, as it is
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    out = np.fromfile(fout, np.uint32)
    assert out.size == 4 * GUARD + V * (K + 2)
    a = GUARD
    dfe = out[a:a + V].view(np.float32)
    b = a + V + GUARD
    pm = out[b:b + V * K].view(np.float32).reshape(V, K)
    c = b + V * K + GUARD
    win = out[c:c + V].view(np.int32)
    guards = np.concatenate([out[:a], out[a + V:b], out[b + V * K:c], out[c + V:]])
    assert guards.size == 4 * GUARD and np.all(guards == GUARD_WORD), "a guard word was written"
    return {"dfe": dfe.copy(), "per_motif": pm.copy(), "windows": win.copy()}


def _same(a, b):
    for key in ("dfe", "per_motif", "windows"):
        assert np.array_equal(a[key].view(np.uint32), b[key].view(np.uint32)), key


def _check(exe, tmp_path, cid, o, stream, n_random=300, seed=1, **kw):
    M = o.motif_length
    pos, alt = variant_list(stream, M, n_random, seed)
    want = variant_effects(o, stream, pos, alt)
    w = want["windows"]
    assert (w == M).any() and (w == 0).any() and (M == 1 or ((0 < w) & (w < M)).any())      # no case hides a branch (M = 1 has no partial count)
    got = _run(exe, tmp_path, cid, o, stream, pos, alt, **kw)
    check(got, want, RTOL, "cfg %d" % cid)
    return pos, alt, got


def test_ds_10x15(exe, tmp_path):
    o = harness.random_model(10, 15, True, 25, draw_c=True)
    pos, alt, got = _check(exe, tmp_path, 0, o, gapped_stream(611, 3, 15))
    assert got["dfe"][-1] == 0.0 and np.all(got["per_motif"][-1] == 0.0)                    # alt == ref
    dup = int(np.flatnonzero((pos[:-2] == pos[-2]) & (alt[:-2] == alt[-2]))[0])                                      # the duplicate: the same bits
    assert got["dfe"][dup].tobytes() == got["dfe"][-2].tobytes() and got["per_motif"][dup].tobytes() == got["per_motif"][-2].tobytes()


def test_ss_10x5(exe, tmp_path):
    _check(exe, tmp_path, 1, harness.random_model(10, 5, False, 15, draw_c=True), gapped_stream(590, 4, 5))


def test_m1(exe, tmp_path):
    _check(exe, tmp_path, 2, harness.random_model(6, 1, True, 7, draw_c=True), gapped_stream(330, 5, 1))


def test_two_and_three_quad_groups(exe, tmp_path):
    _check(exe, tmp_path, 3, harness.random_model(20, 15, True, 35, draw_c=True), gapped_stream(600, 6, 15))
    _check(exe, tmp_path, 4, harness.random_model(36, 6, False, 42, draw_c=True), gapped_stream(597, 7, 6))


def test_m40(exe, tmp_path):
    _check(exe, tmp_path, 5, harness.random_model(5, 40, True, 45, draw_c=True), gapped_stream(627, 8, 40))


def test_slabs_with_an_overlapping_last_slab(exe, tmp_path):
    """23 motifs as slabs of 10: the last slab is moved back to motifs 13..22 and leaves the seven its neighbour writes
    alone; 80 six-letter motifs single-stranded as slabs of 36 likewise.  dfe adds all columns in ascending k."""
    _check(exe, tmp_path, 0, harness.random_model(23, 15, True, 51, draw_c=True), gapped_stream(603, 13, 15))
    _check(exe, tmp_path, 4, harness.random_model(80, 6, False, 52, draw_c=True), gapped_stream(598, 14, 6), n_random=150)


def test_one_variant_65_variants_and_t_eq_m(exe, tmp_path):
    o = harness.random_model(10, 15, True, 25, draw_c=True)
    stream = gapped_stream(611, 3, 15)
    pos, alt = variant_list(stream, 15, 300, 1)
    full = _run(exe, tmp_path, 0, o, stream, pos, alt)
    inside = int(np.flatnonzero(variant_effects(o, stream, pos, alt)["windows"] == 15)[0])
    one = _run(exe, tmp_path, 0, o, stream, pos[inside:inside + 1], alt[inside:inside + 1])     # V = 1: 63 idle lanes
    _same(one, {k: v[inside:inside + 1] for k, v in full.items()})
    some = _run(exe, tmp_path, 0, o, stream, pos[:65], alt[:65])                                # V = 65: a second tile of one variant
    _same(some, {k: v[:65] for k, v in full.items()})
    check(some, variant_effects(o, stream, pos[:65], alt[:65]), RTOL, "V = 65")
    tm = np.random.default_rng(9).integers(0, 4, size=15, dtype=np.uint8)                        # T = M: one window covers every position
    p = np.arange(15, dtype=np.int64)
    a = ((tm + 1 + p % 3) % 4).astype(np.uint8)
    got = _run(exe, tmp_path, 0, o, tm, p, a)
    check(got, variant_effects(o, tm, p, a), RTOL, "T = M")
    assert np.all(got["windows"] == 1)
    got = _run(exe, tmp_path, 0, o, tm[:14], p[:14], a[:14])                                     # T < M: the bias term alone
    check(got, variant_effects(o, tm[:14], p[:14], a[:14]), RTOL, "T < M")
    assert np.all(got["windows"] == 0) and np.abs(got["dfe"]).max() > 0
    none = _run(exe, tmp_path, 0, o, stream, pos[:0], alt[:0])                                   # V = 0: nothing written
    assert none["dfe"].size == 0


def test_geometries_and_a_reversed_list_give_the_same_bits(exe, tmp_path):
    o = harness.random_model(20, 15, True, 35, draw_c=True)
    stream = gapped_stream(611, 12, 15)
    pos, alt = variant_list(stream, 15, 300, 2)
    got = _run(exe, tmp_path, 3, o, stream, pos, alt)
    for grid, threads in ((1, 256), (3, 64)):
        _same(got, _run(exe, tmp_path, 3, o, stream, pos, alt, grid=grid, threads=threads))
    rev = _run(exe, tmp_path, 3, o, stream, pos[::-1], alt[::-1], grid=3, threads=64)
    _same(got, {k: v[::-1] for k, v in rev.items()})


def test_variant_plan_budget_chunks_and_layout(exe):
    """variant_plan (crbm_sweep.h) is what the driver cuts the list by.  A variant costs its 2M - 1 context bytes, three
    bits per context code, 4 (K + 2) output bytes and its alt byte; the chunk is the budget's share, at least one
    variant, at most the list, at most 2^30 context codes, and within 32 MB unless the budget was set by hand; two
    buffer sets exactly when there is more than one chunk; the layout is scan_layout's of chunk * (2M - 1) codes."""
    def plan(nvar, M, K, budget, was_set):
        out = subprocess.run([exe, "plan"] + [str(x) for x in (nvar, M, K, budget, was_set)], capture_output=True, text=True, timeout=60)
        assert out.returncode == 0, out.stderr
        chunk, nsets, per, valid_words, tiles = (int(x) for x in out.stdout.split())
        CW = 2 * M - 1
        assert per == CW + (3 * CW + 7) // 8 + 4 * (K + 2) + 1
        assert 1 <= chunk <= nvar and chunk * CW <= 1 << 30 and nsets == (2 if chunk < nvar else 1)
        assert valid_words == (chunk * CW + 63) // 64 + 2 and tiles == (chunk + 63) // 64
        return chunk, per
    chunk, per = plan(2022, 15, 10, 256 << 20, 0)
    assert per == 29 + 11 + 48 + 1 and chunk == 2022                                    # config #2: 89 bytes a variant, one chunk
    assert plan(10 ** 6, 15, 10, 256 << 20, 0)[0] == (32 << 20) // 89                    # the 32 MB clamp of the default budget
    assert plan(10 ** 6, 15, 10, 256 << 20, 1)[0] == 10 ** 6                             # ... which a hand-set budget lifts
    assert plan(2022, 15, 10, 1, 1)[0] == 1                                              # CRBM_SLAB_BYTES=1: one variant a chunk
    assert plan(2022, 15, 10, 89 * 300, 1)[0] == 300                                     # 7 chunks
    assert plan(2022, 1, 257, 256 << 20, 0)[1] == 1 + 1 + 4 * 259 + 1
    assert plan((1 << 31) - 1, 64, 1, 1 << 40, 1)[0] == (1 << 30) // 127                 # the 32-bit window starts of a chunk
