"""The Markov background kernels (crbm_amd/csrc/crbm_background.h) on CPU threads under AddressSanitizer + UBSan:
tests/emu/background_main.cpp, a stand-alone program built here and run directly (no preloaded runtime).  Counts and
samples equal tests/background_reference.py exactly -- every comparison is equality -- at chunk lengths 8 and 64, and
several grids and block sizes give the same bits; what the entry points refuse is refused (the checks are the
header's); guard words around every output must be intact, and every buffer and the LDS are sized to the byte."""
import os
import subprocess

import numpy as np
import pytest

from tests import background_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD, GUARD_WORD = 8, 0xA5A5BEEF


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("emu_background") / "background_main")
    emu = os.path.join(ROOT, "tests", "emu")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g1", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                           "-fno-sanitize-recover=undefined", "-ffp-contract=off", "-mf16c", "-I", os.path.join(emu, "shim"),
                           "-I", emu, "-I", os.path.join(ROOT, "crbm_amd", "csrc"), os.path.join(emu, "background_main.cpp"),
                           "-o", path, "-lpthread"])
    return path


def _run(exe, tmp_path, header, T, pos0, seed, payload, dtype, count, refused=None):
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    if os.path.exists(fout):
        os.unlink(fout)
    with open(fin, "wb") as f:
        f.write(np.array(list(header) + [0] * (8 - len(header)), np.int32).tobytes())
        f.write(np.array([T, pos0], np.int64).tobytes())
        f.write(np.array([seed & (2 ** 64 - 1)], np.uint64).tobytes())
        for a in payload:
            f.write(np.ascontiguousarray(a).tobytes())
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=600)      # the inherited environment, as it is
    if refused is not None:
        assert r.returncode == 3 and refused in r.stderr, (r.returncode, r.stderr[-2000:])
        assert not os.path.exists(fout)                      # nothing was written
        return None
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    raw = np.fromfile(fout, np.uint8)
    size = count * np.dtype(dtype).itemsize
    assert raw.size == 8 * GUARD + size
    guards = np.concatenate([raw[:4 * GUARD], raw[4 * GUARD + size:]]).view(np.uint32)
    assert np.all(guards == GUARD_WORD), "a guard word was written"
    return raw[4 * GUARD:4 * GUARD + size].copy().view(dtype)


def counts(exe, tmp_path, codes, order, grid=2, threads=128, segment=0, **kw):
    codes = np.asarray(codes, np.uint8)
    return _run(exe, tmp_path, [0, order, grid, threads, 0, 0, segment], codes.size, 0, 0, [codes], np.uint64,
                sum(4 ** j for j in range(1, order + 2)) if 0 <= order <= 3 else 0, **kw)


def sample(exe, tmp_path, table, order, template, seed, chunk, pos0=0, grid=2, threads=64, segment=0, **kw):
    has = not isinstance(template, (int, np.integer))
    T = int(np.asarray(template).size if has else template)
    payload = [np.asarray(table, np.uint32)] + ([np.asarray(template, np.uint8)] if has else [])
    return _run(exe, tmp_path, [1, order, grid, threads, chunk, int(has), segment], T, pos0, seed, payload, np.uint8, max(T, 0), **kw)


@pytest.mark.parametrize("order", [0, 1, 2, 3])
def test_counts_equal_the_reference(exe, tmp_path, order):
    s = R.gapped_stream(700, seed=order, gap_share=0.1, max_run=5)
    s[0] = 4                                                     # a gap at the first position and one at the last
    s[-1] = 4
    s[100:110] = [4, 1, 4, 2, 3, 4, 0, 1, 2, 4]                  # runs shorter than order + 1
    want = R.kmer_counts(s, order)
    got = counts(exe, tmp_path, s, order)
    assert np.array_equal(got, want) and got[:4].sum() == (s < 4).sum()
    for grid, threads, segment in ((1, 64, 0), (3, 256, 0), (2, 64, 233), (5, 128, 64)):   # segments: the halo
        assert np.array_equal(counts(exe, tmp_path, s, order, grid=grid, threads=threads, segment=segment), want), (grid, threads, segment)
    t = s[1:-1]                                                  # letters at both ends
    assert np.array_equal(counts(exe, tmp_path, t, order, segment=100), R.kmer_counts(t, order))
    for T in range(0, order + 2):                                # T < order + 1 and T = 0
        short = np.arange(T, dtype=np.uint8) % 4
        assert np.array_equal(counts(exe, tmp_path, short, order), R.kmer_counts(short, order))


def edge_template(T, C, order):
    """gaps at C - 1, C and C + 1 (of three different chunks), a run that begins at a chunk's last position, runs shorter
    than `order`, and random gap runs"""
    s = R.gapped_stream(T, seed=T + C, gap_share=0.03, max_run=4)
    if T > 8 * C:
        s[C - 1] = 4
        s[2 * C] = 4
        s[3 * C + 1] = 4
        s[5 * C - 3:5 * C - 1] = 4                               # ... a run begins at position 5C - 1
        s[5 * C - 1] = 0
        s[6 * C:6 * C + 8] = [4, 0, 4, 1, 2, 4, 3, 4]
        s[9 * C - 1:9 * C + 2] = 4                               # ... and a gap run across a chunk's edge
    return s


TABLES = {0: R.dirichlet_table(0, 10), 1: R.dirichlet_table(1, 11), 2: R.dirichlet_table(2, 12), 3: R.dirichlet_table(3, 13)}


@pytest.mark.parametrize("chunk", [8, 64])
@pytest.mark.parametrize("order", [0, 1, 2, 3])
def test_samples_equal_the_reference_bit_for_bit(exe, tmp_path, order, chunk):
    table = TABLES[order]
    T = 64 * chunk * 2 + chunk + 3                               # three groups of chunks, the last chunk partial
    for template in (T, edge_template(T, chunk, order)):
        want = R.sample(table, order, template, seed=77 + order)
        got = sample(exe, tmp_path, table, order, template, 77 + order, chunk, grid=2, threads=64)
        assert np.array_equal(got, want)
    for grid, threads, segment in ((1, 128, 0), (5, 64, 0), (3, 64, 40 * chunk + 4), (2, 64, 257)):
        other = sample(exe, tmp_path, table, order, template, 77 + order, chunk, grid=grid, threads=threads, segment=segment)
        assert np.array_equal(other, want), (grid, threads, segment)
    for template in (1, np.full(3 * chunk + 1, 4, np.uint8), np.array([4], np.uint8), 0):      # T = 1, all gaps, T = 0
        assert np.array_equal(sample(exe, tmp_path, table, order, template, 5, chunk), R.sample(table, order, template, 5))


@pytest.mark.parametrize("chunk", [8, 64])
def test_tables_with_memory(exe, tmp_path, chunk):
    T = 70 * chunk + 5
    gaps = np.zeros(T, np.uint8)
    gaps[3 * chunk + 2] = 4                                      # one gap: the letter after it starts a new rotation
    for table, order, template in ((R.dirichlet_table(3, 99), 3, T), (R.stuck_table(3), 3, T), (R.stuck_table(3), 3, gaps),
                                   (R.rotation_table(), 1, T), (R.rotation_table(), 1, gaps)):
        want = R.sample(table, order, template, seed=4)
        assert np.array_equal(sample(exe, tmp_path, table, order, template, 4, chunk, grid=3), want)
    rot = R.sample(R.rotation_table(), 1, T, seed=4)
    assert np.all(np.diff(rot.astype(np.int64)) % 4 == 1)        # the whole run hangs on its first letter


def test_pos0_and_seed(exe, tmp_path):
    table = R.dirichlet_table(2, 3)
    pos0 = 2 ** 34 - 6                                           # crosses the carry into counter word 1
    want = R.sample(table, 2, 300, seed=9, pos0=pos0)
    assert np.array_equal(sample(exe, tmp_path, table, 2, 300, 9, 8, pos0=pos0), want)
    assert not np.array_equal(want, R.sample(table, 2, 300, seed=9, pos0=pos0 + 2 ** 34))      # the same word 0, another word 1
    seed = (1 << 63) | 12345
    assert np.array_equal(sample(exe, tmp_path, table, 2, 300, seed, 64), R.sample(table, 2, 300, seed=seed))


def test_refusals(exe, tmp_path):
    s = np.zeros(20, np.uint8)
    for order in (-1, 4):
        counts(exe, tmp_path, s, order, refused="order must lie in [0, 3]")
        sample(exe, tmp_path, np.zeros((1, 3), np.uint32), order, 10, 1, 8, refused="order must lie in [0, 3]")
    bad = s.copy()
    bad[7] = 5
    counts(exe, tmp_path, bad, 2, refused="codes must lie in 0..4")
    sample(exe, tmp_path, TABLES[1], 1, bad, 1, 8, refused="codes must lie in 0..4")
    table = TABLES[1].copy()
    table[2] = [5, 4, 6]
    sample(exe, tmp_path, table, 1, 10, 1, 8, refused="does not ascend")
    sample(exe, tmp_path, TABLES[1], 1, 10, 1, 8, pos0=-1, refused="pos0")
    _run(exe, tmp_path, [0, 1, 2, 64, 0, 0, 0], -1, 0, 0, [], np.uint64, 0, refused="stream length")
    _run(exe, tmp_path, [1, 1, 2, 64, 8, 0, 0], -1, 0, 0, [TABLES[1]], np.uint8, 0, refused="T must lie")
