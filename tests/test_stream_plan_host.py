"""The segment plan of the stream sweeps (crbm_amd/csrc/crbm_sweep.h: stream_plan, handed out by run_slabs) on the host:
tests/emu/stream_plan_main.cpp, a stand-alone program built here with AddressSanitizer + UBSan and run directly.
For streams from T == M to 2^31 - 1 letters, models of one and five slabs, and three budgets each -- the default, one
that gives exactly 7 segments, one whose segment edge falls inside a window -- the segments tile [0, T - M + 1) without
gap or overlap, every segment's letters [start, start + cnt + M - 1) lie inside [0, T), the layout of a full segment is
at least that of every actual segment in all three fields, two buffer sets exactly when there is more than one segment,
and at the default budget the segment size is what the drivers computed inline before stream_plan existed."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULT_BUDGET = 256 << 20
# (T, M): a single window, two windows, an odd length with a long and with a one-letter motif, more than one default
# segment, the longest stream with the longest motif
STREAMS = [(15, 15), (16, 15), (5003, 15), (5003, 1), ((1 << 24) + 1000, 15), ((1 << 31) - 1, 64)]
NSLAB = [1, 5]


def per_start(nslab):
    return 4 + 4 * nslab


def inline_seg(T, M, nslab):
    """the segment size of the default budget as scan_sites_any and scan_hist_any each computed it: slab_rows of the
    256 MB budget, then the 32 MB clamp that only a hand-set CRBM_SLAB_BYTES lifts"""
    starts_all = T - M + 1
    rows = DEFAULT_BUDGET // max(per_start(nslab), 1)
    if rows < 1:
        rows = 1
    seg = min(rows, starts_all)
    return min(seg, max(1, (32 << 20) // per_start(nslab)))


def budgets(T, M, nslab):
    """(name, budget, budget_was_set, segments expected or None)"""
    starts = T - M + 1
    # 7 segments: segments of ceil(starts / 7) starts.  Fewer than 7 starts cannot make 7 segments: one start each then.
    seg7 = -(-starts // 7)
    n7 = -(-starts // seg7)
    assert n7 == (7 if starts >= 7 else starts)
    # an edge inside a window: two segments that meet in the middle of the stream, off the tile grid; the windows that
    # start less than M - 1 before the edge reach across it (M == 1 has no such window, a single start no edge)
    half = starts // 2 + 1
    if half % 64 == 0:
        half += 1
    half = min(half, starts)
    return [("default", DEFAULT_BUDGET, 0, None),
            ("seven", per_start(nslab) * seg7, 1, n7),
            ("edge", per_start(nslab) * half, 1, 2 if half < starts else 1)]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("stream_plan") / "stream_plan_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g1", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                           "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "crbm_amd", "csrc"),
                           os.path.join(ROOT, "tests", "emu", "stream_plan_main.cpp"), "-o", path])
    return path


@pytest.mark.parametrize("nslab", NSLAB)
@pytest.mark.parametrize("T,M", STREAMS)
def test_stream_plan(exe, T, M, nslab):
    starts = T - M + 1
    for name, budget, was_set, want_segments in budgets(T, M, nslab):
        what = (T, M, nslab, name)
        r = subprocess.run([exe, str(T), str(M), str(nslab), str(budget), str(was_set)], capture_output=True, text=True,
                           timeout=300)                                                # the inherited environment, as it is
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        lines = [tuple(int(x) for x in line.split()) for line in r.stdout.splitlines()]
        (starts_all, seg, nsets, *full), segments = lines[0], lines[1:]
        assert starts_all == starts and 1 <= seg <= starts, what
        if name == "default":
            assert seg == inline_seg(T, M, nslab), what
        else:
            assert seg == budget // per_start(nslab) and len(segments) == want_segments, what
        assert len(segments) == -(-starts // seg), what
        pos = 0
        for i, (s, start, cnt, *layout) in enumerate(segments):
            assert start == pos and 1 <= cnt <= seg, what                              # no gap, no overlap
            assert 0 <= start and start + cnt + M - 1 <= T, what                       # the halo is inside the stream
            assert all(f >= l for f, l in zip(full, layout)) and len(layout) == 3, what
            assert s == (i & 1), what
            pos += cnt
        assert pos == starts, what
        assert nsets == (2 if len(segments) > 1 else 1), what
        if name == "edge" and len(segments) == 2 and M > 1:
            edge = segments[1][1]
            assert edge % 64 != 0 and edge - (M - 1) >= 0 and edge < starts, what     # windows [edge - M + 1, edge) span it
