"""The slab driver of the evaluation sweeps (crbm_amd/csrc/crbm_sweep.h: run_slabs) on the host, under AddressSanitizer
+ UBSan (tests/emu/sweep_driver.cpp records every call of enqueue, collect and drain).  Conditions on the order of calls:
the slabs tile [0, n); every slab is collected once, as it was enqueued; at depth 2 slab i runs on set i & 1 and is
collected after slab i+1 has been enqueued and before slab i+2 is; at depth 1, and in a sweep of one slab, set 0 only
and every slab collected right after it was enqueued; the first error of either callback ends the sweep: nothing more is
enqueued, drain is called once, the error is returned.

The cases run in a subprocess with the sanitizer runtime preloaded: this file is also that subprocess's script."""
import ctypes
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))   # also when run as the child's script
from tests.emu import harness  # noqa: E402

LIB = "libcrbm_sweep_driver.so"
ENQUEUE, COLLECT, DRAIN = 0, 1, 2
# (n, slab): slab >= n (one slab), slab == 1, n a multiple of slab (two, three, many slabs) and not
SHAPES = [(1, 1), (5, 5), (5, 9), (7, 1), (2, 1), (8, 4), (9, 3), (12, 2), (9, 4), (10, 3), (11, 5), (100, 7), (3, 2)]


@pytest.fixture(scope="module")
def emu_env():
    harness.build("sweep_driver.cpp", LIB, kernels=False)
    return harness.child_env()


CASES = ["order_depth2", "order_depth1", "errors_depth2", "errors_depth1"]


@pytest.mark.parametrize("which", CASES)
def test_slab_driver_order_of_calls(emu_env, which):
    r = harness.run_case(os.path.abspath(__file__), which, emu_env, timeout=300)
    assert r.returncode == 0 and "SWEEP OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


# ---- the subprocess side -------------------------------------------------------------------------------------------
def trace(lib, n, slab, depth, fail_kind=-1, fail_slab=-1, fail_code=0):
    """(return code, [(kind, i, set, start, cnt), ...]) of one run_slabs call"""
    cap = 2 * n + 8
    ev = (ctypes.c_int * (5 * cap))()
    nev = ctypes.c_int(0)
    rc = lib.sweep_trace(n, slab, depth, fail_kind, fail_slab, fail_code, ev, cap, ctypes.byref(nev))
    assert nev.value <= cap, (n, slab, depth, nev.value)
    return rc, [tuple(ev[5 * k:5 * k + 5]) for k in range(nev.value)]


def check_order(n, slab, depth, events):
    """the conditions on a sweep (or the part of one before an error): returns the slabs enqueued"""
    what = (n, slab, depth, events)
    enq = [e[1:] for e in events if e[0] == ENQUEUE]
    col = [e[1:] for e in events if e[0] == COLLECT]
    at = {(e[0], e[1]): k for k, e in enumerate(events)}          # (kind, i) -> position in the order of calls
    assert len(at) == len(events), what                           # no slab enqueued or collected twice
    nslabs = (n + slab - 1) // slab
    two = depth == 2 and nslabs > 1
    pos = 0
    for k, (i, s, start, cnt) in enumerate(enq):                  # in order, no gap, no overlap, nothing past n
        assert i == k and start == pos and cnt == min(slab, n - start) and cnt >= 1, what
        assert s == (i & 1 if two else 0), what
        pos += cnt
    assert set(col) <= set(enq) and len(set(col)) == len(col), what   # collected as enqueued, once
    for (i, s, start, cnt) in col:
        c = at[(COLLECT, i)]
        if two:
            # after enqueue(i+1) where there is one (the last slab: after its own), before enqueue(i+2)
            assert c > at[(ENQUEUE, min(i + 1, nslabs - 1))], what
            assert (ENQUEUE, i + 2) not in at or c < at[(ENQUEUE, i + 2)], what
        else:
            assert c == at[(ENQUEUE, i)] + 1, what
    return enq


def run_case(lib, which):
    depth = 2 if which.endswith("2") else 1
    for n, slab in SHAPES:
        nslabs = (n + slab - 1) // slab
        if which.startswith("order"):
            rc, events = trace(lib, n, slab, depth)
            assert rc == 0, (n, slab, depth, rc)
            assert all(e[0] != DRAIN for e in events), (n, slab, depth, events)      # success: never drained
            enq = check_order(n, slab, depth, events)
            assert len(enq) == nslabs and sum(e[3] for e in enq) == n, (n, slab, depth, events)
            assert sorted(e[1:] for e in events if e[0] == COLLECT) == sorted(enq), (n, slab, depth, events)
            continue
        for kind in (ENQUEUE, COLLECT):
            for j in sorted({0, nslabs // 2, nslabs - 1}):       # first, middle, last slab
                code = -(7 + j)
                rc, events = trace(lib, n, slab, depth, kind, j, code)
                what = (n, slab, depth, kind, j, events)
                assert rc == code, what
                assert [e[0] for e in events].count(DRAIN) == 1 and events[-1][0] == DRAIN, what
                assert events[-2][:2] == (kind, j), what          # the failing call was the last one before the drain
                check_order(n, slab, depth, events[:-1])
                # the sweep went as a faultless one up to the failing call
                assert events[:-1] == trace(lib, n, slab, depth)[1][:len(events) - 1], what


if __name__ == "__main__":
    run_case(harness.load(LIB), sys.argv[1])
    print("SWEEP OK")
