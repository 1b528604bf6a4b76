"""The owners of GPU resources (crbm_amd/csrc/crbm_own.h) on the CPU under AddressSanitizer + UBSan: tests/emu/own_main.cpp,
a stand-alone program built here and run directly (no preloaded runtime, no HIP runtime).  It defines counting stand-ins
for the HIP calls the header makes -- malloc'ed memory for allocations, tagged dummy handles for streams, events, code
objects and mapped peer buffers, a journal of every create and destroy, the n-th call of a kind failing on demand -- and
holds the owners to what crbm_api.hip relies on: the growth rule of ensure, an empty owner after a failed allocation, one
owner per resource after moves and swaps, one release however often it is asked for, the order in which a partition goes
(thread joined, stream synchronised and destroyed, event destroyed; the main stream stays), and live counters that an
early return leaves where they were.  Every case ends with all counters at zero and every block freed exactly once."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ["ensure_grows_by_the_rule", "failed_ensure_leaves_the_owner_empty", "exact_zeroed_and_fine_grained",
         "moves_leave_one_owner", "release_then_destruction_frees_once", "partition_goes_thread_then_stream_then_event",
         "early_return_frees_what_the_function_held", "peers_close_what_was_opened_and_not_the_own_buffer"]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("emu_own") / "own_main")
    emu = os.path.join(ROOT, "tests", "emu")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g1", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                           "-fno-sanitize-recover=undefined", "-Wall", "-Werror", "-I", os.path.join(emu, "own_shim"),
                           "-I", os.path.join(ROOT, "crbm_amd", "csrc"), os.path.join(emu, "own_main.cpp"), "-o", path, "-lpthread"])
    return path


@pytest.mark.parametrize("case", CASES)
def test_owner(exe, case):
    r = subprocess.run([exe, case], capture_output=True, text=True, timeout=120)      # the inherited environment, as it is
    assert r.returncode == 0 and r.stdout.strip() == "ok " + case, r.stdout[-2000:] + r.stderr[-4000:]


def test_every_case_of_the_program_is_run_here_and_in_one_process(exe):
    r = subprocess.run([exe, "all"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stdout.split() == [w for c in CASES for w in ("ok", c)]
    assert subprocess.run([exe, "no_such_case"], capture_output=True).returncode == 2


def test_only_the_owners_release_hip_resources():
    """the structure the owners exist for: no other file of csrc frees, destroys, unloads or closes anything"""
    csrc = os.path.join(ROOT, "crbm_amd", "csrc")
    calls = ("hipFree(", "hipEventDestroy(", "hipStreamDestroy(", "hipModuleUnload(", "hipIpcCloseMemHandle(")
    for name in sorted(os.listdir(csrc)):
        if name.endswith((".h", ".hip")) and name != "crbm_own.h":
            text = open(os.path.join(csrc, name)).read()
            assert not [c for c in calls if c in text], name
    own = open(os.path.join(csrc, "crbm_own.h")).read()
    assert all(c in own for c in calls)
