"""The launch plan (crbm_amd/csrc/crbm_plan.h: plan_launches) on the host, under AddressSanitizer + UBSan
(tests/emu/plan_driver.cpp hands it out as plain ints).  crbm_precompile and crbm_create both take their kernels and
geometries from this one function, so what holds of it holds of both.

Invariants, over a grid of models and batches that includes every boundary of the planner (64 / 65 and 256 / 300 motifs,
32 / 33 and 64 / 70 letters, one chain, more chains than a tile holds), at 256 compute units, with the planner's knobs
at their defaults and forced: every geometry that is on is the layout of its model shape, fits the LDS, the tile and the
block sizes the kernels take; the block bound the kernels are compiled with covers every geometry; partitions cover the
batch; generic models have no geometry; slab models are what the slab kernels take.

Recorded plans: for every model __graft_entry__.build() precompiles, what crbm_get_launch_info reports of the plan equals
tests/golden/launch_plans.json, recorded on the MI355X before crbm_plan.h existed.

The cases run in a subprocess with the sanitizer runtime preloaded: this file is also that subprocess's script."""
import ctypes
import itertools
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)   # also when run as the child's script
from tests.emu import harness  # noqa: E402

LIB = "libcrbm_plan_driver.so"
GOLDEN = os.path.join(ROOT, "tests", "golden", "launch_plans.json")
HEAD = ["big", "G", "GS", "has_dense", "chain_parts", "part_chains", "gibbs_wpe", "gibbs_tb", "slab_K", "slab_G", "refused", "NW"]
GEOM = ["threads", "grid", "S", "Lrow", "lds_bytes", "is_layout"]
GEOMS = ["dense", "sparse", "solo", "part"]
# the environment of each case's child
CASES = {
    "invariants": {},
    "invariants_parts1": {"CRBM_CHAIN_PARTS": "1"},
    "invariants_parts3": {"CRBM_CHAIN_PARTS": "3"},
    "invariants_force_big": {"CRBM_FORCE_BIG": "1"},
    "invariants_gibbs_s2": {"CRBM_GIBBS_S": "2"},
    "recorded_default": {},
    "recorded_chain_parts_1": {"CRBM_CHAIN_PARTS": "1"},
    "recorded_topdown_dense": {"CRBM_TOPDOWN": "dense"},
}
KNOBS = ["CRBM_CHAIN_PARTS", "CRBM_FORCE_BIG", "CRBM_GIBBS_S", "CRBM_TOPDOWN", "CRBM_GROUP", "CRBM_GROUP_SOLO", "CRBM_TABLE_BUDGET",
         "CRBM_GIBBS_THREADS", "CRBM_GIBBS_MAX_THREADS", "CRBM_GIBBS_GRID", "CRBM_FUSED_THREADS", "CRBM_SLAB_STATS",
         "CRBM_SLAB_MOTIFS", "CRBM_SLAB_GROUP", "CRBM_SLAB_TABLE_BUDGET"]


@pytest.fixture(scope="module")
def emu_env():
    harness.build("plan_driver.cpp", LIB, kernels=False)
    return harness.child_env()


@pytest.mark.parametrize("which", list(CASES))
def test_launch_plan(emu_env, which):
    env = {k: v for k, v in emu_env.items() if k not in KNOBS}      # the planner's knobs: this case's alone
    env.update(CASES[which])
    r = harness.run_case(os.path.abspath(__file__), which, env, timeout=300)
    assert r.returncode == 0 and "PLAN OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


# ---- the subprocess side -------------------------------------------------------------------------------------------
def plan(lib, K, M, ds, A, pool, Lf, B, num_cu):
    out = (ctypes.c_int * 64)()
    n = lib.plan_ints(K, M, ds, A, pool, Lf, B, num_cu, out)
    assert n == len(HEAD) + len(GEOMS) * len(GEOM)
    p = dict(zip(HEAD, out[:len(HEAD)]))
    for i, name in enumerate(GEOMS):
        at = len(HEAD) + i * len(GEOM)
        p[name] = dict(zip(GEOM, out[at:at + len(GEOM)]))
    return p


def check_invariants(lib):
    grid = itertools.product([1, 2, 10, 64, 65, 100, 256, 300], [1, 4, 15, 32, 33, 64, 70], [0, 1], [1, 2], [4, 20],
                             [1, 4, 20, 512, 8192], [8, 200])
    seen = {"on": 0, "parts": 0, "big": 0, "slab": 0, "solo": 0, "dense": 0}
    for K, M, ds, pool, A, B, Lf in grid:
        what = (K, M, ds, pool, A, B, Lf)
        p = plan(lib, K, M, ds, A, pool, Lf, B, 256)
        what = (what, p)
        on = [p[g] for g in GEOMS if p[g]["threads"] > 0]
        for g in on:
            assert g["is_layout"] == 1, what
            assert g["lds_bytes"] <= 160 * 1024, what
            assert 1 <= g["S"] <= min(B, 64), what
            assert g["threads"] in (64, 128, 256, 512, 1024), what
            assert g["grid"] >= 1, what
            assert g["S"] * g["Lrow"] * p["NW"] < 2 ** 20, what
        assert p["gibbs_tb"] == lib.plan_block_bound(max([g["threads"] for g in on] + [0])), what
        assert (p["dense"]["threads"] > 0) == bool(p["has_dense"] and not p["refused"]), what
        if p["chain_parts"] > 1:
            part = p["part"]
            assert part["threads"] > 0 and p["GS"] == p["G"], what
            assert p["part_chains"] % part["S"] == 0 and p["part_chains"] * p["chain_parts"] >= B, what
        else:
            assert p["part"]["threads"] == 0, what
        if p["big"]:
            assert not on and p["chain_parts"] == 1, what
        else:
            assert p["sparse"]["threads"] > 0 and p["slab_K"] == 0, what
        if p["slab_K"] > 0:
            assert p["big"] and A == 4 and M <= 64 and p["slab_K"] <= 64, what
            assert p["slab_K"] == K or p["slab_K"] % 10 == 0, what
            assert 1 <= p["slab_G"] <= 4, what
        if A != 4 or K > 256 or M > 64:
            assert p["big"], what
        seen["on"] += len(on)
        seen["parts"] += p["chain_parts"] > 1
        seen["big"] += p["big"]
        seen["slab"] += p["slab_K"] > 0
        seen["solo"] += p["solo"]["threads"] > 0
        seen["dense"] += p["dense"]["threads"] > 0
    return seen


def check_recorded(lib, name):
    sys.path.insert(0, ROOT)
    import __graft_entry__ as entry
    with open(GOLDEN) as f:
        golden = json.load(f)
    rows = golden["plans"][name]
    assert [r["config"] for r in rows] == entry.PRECOMPILE         # every model build() precompiles, in its order
    dense = int(os.environ.get("CRBM_TOPDOWN") == "dense")
    for r in rows:
        c = r["config"]
        out = (ctypes.c_int * 7)()
        lib.plan_launch_info(c["num_motifs"], c["motif_length"], int(c.get("doublestranded", 0)), 4, c.get("pooling", 1),
                             c.get("fantasy_hidden_len", 200), c.get("batchsize", 20), golden["num_cu"], dense, out)
        assert dict(zip(golden["fields"], out)) == r["info"], (name, c, list(out), r["info"])


if __name__ == "__main__":
    which = sys.argv[1]
    lib = harness.load(LIB)
    if which.startswith("recorded_"):
        check_recorded(lib, which[len("recorded_"):])
    else:
        seen = check_invariants(lib)
        print(which, seen)
        # the grid reaches what the case is about
        assert seen["big"] > 0 and seen["slab"] > 0
        if which != "invariants_force_big":
            assert seen["on"] > 0 and seen["solo"] > 0 and seen["dense"] > 0
        if which in ("invariants", "invariants_parts3"):
            assert seen["parts"] > 0
        if which == "invariants_parts1":
            assert seen["parts"] == 0
    print("PLAN OK")
