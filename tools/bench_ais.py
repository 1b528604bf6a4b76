"""Annealed importance sampling: time per ladder step of all runs, beside the per-step time of the persistent-chain
kernel (crbm_time_gibbs, 16 steps per launch) of a handle with as many chains of the same length, from the same process.
  config #2's model (10 x 15, single-stranded), L = 200, 8192 runs      -- also logPartition(200, 8192, 1000) in seconds
                                                                           and logLikelihood in sequences per second
  config #4's model (50 x 25, single-stranded), L = 1000, 1024 runs
Timing: the ladder is timed through crbm_ais on the host clock -- one call is `steps` ladder steps in launches of
CRBM_AIS_STEPS (hundreds of microseconds to milliseconds each, far above the launch floor) -- after a warm-up call, in
`reps` repeats: minimum and median per step; the time of one launch of CRBM_AIS_STEPS steps follows.  The chain kernel
is timed by the library on the device clock (crbm_time_gibbs).  One JSON line.

usage: python tools/bench_ais.py [reps] [steps]
"""
import ctypes
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from crbm_amd import CRBM  # noqa: E402
from crbm_amd._lib import fptr  # noqa: E402


def ladder_time(m, L, runs, steps, reps):
    betas = np.linspace(0.0, 1.0, steps + 1).astype(np.float32)
    logw = np.empty(runs, np.float32)
    call = lambda: m._call("crbm_ais", L, runs, 0, fptr(betas), betas.size, 0, steps, None, 7, None, fptr(logw))
    call()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        call()
        ts.append((time.perf_counter() - t) / steps)
    return {"us_per_step_min": 1e6 * min(ts), "us_per_step_median": 1e6 * float(np.median(ts)), "steps": steps, "reps": reps}


def chain_time(m, k=16, launches=20):
    ms = ctypes.c_float()
    m._call("crbm_time_gibbs", k, 3, ctypes.byref(ms))          # warm-up
    ts = []
    for _ in range(5):
        m._call("crbm_time_gibbs", k, launches, ctypes.byref(ms))
        ts.append(1e3 * ms.value / (k * launches))
    return {"us_per_step_min": min(ts), "us_per_step_median": float(np.median(ts)), "steps_per_launch": k, "launches": launches}


def case(K, M, L, runs, reps, steps, seed=2026):
    m = CRBM(K, M, doublestranded=False, batchsize=runs, cd_k=1, fantasy_hidden_len=L - M + 1, seed=seed)
    m.motifs.set_value(np.random.default_rng(42).standard_normal((K, 1, 4, M)).astype(np.float32))
    out = {"K": K, "M": M, "L": L, "runs": runs}
    out["chain"] = chain_time(m)
    out["ais"] = ladder_time(m, L, runs, steps, reps)
    out["ais_over_chain"] = out["ais"]["us_per_step_median"] / out["chain"]["us_per_step_median"]
    out["ms_per_launch_of_default_steps"] = 64 * out["ais"]["us_per_step_median"] / 1e3
    return m, out


def main():
    arg = lambda i, d: int(sys.argv[i]) if len(sys.argv) > i else d
    reps, steps = arg(1, 5), arg(2, 256)
    out = {}
    m, out["cfg2_L200_8192_runs"] = case(10, 15, 200, 8192, reps, steps)
    m.logPartition(200, runs=8192, betas=1000)
    ts = []
    for _ in range(3):
        t = time.perf_counter()
        r = m.logPartition(200, runs=8192, betas=1000)
        ts.append(time.perf_counter() - t)
    out["logPartition_200_8192_1000"] = {"seconds_min": min(ts), "seconds_median": float(np.median(ts)), "logZ": r["logZ"],
                                         "stderr": r["stderr"], "ess": r["ess"]}
    codes = np.random.default_rng(1).integers(0, 4, size=(100000, 200), dtype=np.uint8)
    m.logLikelihood(codes, logZ=r["logZ"])
    ts = []
    for _ in range(5):
        t = time.perf_counter()
        m.logLikelihood(codes, logZ=r["logZ"])
        ts.append(time.perf_counter() - t)
    out["logLikelihood_100000x200"] = {"seconds_median": float(np.median(ts)), "sequences_per_s": codes.shape[0] / float(np.median(ts))}
    del m
    _, out["cfg4_L1000_1024_runs"] = case(50, 25, 1000, 1024, reps, max(32, steps // 4))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
