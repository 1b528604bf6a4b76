"""TEST INFRASTRUCTURE shared by the sanitizer tests (tests/test_emu*.py, tests/test_sweep_host.py, tests/test_plan_host.py): builds a driver of
this folder into a library with ASan + UBSan, gives the environment of the child process that loads it, runs one case
of a test file in such a child, and holds what the children themselves share (ctypes pointers, a model's table image,
the random model of a case).  A plain module: every test file imports it (as tests.emu.harness, with the repository
root on sys.path), as a test and as the child's script."""
import ctypes
import glob
import os
import subprocess
import sys

import numpy as np

EMU = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(EMU))
CSRC = os.path.join(ROOT, "crbm_amd", "csrc")


def _gcc_file(name):
    return subprocess.check_output(["gcc", "-print-file-name=" + name], text=True).strip()


def build(driver, libname, kernels=True):
    """Compiles tests/emu/<driver> into tests/emu/<libname> unless the library is newer than the driver and every
    header of this folder (the shim included) and of crbm_amd/csrc.  kernels=False: a driver of host code alone, which
    needs neither the shim nor F16C."""
    src, lib = os.path.join(EMU, driver), os.path.join(EMU, libname)
    inputs = [src] + glob.glob(os.path.join(EMU, "**", "*.h"), recursive=True) + glob.glob(os.path.join(CSRC, "*.h"))
    if not os.path.exists(lib) or any(os.path.getmtime(s) > os.path.getmtime(lib) for s in inputs):
        cmd = ["g++", "-std=c++17", "-O1", "-g1", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
               "-fno-sanitize-recover=undefined", "-fPIC", "-shared"]
        cmd += ["-mf16c", "-I", os.path.join(EMU, "shim")] if kernels else []
        subprocess.check_call(cmd + ["-I", CSRC, src, "-o", lib, "-lpthread"])


def child_env():
    """the environment of a process that loads such a library: the sanitizer runtimes come first"""
    env = dict(os.environ)
    env["LD_PRELOAD"] = _gcc_file("libasan.so") + ":" + _gcc_file("libubsan.so")
    env["ASAN_OPTIONS"] = "detect_leaks=0:abort_on_error=1"
    return env


def run_case(script, which, env, timeout):
    """one named case of `script` in a child process; the caller asserts on the completed process"""
    return subprocess.run([sys.executable, script, which], env=env, capture_output=True, text=True, timeout=timeout)


# ---- the child's side ------------------------------------------------------------------------------------------------
def load(libname):
    return ctypes.CDLL(os.path.join(EMU, libname))


def fp(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def case_info(info_fn, cid):
    """what a driver's emu_<x>_info reports of configuration `cid`: K, M, DS first, then the driver's own (zero-padded)"""
    info = (ctypes.c_int * 8)()
    assert info_fn(cid, info) == 0
    return list(info)


def model_tables(info_fn, tables_fn, cid, o, tables_at):
    """the table image of oracle model `o` under configuration `cid`, built by the driver's emu_<x>_tables; the size is
    entry `tables_at` of its emu_<x>_info"""
    info = case_info(info_fn, cid)
    K, M = info[:2]
    assert info[:3] == [o.num_motifs, o.motif_length, int(bool(o.doublestranded))]
    W = np.ascontiguousarray(o.W.reshape(K, 4, M), dtype=np.float32)
    b = np.ascontiguousarray(o.b.ravel(), dtype=np.float32)
    c = np.ascontiguousarray(o.c.ravel(), dtype=np.float32)
    tables = np.zeros(info[tables_at], np.float32)
    tables_fn(cid, fp(W), fp(b), fp(c), fp(tables))
    return tables


def random_model(K, M, ds, seed, pool=1, A=4, draw_c=False):
    """the oracle model of a case: N(0, 0.7^2) weights, hidden biases shifted by 3 (livelier hidden units) and, with
    draw_c, visible biases of their own"""
    from oracle.crbm_oracle import OracleCRBM
    rng = np.random.default_rng(seed)
    o = OracleCRBM(K, M, doublestranded=ds, batchsize=4, cd_k=1, fantasy_hidden_len=20, seed=1, pooling=pool, input_dims=A,
                   W=rng.standard_normal((K, 1, A, M)).astype(np.float32) * 0.7)
    o.b = (o.b + 3.0 + rng.standard_normal((1, K)) * 0.5).astype(np.float32).astype(np.float64)
    if draw_c:
        o.c = (rng.standard_normal((1, A)) * 0.3).astype(np.float32).astype(np.float64)
    return o
