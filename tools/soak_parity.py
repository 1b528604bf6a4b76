"""Randomised parity soak: random model shapes / batch shapes, one PCD-k training step and a
few Gibbs steps against the float64 oracle.  usage: python tools/soak_parity.py [n_cases] [seed]
(test infrastructure: imports the oracle)
The launch structures it draws at random (CRBM_STATS unset / two / split) are pinned, raw sums against the oracle, in tests/test_gpu_statistics.py."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle.crbm_oracle import synthetic_onehot  # noqa: E402
import test_gpu_parity as T  # noqa: E402

if __name__ == "__main__":
    n_cases = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    rng = np.random.default_rng(int(sys.argv[2]) if len(sys.argv) > 2 else 0)
    only = int(os.environ["SOAK_ONLY"]) if "SOAK_ONLY" in os.environ else None   # re-run one case of a seed
    bad = 0
    for case in range(n_cases):
        big = case % 4 == 3                              # every fourth case: large model / long sequences
        beyond = case % 8 == 7                           # every eighth: beyond the specialised kernels (generic path, round 4)
        K = int(rng.integers(1, 401 if beyond else 161 if big else 41))
        M = int(rng.integers(1, 121 if beyond else 65 if big else 29))
        ds = bool(rng.integers(0, 2))
        Lf = int(rng.integers(1, 400 if big else 120))
        B = int(rng.integers(1, 40))
        n = int(rng.integers(1, 40))
        L = M + int(rng.integers(0, 700 if big else 150))
        k = int(rng.integers(1, 4))
        pool = [1, 1, 1, 2, 3, 4][int(rng.integers(0, 6))]         # half of the cases pooled
        Lf = -(-Lf // pool) * pool
        L = M - 1 + max(1, (L - M + 1) // pool) * pool            # hidden length a multiple of pooling
        variant = ["", "dense", "sparse"][int(rng.integers(0, 3))]
        if variant:
            os.environ["CRBM_TOPDOWN"] = variant
        else:
            os.environ.pop("CRBM_TOPDOWN", None)
        stats = ["", "two", "split"][int(rng.integers(0, 3))]      # launch structure of the training step
        if stats:
            os.environ["CRBM_STATS"] = stats
        else:
            os.environ.pop("CRBM_STATS", None)
        bshift, wscale = float(rng.uniform(2, 7)), float(rng.uniform(0.3, 1.5))
        A = 4
        if case % 5 == 4:                                # every fifth: an alphabet other than DNA's (generic kernels, byte rows)
            A = [1, 2, 3, 5, 8, 20, 33, 64][int(rng.integers(0, 8))]
            M = min(M, 2048 // A, 40)
            K = min(K, 60)
            L = M - 1 + max(1, (L - M + 1) // pool) * pool
        akw = {"input_dims": A} if A != 4 else {}
        if only is not None and case != only:
            continue
        t0 = time.time()
        try:
            m, o = T.make_pair(K, M, ds=ds, batchsize=B, cd_k=k, Lf=Lf, bshift=bshift, wscale=wscale, pooling=pool, **akw)
            D = synthetic_onehot(n, L, seed=case, A=A)
            m._trainingFct(D)
            o.train_step(D)
            if only is not None:      # diagnosis of a single case: how many samples of the chain differ?
                hh, hhp = m.get_fantasy()
                vv = m.get_fantasy_visible()
                print("  differing samples: visible %d of %d, hidden %d of %d; max |dW| %.3g" % (
                    int((vv != o.last_v_model).any(axis=2).sum()), vv.shape[0] * vv.shape[3],
                    int((hh != o.fantasy_h).sum()), hh.size, float(np.abs(m.motifs.get_value() - o.W).max())), flush=True)
            tie_note = ""
            try:
                np.testing.assert_allclose(m.motifs.get_value(), o.W, rtol=2e-4, atol=2e-5)
                np.testing.assert_allclose(m.bias.get_value(), o.b, rtol=2e-4, atol=2e-5)
                np.testing.assert_allclose(m.c.get_value(), o.c, rtol=2e-4, atol=2e-5)
            except AssertionError:
                # With a few dozen chains one differing sample moves the model statistics by 1/(chains * Lf):
                # legitimate only if every differing sample of the chain sits on a p == u tie.  Replay the
                # chain of a fresh pair one step at a time from identical states (raises on anything else).
                m2, o2 = T.make_pair(K, M, ds=ds, batchsize=B, cd_k=k, Lf=Lf, bshift=bshift, wscale=wscale, pooling=pool, **akw)
                ties = T.assert_chain_steps(m2, o2, k)
                if ties < 1:
                    raise
                tie_note = " (update differs through %d sample(s) on a p == u tie)" % ties
                m, o = m2, o2
            h, hp = m.get_fantasy()
            mism = float((h != o.fantasy_h).mean())
            assert mism < 2e-3, ("chain mismatch", mism)
            np.testing.assert_allclose(m.freeEnergy(D), o.freeEnergy(D), rtol=2e-4, atol=1e-5)
            P = o.motifHitProbs(D)
            s = m.motifHitSummary(D)
            np.testing.assert_allclose(s["max"], P.max(axis=(2, 3)), rtol=2e-4, atol=1e-6)
            np.testing.assert_allclose(s["position_mean"], P.mean(axis=(0, 2)), rtol=2e-4, atol=1e-6)
            status = "ok" + tie_note
        except Exception as e:   # report every failing shape, keep going
            bad += 1
            status = "FAIL %s" % (str(e)[:300].replace("\n", " "))
        print("case %d K=%d M=%d A=%d ds=%d pool=%d Lf=%d B=%d n=%d L=%d k=%d td=%s stats=%s: %s (%.1fs)" % (
            case, K, M, A, ds, pool, Lf, B, n, L, k, variant or "default", stats or "one", status, time.time() - t0), flush=True)
    print("SOAK DONE, failures:", bad)
    sys.exit(1 if bad else 0)
