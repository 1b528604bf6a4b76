"""Record the chains of the chain kernels as a fixture: tests/golden/chain_parent.npz.

    python tools/record_chain_golden.py [out.npz]        # on a GPU, on the commit whose chains are to be kept

For every shape of SHAPES a model with seeded parameters starts from a seeded hidden state and takes launches of 1, 1 and
3 Gibbs steps (crbm_gibbs_steps); after each launch the packed hidden state of both strands and the letters of the
visible sample are recorded.  The chain kernels run with the launch geometry compiled in (CRBM_GEOM=2) and the recorder
checks that the run-time form (CRBM_GEOM=0) leaves the same words before it writes anything.
tests/test_gpu_chain_golden.py replays the same launches on its own tree and demands exact equality: a change to the
chain kernels that is meant to keep every sample (fewer instructions, another schedule) is held to the chains of the
commit before it.  The fixture is recorded once per intended change of the chains, never to make a test pass."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

# (name, K, M, double-stranded, Lf, chains, chains per tile); __graft_entry__.GOLDEN_SHAPES compiles their kernels
SHAPES = [("ss_186_aligned", 10, 15, False, 186, 8, 4),     # the six of tests/test_gpu_geometry.py: Lv % 4 of 0 and 3, both
          ("ss_185", 10, 15, False, 185, 8, 4),             # state-load paths, both strands, two mask words, a ragged tile
          ("ss_185_word_path", 10, 15, False, 185, 6, 2),
          ("ds_50", 10, 15, True, 50, 6, 2),
          ("two_mask_words", 40, 6, False, 30, 4, 4),
          ("ragged", 10, 15, False, 186, 9, 4),
          ("k7_straddle", 7, 5, False, 20, 4, 2),           # nine masks per window word, one across bit 32 (bits 28..35)
          ("k16_exact", 16, 5, False, 20, 4, 2),            # four masks fill the 64 bits, none across bit 32
          ("k21_three", 21, 5, False, 20, 4, 2)]            # three masks per word, one across bit 32 (bits 21..41)
LAUNCHES = (1, 1, 3)


def run_chain(K, M, ds, Lf, B, S, geom):
    """The records of one shape in one geometry form: a dict of uint8 arrays, keys h<j>, hp<j> (packed bits) and v<j>
    (letters) after launch j."""
    from crbm_amd import CRBM
    knobs = {"CRBM_GIBBS_S": str(S), "CRBM_GEOM": str(geom)}
    saved = {k: os.environ.get(k) for k in knobs}
    os.environ.update(knobs)
    try:
        rng = np.random.default_rng(9000 + 101 * K + 7 * M + Lf + B)
        model = CRBM(K, M, doublestranded=ds, batchsize=B, cd_k=1, fantasy_hidden_len=Lf, seed=11)
        model.motifs.set_value(rng.standard_normal((K, 1, 4, M)).astype(np.float32))
        model.bias.set_value((-3.0 + 0.5 * rng.standard_normal((1, K))).astype(np.float32).reshape(model.bias._shape))
        model.c.set_value((0.3 * rng.standard_normal((1, 4))).astype(np.float32).reshape(model.c._shape))
        h0 = rng.binomial(1, 0.08, size=(B, K, 1, Lf)).astype(np.float32)
        hp0 = rng.binomial(1, 0.08, size=(B, K, 1, Lf)).astype(np.float32) if ds else None
        model.set_fantasy(h0, hp0)
        model.set_rng(gibbs_step=0)
        out = {}
        for j, k in enumerate(LAUNCHES):
            model.gibbsSteps(k)
            h, hp = model.get_fantasy()
            v = model.get_fantasy_visible()
            assert np.all((h == 0) | (h == 1)) and np.all(v.sum(axis=2) == 1)
            out["h%d" % j] = np.packbits(h.astype(np.uint8).ravel())
            if ds:
                out["hp%d" % j] = np.packbits(hp.astype(np.uint8).ravel())
            out["v%d" % j] = np.argmax(v[:, 0], axis=1).astype(np.uint8)
        assert sum(int(np.unpackbits(out["h%d" % j]).sum()) for j in range(len(LAUNCHES))) > 0, "the chains died out"
        return out
    finally:
        for k, val in saved.items():
            if val is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = val


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "chain_parent.npz")
    rec = {}
    for name, K, M, ds, Lf, B, S in SHAPES:
        ct, rt = run_chain(K, M, ds, Lf, B, S, 2), run_chain(K, M, ds, Lf, B, S, 0)
        assert ct.keys() == rt.keys() and all(np.array_equal(ct[k], rt[k]) for k in ct), name + ": the geometry forms differ"
        for k, a in ct.items():
            rec[name + "/" + k] = a
        print("%-18s %6d bits set after the last launch" % (name, int(np.unpackbits(ct["h%d" % (len(LAUNCHES) - 1)]).sum())))
    np.savez_compressed(path, **rec)
    print("wrote %s: %d arrays, %d bytes" % (path, len(rec), os.path.getsize(path)))


if __name__ == "__main__":
    main()
