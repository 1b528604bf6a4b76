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
SAMPLER_SEED = 11      # the sampler seed (the Philox key) of every recorded chain

# tests/golden/chain_exact_path.npz (tests/test_gpu_chain_exact_path.py): chains long enough that the exact path of the
# hidden sampler -- entered by 2^-12 of all units -- sees every one of the ten 12-bit field slots of a Philox call, on
# both strands where there are two.  The last entry is the sampler seed (the Philox key), chosen with exact_path_census
# below on the CPU: tests/test_chain_exact_path_census.py holds the recorded run to at least two undecided units per slot.
# __graft_entry__.EXACT_PATH_SHAPES compiles their kernels.
EXACT_PATH_SHAPES = [("k10_ss_186_x32", 10, 15, False, 186, 32, 4, SAMPLER_SEED),    # the sampler resolves its units in the wave
                     ("k21_ds_64_x32", 21, 8, True, 64, 32, 2, SAMPLER_SEED)]         # ... queues them per block; three groups, the last of one unit
# the second shape once more with sample_hidden's own exact path in place of the block queue (crbm_kernels.h, gibbs_body)
INLINE_EXACT_PATH_DEFINES = "-DCRBM_INLINE_EXACT_PATH"


def chain_inputs(K, M, ds, Lf, B):
    """Seeded parameters and start state of one shape: (W, b, c, h0, hp0), float32, hp0 None on one strand."""
    rng = np.random.default_rng(9000 + 101 * K + 7 * M + Lf + B)
    W = rng.standard_normal((K, 1, 4, M)).astype(np.float32)
    b = (-3.0 + 0.5 * rng.standard_normal((1, K))).astype(np.float32)
    c = (0.3 * rng.standard_normal((1, 4))).astype(np.float32)
    h0 = rng.binomial(1, 0.08, size=(B, K, 1, Lf)).astype(np.float32)
    hp0 = rng.binomial(1, 0.08, size=(B, K, 1, Lf)).astype(np.float32) if ds else None
    return W, b, c, h0, hp0


def exact_path_census(K, M, ds, Lf, B, seed=SAMPLER_SEED, steps=sum(LAUNCHES)):
    """The undecided units of the same chain on the CPU, by the float64 oracle and its sampler: counts[strand, slot] of
    the units whose coarse 12-bit field equals floor(4096 P) -- those the coarse tests of sample_hidden leave open --
    over all steps of the launches; slot = unit % 10 is the field of the Philox call the unit draws."""
    from oracle.crbm_oracle import OracleCRBM, hidden_uniforms, visible_uniforms, KIND_CHAIN_H, KIND_CHAIN_V
    W, b, c, h, hp = chain_inputs(K, M, ds, Lf, B)
    o = OracleCRBM(K, M, doublestranded=ds, batchsize=B, cd_k=1, fantasy_hidden_len=Lf, seed=seed, W=W)
    o.b, o.c = b.astype(np.float64), c.astype(np.float64)
    idx = np.arange(B)
    counts = np.zeros((2 if ds else 1, 10), dtype=np.int64)
    slot = np.arange(K) % 10
    for t in range(steps):
        _, v = o._computeVgivenH(h, hp, visible_uniforms(seed, t, idx, Lf + M - 1, KIND_CHAIN_V))
        new = []
        for strand in range(2 if ds else 1):
            u = hidden_uniforms(seed, t, idx, K, Lf, strand, KIND_CHAIN_H)
            P, hs = o._computeHgivenV(v, bool(strand), u)
            coarse = np.floor(u * 4096.0)                     # u = (coarse * 4096 + fine) / 2^24
            open_ = np.floor(P * 4096.0) == coarse
            counts[strand] += np.bincount(np.broadcast_to(slot[None, :, None, None], open_.shape)[open_], minlength=10)
            new.append(hs)
        h, hp = new[0], (new[1] if ds else None)
    return counts


def run_chain(K, M, ds, Lf, B, S, geom, seed=SAMPLER_SEED):
    """The records of one shape in one geometry form: a dict of uint8 arrays, keys h<j>, hp<j> (packed bits) and v<j>
    (letters) after launch j."""
    from crbm_amd import CRBM
    knobs = {"CRBM_GIBBS_S": str(S), "CRBM_GEOM": str(geom)}
    saved = {k: os.environ.get(k) for k in knobs}
    os.environ.update(knobs)
    try:
        W, b, c, h0, hp0 = chain_inputs(K, M, ds, Lf, B)
        model = CRBM(K, M, doublestranded=ds, batchsize=B, cd_k=1, fantasy_hidden_len=Lf, seed=seed)
        model.motifs.set_value(W)
        model.bias.set_value(b.reshape(model.bias._shape))
        model.c.set_value(c.reshape(model.c._shape))
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
    # python tools/record_chain_golden.py --exact-path [out.npz] records EXACT_PATH_SHAPES into chain_exact_path.npz
    args = [a for a in sys.argv[1:] if a != "--exact-path"]
    exact = len(args) != len(sys.argv) - 1
    path = args[0] if args else os.path.join(ROOT, "tests", "golden", "chain_exact_path.npz" if exact else "chain_parent.npz")
    rec = {}
    for name, K, M, ds, Lf, B, S, seed in (EXACT_PATH_SHAPES if exact else [s + (SAMPLER_SEED,) for s in SHAPES]):
        ct, rt = run_chain(K, M, ds, Lf, B, S, 2, seed), run_chain(K, M, ds, Lf, B, S, 0, seed)
        assert ct.keys() == rt.keys() and all(np.array_equal(ct[k], rt[k]) for k in ct), name + ": the geometry forms differ"
        for k, a in ct.items():
            rec[name + "/" + k] = a
        print("%-18s %6d bits set after the last launch" % (name, int(np.unpackbits(ct["h%d" % (len(LAUNCHES) - 1)]).sum())))
    np.savez_compressed(path, **rec)
    print("wrote %s: %d arrays, %d bytes" % (path, len(rec), os.path.getsize(path)))


if __name__ == "__main__":
    main()
