"""Every GPU resource of a handle goes with the handle (crbm_amd/csrc/crbm_own.h): the live counters of
crbm_live_resources -- device buffers, their bytes, streams, events, loaded code objects -- are read before a model is
made and after it has been destroyed, and must be equal, exactly.  The cases cover what a handle can own: a specialised
model that is trained for an epoch (the per-epoch evaluation allocates `eval_ones`, which the hand-written list of the
old crbm_destroy had forgotten) and then asked for free energies, hit probabilities, sites, a stream scan and a score
histogram; a generic model with slabs (the slab model's code object, tables and scratch); config #2's shape, whose plain
chain launches run in partitions (worker threads, partition streams, partition events); creates that are refused; and
twenty create/destroy pairs.  Only shapes __graft_entry__.build() precompiles: nothing is compiled here."""
import ctypes
import gc

import numpy as np
import pytest

from crbm_amd import CRBM, _lib

pytestmark = pytest.mark.gpu

SMALL = dict(num_motifs=3, motif_length=3, doublestranded=True, batchsize=4, fantasy_hidden_len=8)
NAMES = ("buffers", "bytes", "streams", "events", "modules")


def live():
    """the live counters now; models that earlier tests dropped without destroying them are collected first"""
    gc.collect()
    counts = (ctypes.c_int64 * 5)()
    assert _lib.load().crbm_live_resources(counts) == 0
    return dict(zip(NAMES, counts))


def destroy(model):
    assert model._handle is not None
    assert model._lib.crbm_destroy(model._handle) == 0
    model._handle = None


def codes(n, L, seed):
    return np.random.default_rng(seed).integers(0, 4, size=(n, L), dtype=np.uint8)


def onehot(c):
    return np.ascontiguousarray(np.eye(4, dtype=np.float32)[c].transpose(0, 2, 1)[:, None])      # (n, 1, 4, L)


def test_specialised_model_trained_and_queried(capsys):
    before = live()
    m = CRBM(epochs=1, seed=7, **SMALL)
    data = codes(8, 12, 1)
    m.fit(data)                                        # one epoch: crbm_train_epoch_resident, crbm_eval_epoch_resident
    held = live()
    assert held["buffers"] > before["buffers"] and held["streams"] == before["streams"] + 2
    assert held["modules"] > before["modules"] and held["events"] > before["events"] and held["bytes"] > before["bytes"]
    assert m.freeEnergy(data).shape == (8,)
    assert m.motifHitProbs(data).shape == (8, 3, 1, 10)
    m.motifSites(data, threshold=0.3)
    stream = codes(1, 200, 2)[0]
    stream[[50, 120]] = 4
    m.scanSites(stream, threshold=0.3)
    assert m.scoreHistogram(stream, bins=16, lo=-8.0, hi=8.0).windows > 0
    destroy(m)
    assert live() == before


def test_generic_model_with_slabs():
    before = live()
    m = CRBM(300, 10, doublestranded=False, fantasy_hidden_len=51, cd_k=1, seed=8)
    data = onehot(codes(20, 60, 3))
    m._trainingFct(data)
    assert m.freeEnergy(data).shape == (20,)
    held = live()
    assert held["modules"] == before["modules"] + 1    # the slab model's kernels: a generic handle has no others
    destroy(m)
    assert live() == before


def test_partitioned_plain_launches():
    before = live()
    m = CRBM(10, 15, doublestranded=False, batchsize=8192, fantasy_hidden_len=186, seed=9)
    info = _lib.CrbmLaunchInfo()
    handle = m._h()
    m._check(m._lib.crbm_get_launch_info(handle, ctypes.byref(info)))
    assert info.chain_parts > 1                        # or nothing below is about partitions
    held = live()
    assert held["streams"] == before["streams"] + 2 + (info.chain_parts - 1)       # stream, stream2, one per further partition
    m.gibbsSteps(1)
    destroy(m)
    assert live() == before


def test_refused_creates(monkeypatch, tmp_path):
    before = live()
    with pytest.raises(Exception, match="device ordinal out of range"):
        CRBM(device=1 << 20, **SMALL)._h()
    assert live() == before
    # refused with the handle half built: its kernels cannot be specialised
    monkeypatch.setenv("CRBM_KERNEL_SRC_DIR", str(tmp_path))
    with pytest.raises(Exception, match="kernel specialisation failed: kernel sources not found in"):
        CRBM(**SMALL)._h()
    assert live() == before
    monkeypatch.delenv("CRBM_KERNEL_SRC_DIR")
    m = CRBM(**SMALL)                                  # and the next create is served
    m._h()
    destroy(m)
    assert live() == before


def test_twenty_creates_and_destroys():
    before = live()
    for i in range(20):
        m = CRBM(seed=i, **SMALL)
        m.gibbsSteps(1)
        destroy(m)
    assert live() == before
