"""`CRBM` -- the reference's Python surface (secomo/convRBM.py:25-726) over the
HIP C-ABI (include/crbm_amd.h).

Same constructor signature, same validation and messages, same methods
(`fit`, `freeEnergy`, `motifHitProbs`, `getPFMs`, `saveModel`, `loadModel`) and
the `motifs` / `bias` / `c` objects with `get_value()` / `set_value()`; plus
`trainModel` (alias of `fit`, the name BASELINE.json's north_star uses).
Every tensor operation the reference hands to Theano runs in the HIP library;
this file only holds host logic (argument checks, batching, printing, pickles).
"""
import ctypes
import os
import time
import warnings

import joblib
import numpy as np
import scipy.stats

from . import _lib
from ._lib import CrbmConfig, as_f32, fptr
from .sequences import _LUT as _LETTER_LUT          # byte -> code 0..3 for ACGT / acgt, 255 otherwise


_RAW_SITE = np.dtype([("seq", "<i4"), ("motif", "<i4"), ("start", "<i4"), ("strand", "<i4"), ("prob", "<f4")])   # crbm_site


class _DeviceShared(object):
    """Stand-in for a `theano.shared` variable (convRBM.py:133,149,152):
    `get_value()` / `set_value()` on a parameter that lives on the GPU."""

    def __init__(self, model, name, shape):
        self._model = model
        self.name = name
        self._shape = shape

    def get_value(self, borrow=False):
        return self._model._get_param(self.name).copy()

    def set_value(self, value, borrow=False):
        value = as_f32(value)
        if value.shape != self._shape:
            raise ValueError("%s: expected shape %s, got %s" % (self.name, self._shape, value.shape))
        self._model._set_param(self.name, value)

    def __repr__(self):
        return self.name


class CRBM(object):
    """Convolutional RBM for DNA motifs; API of secomo.CRBM (convRBM.py:25-67).

    Parameters follow convRBM.py:68-71.  Keyword-only extras (not in the
    reference): ``fantasy_hidden_len`` (the reference hard-codes the hidden
    length of the persistent chains to 200, convRBM.py:168), ``seed``
    (reference: wall clock, convRBM.py:155) and ``device``.
    """

    def __init__(self, num_motifs, motif_length, epochs=100, input_dims=4,
                 doublestranded=True, batchsize=20, learning_rate=0.1,
                 momentum=0.95, pooling=1, cd_k=5,
                 rho=0.01, lambda_rate=0.1, **extra):
        # sanity checks: convRBM.py:72-108 (same order, same messages)
        if num_motifs <= 0:
            raise Exception("Number of motifs must be positive.")
        if motif_length <= 0:
            raise Exception("Motif length must be positive.")
        if epochs < 0:
            raise Exception("Epochs must be non-negative.")
        if input_dims <= 0:
            raise Exception("input_dims must be positive.")
        elif input_dims != 4:
            warnings.warn("input_dims != 4 was not comprehensively "
                          "tested yet. Be careful when interpreting the results.",
                          UserWarning)
        if batchsize <= 0:
            raise Exception("batchsize must be positive.")
        if learning_rate <= 0.0:
            raise Exception("learning_rate must be positive.")
        if not (momentum >= 0.0 and momentum < 1.):
            raise Exception("momentum must be between zero and one.")
        if pooling <= 0:
            raise Exception("pooling must be positive.")
        if cd_k <= 0:
            raise Exception("cd_k must be positive.")
        if not (rho >= 0.0 and rho < 1.):
            raise Exception("rho must be between zero and one.")
        if lambda_rate < 0.:
            raise Exception("lambda_rate must be non-negative.")

        fantasy_hidden_len = int(extra.pop("fantasy_hidden_len", 200))
        seed = extra.pop("seed", None)
        device = extra.pop("device", None)
        if extra:
            raise TypeError("unexpected keyword arguments: %s" % sorted(extra))
        # The reference takes any positive num_motifs and motif_length (convRBM.py:72-108); so does the library: models
        # beyond its specialised kernels (256 motifs, 64 letters, tables + one chain in the LDS) run on generic ones.
        # What remains is a capacity limit (README "Limits"): refuse at construction, not in the middle of fit().
        if num_motifs > 65536:
            raise Exception("num_motifs > 65536 is not supported.")
        if motif_length > 512:
            raise Exception("motif_length > 512 is not supported.")
        # any alphabet (the reference warns and runs: convRBM.py:84-87); other than DNA's four letters on the generic kernels
        if input_dims > 64:
            raise Exception("input_dims > 64 is not supported.")
        if input_dims * motif_length > 2048:
            raise Exception("input_dims * motif_length > 2048 is not supported.")

        # convRBM.py:111-123
        self.num_motifs = num_motifs
        self.motif_length = motif_length
        self.input_dims = input_dims
        self.doublestranded = doublestranded
        self.batchsize = batchsize
        self.learning_rate = learning_rate
        self.momentum = momentum
        self.rho = rho
        self.lambda_rate = lambda_rate
        self.pooling = pooling
        self.cd_k = cd_k
        self.epochs = epochs
        self.spmethod = 'entropy'
        self.fantasy_hidden_len = fantasy_hidden_len
        self.seed = int(time.time()) if seed is None else int(seed)      # :155
        if device is None:
            device = int(os.environ.get("LOCAL_RANK", "0"))
        self.device = device

        # convRBM.py:127-131: N(0,1) filters from NumPy's global RNG
        W = np.random.randn(num_motifs, 1, input_dims, motif_length).astype(np.float32)
        # convRBM.py:136-140
        if not rho:
            rho = 1. / (self.num_motifs * self.motif_length)
            if self.doublestranded:
                rho = rho / 2.
            self.rho = rho
        # convRBM.py:143-149 (floatX=float32; NumPy 2 would promote, so cast)
        b = (np.zeros((1, num_motifs)) +
             scipy.stats.norm.ppf(self.rho, 0, np.sqrt(motif_length))).astype(np.float32)
        c = np.zeros((1, input_dims), dtype=np.float32)                  # :151
        self._host = {"motifs": W, "bias": b, "c": c}
        self._handle = None
        self._control = None          # crbm_amd.dist.ControlPlane of a data-parallel job
        self._allreduce = None        # "rccl" or "ipc" once crbm_amd.dist.attach has made this model a rank
        self._pending_state = None    # velocities / chains / counters to install when the handle is created
        self.motifs = _DeviceShared(self, "motifs", W.shape)
        self.bias = _DeviceShared(self, "bias", b.shape)
        self.c = _DeviceShared(self, "c", c.shape)
        # data-parallel state (set by crbm_amd.dist.attach)
        self.world_size = 1
        self.rank = 0

    # ------------------------------------------------------------------ device
    def _h(self):
        """The device handle; created on first use.  Replaces the Theano
        compile step (convRBM.py:175, :453-515).  No CPU fallback."""
        if self._handle is not None:
            return self._handle
        lib = _lib.load()
        if self.batchsize % self.world_size != 0:
            raise Exception("batchsize must be divisible by the number of GPUs")
        cfg = CrbmConfig(
            num_motifs=self.num_motifs, motif_length=self.motif_length, input_dims=self.input_dims,
            doublestranded=1 if self.doublestranded else 0,
            batchsize=self.batchsize // self.world_size, cd_k=self.cd_k, pooling=self.pooling,
            fantasy_hidden_len=self.fantasy_hidden_len, learning_rate=self.learning_rate,
            momentum=self.momentum, rho=self.rho, lambda_rate=self.lambda_rate,
            seed=self.seed & 0xFFFFFFFFFFFFFFFF, device=self.device, reserved=0)
        handle = ctypes.c_void_p()
        rc = lib.crbm_create(ctypes.byref(cfg), ctypes.byref(handle))
        if rc != 0:
            raise Exception("crbm_create failed (%d): %s" % (rc, lib.crbm_last_error(None).decode()))
        self._handle = handle
        self._lib = lib
        self._call("crbm_set_params", fptr(self._host["motifs"]), fptr(self._host["bias"]),
                                        fptr(self._host["c"]))
        self._call("crbm_set_shard", self.rank * (self.batchsize // self.world_size))
        if self._pending_state is not None:
            st, self._pending_state = self._pending_state, None
            self._install_state(st)
        return handle

    def _call(self, name, *args):
        h = self._h()
        self._check(getattr(self._lib, name)(h, *args))

    def _check(self, rc):
        if rc != 0:
            raise Exception("HIP CRBM call failed (%d): %s"
                            % (rc, self._lib.crbm_last_error(self._handle).decode()))

    def __del__(self):
        try:
            if getattr(self, "_handle", None) is not None:
                self._lib.crbm_destroy(self._handle)
                self._handle = None
        except Exception:
            pass

    def _get_param(self, name):
        if self._handle is None:
            return self._host[name]
        W = np.empty((self.num_motifs, 1, self.input_dims, self.motif_length), dtype=np.float32)
        b = np.empty((1, self.num_motifs), dtype=np.float32)
        c = np.empty((1, self.input_dims), dtype=np.float32)
        self._check(self._lib.crbm_get_params(self._handle, fptr(W), fptr(b), fptr(c)))
        return {"motifs": W, "bias": b, "c": c}[name]

    def _set_param(self, name, value):
        if self._handle is None:
            self._host[name] = value
            return
        cur = {n: self._get_param(n) for n in ("motifs", "bias", "c")}
        cur[name] = value
        self._check(self._lib.crbm_set_params(self._handle, fptr(cur["motifs"]), fptr(cur["bias"]),
                                              fptr(cur["c"])))

    def _data(self, data):
        data = as_f32(data)
        if data.ndim != 4 or data.shape[1] != 1 or data.shape[2] != self.input_dims:
            raise Exception("expected a one-hot array of shape (n,1,%d,L), got %s" % (self.input_dims, data.shape))
        return data

    @staticmethod
    def _is_codes(data):
        """True for the packed input form: a 2-D uint8 array (n, L) of letter codes 0..input_dims-1
        (DNA: crbm_amd.sequences.seqsToCodes / fastaToCodes)."""
        return isinstance(data, np.ndarray) and data.ndim == 2 and data.dtype == np.uint8

    def _input(self, data):
        """-> (suffix, leading ctypes args, n, L) for the `crbm_*` / `crbm_*_codes` entry points."""
        if self._is_codes(data):
            codes = np.ascontiguousarray(data)
            return "_codes", (codes.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), codes.shape[0], codes.shape[1]), \
                codes.shape[0], codes.shape[1], codes
        data = self._data(data)
        return "", (fptr(data), data.shape[0], data.shape[3]), data.shape[0], data.shape[3], data

    # ------------------------------------------------------------- persistence
    def saveModel(self, filename):
        """convRBM.py:177-204 -- same pickle tuple."""
        numpyParams = (self.motifs.get_value(), self.bias.get_value(), self.c.get_value())
        hyperparams = (self.num_motifs, self.motif_length, self.input_dims, self.doublestranded,
                       self.batchsize, self.learning_rate, self.momentum, self.rho, self.lambda_rate,
                       self.pooling, self.cd_k, self.epochs, self.spmethod)
        joblib.dump((numpyParams, hyperparams), filename, protocol=2)

    @classmethod
    def loadModel(cls, filename):
        """convRBM.py:206-236 -- velocities and chains restart from zero."""
        numpyParams, hyperparams = joblib.load(filename)
        (num_motifs, motif_length, input_dims, doublestranded, batchsize, learning_rate,
         momentum, rho, lambda_rate, pooling, cd_k, epochs, spmethod) = hyperparams
        obj = cls(num_motifs, motif_length, epochs=epochs, input_dims=input_dims,
                  doublestranded=doublestranded, batchsize=batchsize, learning_rate=learning_rate,
                  momentum=momentum, pooling=pooling, cd_k=cd_k, rho=rho, lambda_rate=lambda_rate)
        motifs, bias, c = numpyParams
        obj.motifs.set_value(motifs)
        obj.bias.set_value(bias)
        obj.c.set_value(c)
        return obj

    def _full_state(self):
        """velocities, chains of ALL ranks (bit-packed) and sampler counters; collective in a
        data-parallel job (every rank calls it, every rank gets the global state)."""
        h = self._h()
        seed, gstep, estep = ctypes.c_uint64(), ctypes.c_uint32(), ctypes.c_uint32()
        self._check(self._lib.crbm_get_rng(h, ctypes.byref(seed), ctypes.byref(gstep), ctypes.byref(estep)))
        fh, fhp = self.get_fantasy()
        mine = (np.packbits(fh.astype(np.uint8), axis=None),
                None if fhp is None else np.packbits(fhp.astype(np.uint8), axis=None))
        parts = [mine] if self.world_size == 1 else self._control.gather(mine)
        shape = (self.batchsize, self.num_motifs, 1, self.fantasy_hidden_len)
        per = (self.batchsize // self.world_size) * self.num_motifs * self.fantasy_hidden_len

        def unpack(i):
            if parts[0][i] is None:
                return None
            rows = [np.unpackbits(p[i], count=per) for p in parts]
            return np.packbits(np.concatenate(rows).reshape(shape), axis=3)   # along Lf, one byte per 8 positions
        return {"velocities": self.get_velocities(), "fantasy_bits": (unpack(0), unpack(1)),
                "fantasy_hidden_len": self.fantasy_hidden_len, "world_size": self.world_size,
                "rng": (int(seed.value), int(gstep.value), int(estep.value))}

    def saveState(self, filename):
        """Full training state: the reference tuple of
        saveModel plus velocities, persistent chains and the sampler counters,
        so that training resumes exactly (the reference's loadModel restarts
        momentum and chains from zero, convRBM.py:226-235).  A joblib file whose
        first two entries are the reference's (numpyParams, hyperparams).  In a
        data-parallel job every rank calls it; the chains of all ranks are
        gathered and rank 0 writes the one file, which loads at any world size."""
        numpyParams = (self.motifs.get_value(), self.bias.get_value(), self.c.get_value())
        hyperparams = (self.num_motifs, self.motif_length, self.input_dims, self.doublestranded,
                       self.batchsize, self.learning_rate, self.momentum, self.rho, self.lambda_rate,
                       self.pooling, self.cd_k, self.epochs, self.spmethod)
        extra = self._full_state()
        if self.rank == 0:
            joblib.dump((numpyParams, hyperparams, extra), filename, protocol=2)
        if self._control is not None:
            self._control.barrier()

    @classmethod
    def loadState(cls, filename):
        """Counterpart of saveState.  The device state (velocities, chains, counters) is
        installed when the handle is created, so `crbm_amd.dist.attach()` can still be called
        on the returned model; each rank then takes its own chains out of the global state."""
        numpyParams, hyperparams, extra = joblib.load(filename)
        (num_motifs, motif_length, input_dims, doublestranded, batchsize, learning_rate,
         momentum, rho, lambda_rate, pooling, cd_k, epochs, spmethod) = hyperparams
        seed, gstep, estep = extra["rng"]
        obj = cls(num_motifs, motif_length, epochs=epochs, input_dims=input_dims,
                  doublestranded=doublestranded, batchsize=batchsize, learning_rate=learning_rate,
                  momentum=momentum, pooling=pooling, cd_k=cd_k, rho=rho, lambda_rate=lambda_rate,
                  fantasy_hidden_len=extra["fantasy_hidden_len"], seed=seed)
        motifs, bias, c = numpyParams
        obj.motifs.set_value(motifs)
        obj.bias.set_value(bias)
        obj.c.set_value(c)
        if "fantasy_bits" not in extra:      # files written before the chains were bit-packed
            fh, fhp = extra["fantasy"]
            extra = dict(extra, fantasy_bits=(np.packbits(fh.astype(np.uint8), axis=3),
                                              None if fhp is None else np.packbits(fhp.astype(np.uint8), axis=3)))
        obj._pending_state = {"velocities": extra["velocities"], "fantasy_bits": extra["fantasy_bits"],
                              "rng": (seed, gstep, estep)}
        return obj

    def _install_state(self, st):
        nb = self.batchsize // self.world_size
        lo = self.rank * nb

        def rows(bits):
            if bits is None:
                return None
            if bits.shape[0] != self.batchsize:
                raise Exception("saved state holds %d chains, the model has %d" % (bits.shape[0], self.batchsize))
            return np.unpackbits(bits[lo:lo + nb], axis=3, count=self.fantasy_hidden_len).astype(np.float32)
        self.set_velocities(*st["velocities"])
        fb, fbp = st["fantasy_bits"]
        self.set_fantasy(rows(fb), rows(fbp))
        seed, gstep, estep = st["rng"]
        self.set_rng(seed, gstep, estep)

    # ------------------------------------------- graph builders as plain calls
    def _hgv(self, data, flip, want, rng_step=0):
        data = self._data(data)
        n, L = data.shape[0], data.shape[3]
        shape = (n, self.num_motifs, 1, L - self.motif_length + 1)
        outs = [np.empty(shape, dtype=np.float32) if w else None for w in want]
        self._call("crbm_h_given_v", fptr(data), n, L, 1 if flip else 0,
                                             rng_step, fptr(outs[0]), fptr(outs[1]), fptr(outs[2]))
        return outs

    def _bottomUpActivity(self, data, flip_motif=False):
        """convRBM.py:238-243."""
        return self._hgv(data, flip_motif, (True, False, False))[0]

    def _bottomUpProbabilityOfData(self, data, flip_motif=False):
        """_bottomUpProbability(_bottomUpActivity(data)) (convRBM.py:245-257)."""
        return self._hgv(data, flip_motif, (False, True, False))[1]

    def _computeHgivenV(self, data, flip_motif=False, rng_step=0):
        """convRBM.py:269-275 -> [probability, sample]."""
        o = self._hgv(data, flip_motif, (False, True, True), rng_step)
        return [o[1], o[2]]

    def _vgh(self, h, hprime, want, rng_step=0):
        h = as_f32(h)
        hp = None if hprime is None else as_f32(hprime)
        if h.ndim != 4 or h.shape[1] != self.num_motifs or h.shape[2] != 1:
            raise Exception("expected hidden array of shape (n,K,1,Lh), got %s" % (h.shape,))
        if hp is not None and hp.shape != h.shape:
            raise Exception("h and hprime must have the same shape")
        n, Lh = h.shape[0], h.shape[3]
        shape = (n, 1, self.input_dims, Lh + self.motif_length - 1)
        outs = [np.empty(shape, dtype=np.float32) if w else None for w in want]
        self._call("crbm_v_given_h", fptr(h), fptr(hp), n, Lh, rng_step,
                                             fptr(outs[0]), fptr(outs[1]), fptr(outs[2]))
        return outs

    def _topDownActivity(self, h, hprime=None):
        """convRBM.py:277-292."""
        return self._vgh(h, hprime, (True, False, False))[0]

    def _topDownProbabilityOfHidden(self, h, hprime=None):
        """_topDownProbability(_topDownActivity(h, hprime)) (convRBM.py:294-299)."""
        return self._vgh(h, hprime, (False, True, False))[1]

    def _computeVgivenH(self, H_sample, H_sample_prime=None, rng_step=0):
        """convRBM.py:317-325 -> [probability, sample]."""
        o = self._vgh(H_sample, H_sample_prime, (False, True, True), rng_step)
        return [o[1], o[2]]

    # ------------------------------------------------------------ evaluation
    def _evaluateData(self, data):
        """convRBM.py:517-522 -> [mean free energy, mean of a sampled H]."""
        data = self._data(data)
        mfe, nmh = ctypes.c_float(), ctypes.c_float()
        self._call("crbm_eval_data", fptr(data), data.shape[0], data.shape[3],
                                             ctypes.byref(mfe), ctypes.byref(nmh))
        return [mfe.value, nmh.value]

    def _evaluateParams(self):
        """convRBM.py:528-533 -> [rms(W), IC, median IC]."""
        a, b, c = ctypes.c_float(), ctypes.c_float(), ctypes.c_float()
        self._call("crbm_eval_params", ctypes.byref(a), ctypes.byref(b), ctypes.byref(c))
        return [a.value, b.value, c.value]

    def _trainingFct(self, data):
        """convRBM.py:524-526: one PCD-k update on a mini-batch."""
        data = self._data(data)
        self._call("crbm_train_step", fptr(data), data.shape[0], data.shape[3])

    def motifHitProbs(self, data):
        """convRBM.py:535-547 -> (n,K,1,L-M+1).  `data` is the reference's one-hot
        array or, for data-set scale sweeps, (n,L) uint8 letter codes."""
        suffix, args, n, L, _keep = self._input(data)
        out = np.empty((n, self.num_motifs, 1, L - self.motif_length + 1), dtype=np.float32)
        self._call("crbm_hit_probs" + suffix, *(args + (fptr(out),)))
        return out

    def motifHitSummary(self, data, position_mean=True):
        """The reductions of motifHitProbs() the reference's analysis code takes
        (utils.py:113-116, :154, :242-244, :305), computed on the device without the
        dense (n,K,1,Lh) tensor: dict with 'max' (n,K) = P.max(axis=(2,3)),
        'mean' (n,K) = P.mean(axis=(2,3)), 'position_mean' (K,Lh) = P.mean(axis=(0,2))."""
        suffix, args, n, L, _keep = self._input(data)
        K, Lh = self.num_motifs, L - self.motif_length + 1
        hmax = np.empty((n, K), dtype=np.float32)
        hmean = np.empty((n, K), dtype=np.float32)
        pos = np.empty((K, Lh), dtype=np.float32) if position_mean else None
        self._call("crbm_hit_summary" + suffix, *(args + (fptr(hmax), fptr(hmean),
                                                           fptr(pos) if position_mean else None)))
        out = {"max": hmax, "mean": hmean}
        if position_mean:
            out["position_mean"] = pos
        return out

    # motifSites() records: crbm_site of include/crbm_amd.h, with the strand narrowed to one byte
    SITE_DTYPE = np.dtype([("seq", "<i4"), ("motif", "<i4"), ("start", "<i4"), ("strand", "i1"), ("prob", "<f4")])

    @staticmethod
    def _threshold(threshold):
        t = float(threshold)
        if not 0.0 <= t <= 1.0:          # (NaN too)
            raise ValueError("threshold must lie in [0, 1], got %r" % (threshold,))
        return t

    def _sites_input(self, data):
        """_input() (which checks the one-hot shape) and the sequence length, before any C call."""
        got = self._input(data)
        if got[3] < self.motif_length:
            raise ValueError("sequences of length %d are shorter than motif_length %d" % (got[3], self.motif_length))
        return got

    def motifSites(self, data, threshold=0.5):
        """Where the motifs occur: every (sequence, motif, position, strand) whose probability reaches
        `threshold`, as a NumPy structured array (SITE_DTYPE: seq, motif, start, strand, prob) sorted by
        (seq, motif, start, strand), + before -.  `start` is the 0-based hidden position; the site covers
        letters [start, start + motif_length).  The score is that of motifHitProbs() (convRBM.py:507-514);
        a double-stranded model also reports the reverse-complemented filter (strand -1; motifHitProbs has
        the forward strand only), a single-stranded one has strand 0.  `data`: one-hot or (n, L) uint8 codes.
        The records are gathered on the device without the dense (n,K,1,Lh) tensor; if there are more than
        the first buffer takes, the whole pass is computed once more into a buffer of the exact size."""
        t = self._threshold(threshold)
        suffix, args, n, L, _keep = self._sites_input(data)
        K, Lh = self.num_motifs, L - self.motif_length + 1
        S = 2 if self.doublestranded else 1
        count = ctypes.c_int64(0)

        def call(capacity):
            raw = np.empty(capacity, dtype=_RAW_SITE)
            self._call("crbm_motif_sites" + suffix, *(args + (t, capacity, raw.ctypes.data_as(ctypes.POINTER(_lib.CrbmSite)),
                                                             ctypes.byref(count), None, None, None)))
            return raw
        capacity = min(n * K * S * Lh, max(1 << 20, 4 * n * K))
        raw = call(capacity)
        if count.value > capacity:
            raw = call(count.value)          # more sites than the first buffer took: the pass is computed again
        raw = raw[:count.value]
        out = np.empty(count.value, dtype=self.SITE_DTYPE)
        for f in ("seq", "motif", "start", "strand", "prob"):
            out[f] = raw[f]
        return out

    _SCAN_MAX = 2 ** 31 - 1          # letters one crbm_scan_sites_codes call takes (start is 32 bits wide)

    def _scan_input(self, stream, threshold, offsets):
        """the argument checks of scanSites, before any C call: (threshold, stream, offsets or None)"""
        t = self._threshold(threshold)
        if not isinstance(stream, np.ndarray) or stream.dtype != np.uint8:
            raise ValueError("stream must be a uint8 array of codes 0..4 (sequences.seqsToStream)")
        if stream.ndim != 1:
            raise ValueError("stream must be one-dimensional, got shape %r" % (stream.shape,))
        stream = np.ascontiguousarray(stream)
        if stream.size and int(stream.max()) > 4:
            raise ValueError("stream codes must lie in 0..4 (0..3 = A,C,G,T; 4 = no letter)")
        if offsets is not None:
            offsets = np.asarray(offsets)
            if offsets.ndim != 1 or offsets.size < 1 or not np.issubdtype(offsets.dtype, np.integer):
                raise ValueError("offsets must be a 1-D integer array of record starts (sequences.seqsToStream)")
            offsets = offsets.astype(np.int64)
            if offsets[0] != 0 or np.any(np.diff(offsets) < 1):
                raise ValueError("offsets must start at 0 and ascend (every record is followed by one separator)")
            if offsets.size > 1 and offsets[-1] != stream.size + 1:
                raise ValueError("offsets do not fit the stream: the last entry must be len(stream) + 1")
            if offsets.size == 1 and stream.size:
                raise ValueError("offsets do not fit the stream: no records, but letters")
            if offsets.size > 2 and np.any(stream[offsets[1:-1] - 1] != 4):
                raise ValueError("offsets do not fit the stream: records must be separated by a code 4")
        return t, stream, offsets

    def _scan_call(self, stream, t):
        """crbm_scan_sites_codes over one piece of at most _SCAN_MAX letters: raw records"""
        count = ctypes.c_int64(0)

        def call(capacity):
            raw = np.empty(capacity, dtype=_RAW_SITE)
            self._call("crbm_scan_sites_codes", stream.ctypes.data_as(_lib._U8P), stream.size, t, capacity,
                       raw.ctypes.data_as(ctypes.POINTER(_lib.CrbmSite)), ctypes.byref(count))
            return raw
        capacity = int(min(max(stream.size, 1) * self.num_motifs * 2, max(1 << 20, stream.size // 16)))
        raw = call(capacity)
        if count.value > capacity:
            raw = call(count.value)          # more sites than the first buffer took: the scan is computed again
        return raw[:count.value]

    def _scan_cuts(self, stream, offsets):
        """[lo, hi) of the pieces of at most _SCAN_MAX letters a stream is scanned in, cut at record boundaries"""
        lo = 0
        while True:
            hi = stream.size
            if hi - lo > self._SCAN_MAX:
                if offsets is None:
                    raise ValueError("a stream of more than 2^31 - 1 letters needs offsets (it is cut at record boundaries)")
                i = int(np.searchsorted(offsets, lo + self._SCAN_MAX + 1, side="right")) - 1
                hi = int(offsets[i]) - 1     # the separator in front of record i: the piece ends with the record before
                if hi <= lo:
                    raise ValueError("a record of more than 2^31 - 1 letters cannot be scanned")
            yield lo, hi
            if hi >= stream.size:
                break
            lo = hi + 1

    def scanSites(self, stream, threshold=0.5, offsets=None):
        """motifSites for whole records of any length: `stream` is a 1-D uint8 array of codes, 0..3 = A,C,G,T and
        4 = no letter (N, ambiguity codes, record separators) -- sequences.seqsToStream / fastaToStream make it.  Every
        window of motif_length letters is scored as motifSites scores the same letters in a row (the same bits); a
        window that touches a code 4 yields nothing.  Returns SITE_DTYPE records.  Without `offsets`: seq 0, start the
        stream position, sorted by (start, motif, strand).  With the `offsets` of seqsToStream: seq the record index,
        start relative to the record, sorted by (seq, start, motif, strand), + before - -- saveSites(model, sites,
        "x.bed", names=names) writes them as BED.  Models with pooling, other alphabets or motifs beyond 64 letters are
        refused."""
        t, stream, offsets = self._scan_input(stream, threshold, offsets)
        pieces = [(lo, self._scan_call(stream[lo:hi], t)) for lo, hi in self._scan_cuts(stream, offsets)]
        n = sum(r.size for _, r in pieces)
        out = np.empty(n, dtype=self.SITE_DTYPE)
        pos = np.empty(n, dtype=np.int64)
        at = 0
        for lo, raw in pieces:
            sl = slice(at, at + raw.size)
            for f in ("motif", "strand", "prob"):
                out[f][sl] = raw[f]
            pos[sl] = raw["start"].astype(np.int64) + lo
            at += raw.size
        if offsets is None:
            out["seq"] = 0
            out["start"] = pos
        else:
            seq = np.searchsorted(offsets, pos, side="right") - 1
            out["seq"] = seq
            out["start"] = pos - offsets[seq]
        return out

    def _hist_call(self, stream, lo, hi, bins):
        """crbm_scan_histogram_codes over one piece of at most _SCAN_MAX letters: (counts (K, S, bins) uint64, windows)"""
        S = 2 if self.doublestranded else 1
        counts = np.zeros((self.num_motifs, S, bins), dtype=np.uint64)
        windows = ctypes.c_int64(0)
        self._call("crbm_scan_histogram_codes", stream.ctypes.data_as(_lib._U8P), stream.size, lo, hi, bins,
                   counts.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), ctypes.byref(windows))
        return counts, windows.value

    def scoreHistogram(self, stream, bins=512, lo=-16.0, hi=16.0, offsets=None):
        """The scores scanSites would see on `stream`, as a calibrate.ScoreHistogram: per motif and strand the counts of
        the log-odds x (prob = sigmoid(x)) of every valid window in `bins` equal bins over [lo, hi), the first and the
        last bin open to the outside.  Run it on a background -- sequences.shuffleStream(stream, seed) of the data, or
        background.sampleBackground from a Markov background fitted to it, which keeps the dinucleotide dependence --
        and take per-motif thresholds (thresholds(fpr)) or p-values of scanSites records (pvalues(sites)) from the
        result.  Nothing but the counts leaves the device.  `stream` and `offsets` as in scanSites; lo and hi are
        rounded to float32.  The same models are refused, and more than 1024 bins."""
        _, stream, offsets = self._scan_input(stream, 0.0, offsets)
        if isinstance(bins, bool) or not isinstance(bins, (int, np.integer)) or not 1 <= bins <= 1024:
            raise ValueError("bins must be an integer in [1, 1024]")
        try:
            with np.errstate(over="ignore"):
                lo, hi = float(np.float32(lo)), float(np.float32(hi))
        except (TypeError, ValueError):
            raise ValueError("lo and hi must be numbers")
        if not (np.isfinite(lo) and np.isfinite(hi) and lo < hi):
            raise ValueError("lo and hi must be finite with lo < hi")
        from .calibrate import ScoreHistogram
        S = 2 if self.doublestranded else 1
        counts, windows = np.zeros((self.num_motifs, S, int(bins)), np.int64), 0
        for a, b in self._scan_cuts(stream, offsets):
            c, w = self._hist_call(stream[a:b], lo, hi, int(bins))
            counts += c.astype(np.int64)
            windows += w
        return ScoreHistogram(counts, np.linspace(lo, hi, int(bins) + 1), windows, self.doublestranded)

    def _records_call(self, stream, rec_start):
        """crbm_scan_records_codes over one piece (at most _SCAN_MAX letters, accumulators within the slab budget):
        the dict of recordSummary for its records"""
        R, K = rec_start.size - 1, self.num_motifs
        out = {"windows": np.zeros(R, np.int64), "letters": np.zeros((R, 4), np.int64),
               "per_motif": np.zeros((R, K), np.float32), "fe": np.zeros(R, np.float32),
               "start": np.full((R, K), -1, np.int32), "strand": np.zeros((R, K), np.int32),
               "prob": np.zeros((R, K), np.float32)}
        unit = ctypes.c_double(0.0)
        self._call("crbm_scan_records_codes", stream.ctypes.data_as(_lib._U8P), stream.size,
                   rec_start.ctypes.data_as(_lib._I64P), R, out["windows"].ctypes.data_as(_lib._I64P),
                   out["letters"].ctypes.data_as(_lib._I64P), fptr(out["fe"]), fptr(out["per_motif"]),
                   out["start"].ctypes.data_as(_lib._I32P), out["strand"].ctypes.data_as(_lib._I32P), fptr(out["prob"]),
                   ctypes.byref(unit))
        out["unit"] = unit.value
        return out

    def _records_cuts(self, stream, offsets):
        """[r0, r1) of the records of the pieces a stream is summarised in: _scan_cuts' pieces of at most _SCAN_MAX
        letters, cut again so that the device accumulators of a piece, records * (16 K + 40) bytes (sums and keys per
        motif, the valid windows, four letter counts), stay within the slab budget (CRBM_SLAB_BYTES, or 256 MB)"""
        budget = int(os.environ.get("CRBM_SLAB_BYTES", 256 << 20))
        most = max(1, budget // (16 * self.num_motifs + 40))
        for lo, hi in self._scan_cuts(stream, offsets):
            r0 = int(np.searchsorted(offsets, lo, side="left"))
            r1 = int(np.searchsorted(offsets, hi + 1, side="left"))
            for r in range(r0, r1, most):
                yield r, min(r + most, r1)

    def recordSummary(self, stream, offsets):
        """How well the model explains every record of a stream, and where: freeEnergy and motifBestSites for records of
        any length with N.  `stream` and `offsets` are those of sequences.seqsToStream / fastaToStream (R records,
        R + 1 offsets, one code 4 between two records); `offsets` is required -- a stream without records of its own is
        offsets=[0, len(stream) + 1].  Returns a dict:
          windows   (R,) int64     valid windows of the record: all motif_length codes are letters
          letters   (R, 4) int64   its A, C, G, T
          per_motif (R, K) float32 -sum over its valid windows and the strands of softplus(x_k), x as in variantEffects
                                   (single-stranded models: the forward activation alone).  The hidden part only: the
                                   visible bias is NOT added to every column, unlike freeEnergy(permotif=True) and the
                                   reference's _freeEnergyPerMotif
          fe        (R,) float32   sum_k per_motif[r, k] - sum_a letters[r, a] c[a]: variantEffects' F of the record
                                   alone; L * freeEnergy(codes) for a record of L letters without N
          start, strand, prob (R, K) int32, int8, float32: the best site of every (record, motif) with scanSites'
                                   scores (the same bits), start relative to the record, ties to the smaller start,
                                   then to + (motifBestSites' rule)
          unit      float          the fixed-point unit of the free-energy sums: a window's softplus is rounded to it
                                   once, then integers are added -- the same bits in every run, for every
                                   CRBM_SLAB_BYTES, and the rows of two streams joined by a code 4 are the rows of one
                                   followed by the rows of the other
        A record without a valid window (shorter than motif_length, empty, all N) has windows 0, a per_motif row of
        exact zeros, start -1, strand 0 and prob 0.  The models scanSites refuses are refused."""
        if offsets is None:
            raise ValueError("offsets is required (sequences.seqsToStream; one record: offsets=[0, len(stream) + 1])")
        _, stream, offsets = self._scan_input(stream, 0.0, offsets)
        R = offsets.size - 1
        pieces = [self._records_call(stream[offsets[r0]:offsets[r1] - 1], np.ascontiguousarray(offsets[r0:r1 + 1] - offsets[r0]))
                  for r0, r1 in self._records_cuts(stream, offsets)] if R else []
        if not pieces:
            pieces = [self._records_call(stream, np.zeros(1, np.int64))]
        out = {k: np.concatenate([p[k] for p in pieces]) for k in ("windows", "letters", "per_motif", "fe", "start", "strand", "prob")}
        out["strand"] = out["strand"].astype(np.int8)
        out["unit"] = pieces[0]["unit"]
        return out

    @staticmethod
    def _letter_codes(x, what, V):
        """`what` (alt or ref of variantEffects) as (V,) uint8 codes: a uint8 array of codes, or a string / an array of
        letters ACGT (N and anything else: 255)"""
        if isinstance(x, (str, bytes)):
            x = np.frombuffer(x.encode("latin-1") if isinstance(x, str) else x, dtype=np.uint8)
            codes = _LETTER_LUT[x]
        else:
            x = np.asarray(x)
            if x.dtype == np.uint8:
                codes = x
            elif x.dtype.kind in "US" and x.dtype.itemsize == (4 if x.dtype.kind == "U" else 1):
                flat = np.ascontiguousarray(x).view(np.uint32 if x.dtype.kind == "U" else np.uint8)
                codes = _LETTER_LUT[np.minimum(flat, 255).astype(np.uint8)].reshape(x.shape)
            else:
                raise ValueError("%s must be a uint8 array of codes, or a string or an array of single letters ACGT" % what)
        if codes.ndim != 1 or codes.size != V:
            raise ValueError("%s must hold one entry per variant (%d), got shape %r" % (what, V, codes.shape))
        return np.ascontiguousarray(codes)

    def variantEffects(self, stream, pos, alt, offsets=None, seq=None, ref=None):
        """What single-letter variants change in the model's free energy: dict of 'dfe' (V,) float32, 'per_motif' (V, K)
        float32 and 'windows' (V,) int32.  dfe[i] = F(stream with letter pos[i] replaced by alt[i]) - F(stream), with F
        the free energy of mutagenesis() taken over the valid windows of the stream (a window that touches a code 4 is
        left out, as scanSites leaves it out); per_motif[i, k] is motif k's share of it (the hidden part only:
        dfe = per_motif.sum(1) - (c[alt] - c[ref])), negative where the variant makes the motif fit better; windows[i]
        counts the valid windows around the variant, 0..motif_length.  A variant on a code 4 gives zeros.
        `stream` and `offsets` as in scanSites.  `pos`: integer positions in the stream, or -- with `offsets` and `seq`,
        the record index of every variant -- positions inside record seq[i].  `alt`: a uint8 array of codes 0..3, or a
        string or an array of letters ACGT.  `ref`, when given (codes or letters, N = 4), must be what the stream holds
        at every position: the wrong-assembly check.  Variants may come in any order and may repeat; the outputs follow
        the caller's order.  The same models are refused as in scanSites."""
        _, stream, offsets = self._scan_input(stream, 0.0, offsets)
        pos = np.asarray(pos)
        if pos.ndim != 1 or not (np.issubdtype(pos.dtype, np.integer) or pos.size == 0):
            raise ValueError("pos must be a 1-D integer array")
        pos = pos.astype(np.int64)
        V = pos.size
        alt = self._letter_codes(alt, "alt", V)
        if V and int(alt.max()) > 3:
            raise ValueError("alt must hold letters: codes 0..3 or A, C, G, T")
        if seq is not None:
            if offsets is None:
                raise ValueError("seq needs the offsets of the records")
            seq = np.asarray(seq)
            if seq.shape != pos.shape or not (np.issubdtype(seq.dtype, np.integer) or seq.size == 0):
                raise ValueError("seq must be an integer array with one record index per variant")
            seq = seq.astype(np.int64)
            if V and (seq.min() < 0 or seq.max() >= offsets.size - 1):
                raise ValueError("seq must lie in [0, %d)" % (offsets.size - 1))
            length = offsets[seq + 1] - 1 - offsets[seq]
            bad = np.flatnonzero((pos < 0) | (pos >= length))
            if bad.size:
                raise ValueError("pos outside its record at variants %s" % bad[:5].tolist())
            pos = pos + offsets[seq]
        bad = np.flatnonzero((pos < 0) | (pos >= stream.size))
        if bad.size:
            raise ValueError("pos outside the stream at variants %s" % bad[:5].tolist())
        if ref is not None:
            ref = self._letter_codes(ref, "ref", V)
            ref = np.where(ref > 3, 4, ref).astype(np.uint8)
            bad = np.flatnonzero(ref != stream[pos])
            if bad.size:
                raise ValueError("ref does not match the stream at %d of %d variants, the first at indices %s (another assembly?)"
                                 % (bad.size, V, bad[:5].tolist()))
        K = self.num_motifs
        out = {"dfe": np.zeros(V, np.float32), "per_motif": np.zeros((V, K), np.float32), "windows": np.zeros(V, np.int32)}
        for lo, hi in self._scan_cuts(stream, offsets):
            idx = np.flatnonzero((pos >= lo) & (pos < hi))           # (a separator between two pieces holds no variant's letter: zeros)
            if idx.size == 0:
                continue
            piece = stream[lo:hi]
            p = np.ascontiguousarray(pos[idx] - lo)
            a = np.ascontiguousarray(alt[idx])
            dfe, pm, win = np.empty(idx.size, np.float32), np.empty((idx.size, K), np.float32), np.empty(idx.size, np.int32)
            self._call("crbm_variant_effects_codes", piece.ctypes.data_as(_lib._U8P), piece.size, idx.size,
                       p.ctypes.data_as(_lib._I64P), a.ctypes.data_as(_lib._U8P), fptr(dfe), fptr(pm),
                       win.ctypes.data_as(_lib._I32P))
            out["dfe"][idx], out["per_motif"][idx], out["windows"][idx] = dfe, pm, win
        return out

    @staticmethod
    def _allele_strings(x, what, V):
        """`what` (ref or alt of alleleEffects), a sequence of V strings, as (codes, offsets): the letters of all
        alleles in one uint8 array (ACGT in either case 0..3, N 4, anything else 255) and the int64 offsets (V + 1) of
        every allele in it; "", "-" and "." are empty"""
        if isinstance(x, (str, bytes)) or not hasattr(x, "__len__"):
            raise ValueError("%s must be a sequence of strings, one per variant" % what)
        x = list(x)
        if len(x) != V:
            raise ValueError("%s must hold one entry per variant (%d), got %d" % (what, V, len(x)))
        try:
            text = "".join(x)                                        # (refuses what is no string)
            if "-" in text or "." in text:
                x = ["" if s == "-" or s == "." else s for s in x]
                text = "".join(x)
            off = np.zeros(V + 1, np.int64)
            np.cumsum(np.fromiter(map(len, x), np.int64, V), out=off[1:])
        except TypeError:
            raise ValueError("%s must be a sequence of strings, one per variant" % what)
        try:
            raw = np.frombuffer(text.encode("latin-1"), dtype=np.uint8)
        except UnicodeEncodeError:
            raw = np.full(int(off[-1]), ord("?"), np.uint8)
        lut = _LETTER_LUT.copy()
        lut[ord("N")] = lut[ord("n")] = 4
        return lut[raw], off

    @staticmethod
    def _segments(flat, start, length):
        """the runs flat[start[i] : start[i] + length[i]] back to back, and their offsets (n + 1)"""
        off = np.zeros(start.size + 1, np.int64)
        np.cumsum(length, out=off[1:])
        idx = np.repeat(start - off[:-1], length) + np.arange(int(off[-1]), dtype=np.int64)
        return flat[idx], off

    _ALLELE_MAX = 65535              # letters of a ref or an alt (crbm_allele_effects_codes)

    def alleleEffects(self, stream, pos, ref, alt, offsets=None, seq=None, trim=True):
        """variantEffects for alleles of any length -- insertions, deletions, block substitutions: dict of 'dfe' (V,)
        float32, 'per_motif' (V, K) float32 and 'windows' (V, 2) int32.  Variant i replaces the len(ref[i]) letters
        of the stream from pos[i] on by alt[i]; dfe[i] = F(edited stream) - F(stream) with the F of variantEffects,
        per_motif[i, k] motif k's share of the hidden part (dfe = per_motif.sum(1) - (sum c[alt] - sum c[ref])),
        windows[i] the valid windows of the reference and of the alternative haplotype around the variant.
        `ref` and `alt`: sequences of strings, one per variant; ACGT in either case are letters, N in `ref` is code 4,
        "", "-" and "." are empty (a pure insertion or deletion); any other letter in `alt` is refused.  `ref` is
        always checked against the stream.  `pos`, `seq` and `offsets` as in variantEffects; pos + len(ref) must stay
        inside the record (with `seq`) or the stream.  trim=True removes the longest common prefix of (ref, alt), then
        the longest common suffix, and advances pos by the prefix: the anchor base of a VCF indel goes.  A variant
        that trims to nothing, or whose replaced span holds a code 4, gives zeros.  sequences.readVcf reads the
        arguments from a file.  The same models are refused as in scanSites."""
        _, stream, offsets = self._scan_input(stream, 0.0, offsets)
        pos = np.asarray(pos)
        if pos.ndim != 1 or not (np.issubdtype(pos.dtype, np.integer) or pos.size == 0):
            raise ValueError("pos must be a 1-D integer array")
        pos = pos.astype(np.int64)
        V = pos.size
        rc, ro = self._allele_strings(ref, "ref", V)
        ac, ao = self._allele_strings(alt, "alt", V)
        if rc.size and int(rc.max()) > 4:
            raise ValueError("ref must hold letters A, C, G, T or N")
        if ac.size and int(ac.max()) > 3:
            raise ValueError("alt must hold letters A, C, G, T")
        R, A = np.diff(ro), np.diff(ao)
        if seq is not None:
            if offsets is None:
                raise ValueError("seq needs the offsets of the records")
            seq = np.asarray(seq)
            if seq.shape != pos.shape or not (np.issubdtype(seq.dtype, np.integer) or seq.size == 0):
                raise ValueError("seq must be an integer array with one record index per variant")
            seq = seq.astype(np.int64)
            if V and (seq.min() < 0 or seq.max() >= offsets.size - 1):
                raise ValueError("seq must lie in [0, %d)" % (offsets.size - 1))
            length = offsets[seq + 1] - 1 - offsets[seq]
            bad = np.flatnonzero((pos < 0) | (pos + R > length))
            if bad.size:
                raise ValueError("pos outside its record at variants %s" % bad[:5].tolist())
            pos = pos + offsets[seq]
        bad = np.flatnonzero((pos < 0) | (pos + R > stream.size))
        if bad.size:
            raise ValueError("pos outside the stream at variants %s" % bad[:5].tolist())
        owner = np.repeat(np.arange(V, dtype=np.int64), R)
        at = np.repeat(pos - ro[:-1], R) + np.arange(rc.size, dtype=np.int64)      # the stream position of every ref letter
        bad = np.unique(owner[rc != stream[at]])
        if bad.size:
            raise ValueError("ref does not match the stream at %d of %d variants, the first at indices %s (another assembly?)"
                             % (bad.size, V, bad[:5].tolist()))
        rs, as_ = ro[:-1].copy(), ao[:-1].copy()                                     # (start, length) of every allele in rc / ac
        R, A = R.copy(), A.copy()
        if trim:
            # the common prefix, then the common suffix of what is left: one letter of every allele still in the running
            # per round, so the rounds are as many as the longest common run
            for back in (False, True):
                n, run = np.minimum(R, A), np.zeros(V, np.int64)
                act = np.flatnonzero(n > 0)
                while act.size:
                    at = R[act] - 1 - run[act] if back else run[act]
                    bt = A[act] - 1 - run[act] if back else run[act]
                    act = act[rc[rs[act] + at] == ac[as_[act] + bt]]
                    run[act] += 1
                    act = act[run[act] < n[act]]
                if not back:
                    rs += run; as_ += run; pos += run
                R -= run; A -= run
        bad = np.flatnonzero((R > self._ALLELE_MAX) | (A > self._ALLELE_MAX))
        if bad.size:
            raise ValueError("ref and alt hold at most %d letters each; longer at variants %s" % (self._ALLELE_MAX, bad[:5].tolist()))
        gaps = np.concatenate([[0], np.cumsum(rc == 4)])
        send = ((R > 0) | (A > 0)) & (gaps[rs + R] == gaps[rs])                      # the rest: zeros by definition
        K = self.num_motifs
        out = {"dfe": np.zeros(V, np.float32), "per_motif": np.zeros((V, K), np.float32), "windows": np.zeros((V, 2), np.int32)}
        for lo, hi in self._scan_cuts(stream, offsets):
            idx = np.flatnonzero(send & (pos >= lo) & (pos + R <= hi))
            if idx.size == 0:
                continue
            piece = stream[lo:hi]
            p = np.ascontiguousarray(pos[idx] - lo)
            rl = np.ascontiguousarray(R[idx], np.int32)
            codes, aoff = self._segments(ac, as_[idx], A[idx])
            codes = np.ascontiguousarray(codes, np.uint8)
            dfe, pm, win = np.empty(idx.size, np.float32), np.empty((idx.size, K), np.float32), np.empty((idx.size, 2), np.int32)
            self._call("crbm_allele_effects_codes", piece.ctypes.data_as(_lib._U8P), piece.size, idx.size,
                       p.ctypes.data_as(_lib._I64P), rl.ctypes.data_as(_lib._I32P), aoff.ctypes.data_as(_lib._I64P),
                       codes.ctypes.data_as(_lib._U8P), fptr(dfe), fptr(pm), win.ctypes.data_as(_lib._I32P))
            out["dfe"][idx], out["per_motif"][idx], out["windows"][idx] = dfe, pm, win
        return out

    def motifBestSites(self, data):
        """The best site of every (sequence, motif): dict of 'start' (n,K) int32, 'strand' (n,K) int8 and
        'prob' (n,K) float32 -- the largest probability over positions and strands (motifSites' scores),
        ties to the smaller start, then to +."""
        suffix, args, n, L, _keep = self._sites_input(data)
        K = self.num_motifs
        start = np.empty((n, K), dtype=np.int32)
        strand = np.empty((n, K), dtype=np.int32)
        prob = np.empty((n, K), dtype=np.float32)
        i32 = ctypes.POINTER(ctypes.c_int32)
        self._call("crbm_motif_sites" + suffix, *(args + (0.0, 0, None, None, start.ctypes.data_as(i32),
                                                         strand.ctypes.data_as(i32), fptr(prob))))
        return {"start": start, "strand": strand.astype(np.int8), "prob": prob}

    def mutagenesis(self, data):
        """In-silico mutagenesis: (n, L, input_dims) float32, dF[n, p, a] = F(sequence n with letter p replaced by a)
        - F(sequence n) with F = L * freeEnergy, the unnormalised free energy (convRBM.py:657-676).  The entry of
        the sequence's own letter is exactly 0; negative means the substitution fits the model better.  Only the
        windows that cover p are evaluated; the mutated sequences are never built on the host.
        `data`: one-hot or (n, L) uint8 codes."""
        suffix, args, n, L, _keep = self._sites_input(data)
        out = np.empty((n, L, self.input_dims), dtype=np.float32)
        self._call("crbm_mutagenesis" + suffix, *(args + (fptr(out), None)))
        return out

    def pseudoLogLikelihood(self, data):
        """(n,) float32: sum over positions of log P(v_p | all other letters) = sum_p -log sum_a exp(-dF[n, p, a]) with
        dF of mutagenesis(); <= 0, larger is a better fit.  The dense (n, L, input_dims) array is not formed.
        `data`: one-hot or (n, L) uint8 codes."""
        suffix, args, n, L, _keep = self._sites_input(data)
        out = np.empty((n,), dtype=np.float32)
        self._call("crbm_mutagenesis" + suffix, *(args + (None, fptr(out))))
        return out

    def freeEnergy(self, data, permotif=False):
        """convRBM.py:549-568 -> (n,) or (n,K); one-hot or (n,L) uint8 codes."""
        suffix, args, n, L, _keep = self._input(data)
        out = np.empty((n, self.num_motifs) if permotif else (n,), dtype=np.float32)
        if suffix:
            self._call("crbm_free_energy_codes", *(args + ((None, fptr(out)) if permotif else (fptr(out), None))))
        else:
            self._call("crbm_free_energy_per_motif" if permotif else "crbm_free_energy", *(args + (fptr(out),)))
        return out

    # ------------------------------------------- annealed importance sampling
    @staticmethod
    def _ais_ladder(betas):
        """The ladder as float32: an int T (linspace(0, 1, T + 1)) or an array from 0 to 1 that never decreases."""
        if isinstance(betas, (int, np.integer)) and not isinstance(betas, bool):
            if betas < 1:
                raise ValueError("betas must be at least 1 temperature step, got %r" % (betas,))
            return np.linspace(0.0, 1.0, int(betas) + 1).astype(np.float32)
        b = np.ascontiguousarray(betas, dtype=np.float32)
        if b.ndim != 1 or b.size < 2:
            raise ValueError("betas must be an int or a 1-D array of at least two values")
        if not np.all(np.isfinite(b)) or b[0] != 0.0 or b[-1] != 1.0:
            raise ValueError("betas must start at 0 and end at 1")
        if np.any(np.diff(b) < 0):
            raise ValueError("betas must not decrease")
        return b

    def _ais_base(self, base):
        """cA (A,) float32 of the base-rate model, or None for the model's own c.  `base`: None, a (1,A) / (A,) array
        of biases, or data (letter codes or one-hot) whose letter frequencies with a pseudo-count of 1 give cA."""
        A = self.input_dims
        if base is None:
            return None
        if self._is_codes(base):
            if base.size and base.max() >= A:
                raise ValueError("base holds a letter code outside 0..%d" % (A - 1))
            counts = np.bincount(base.ravel(), minlength=A).astype(np.float64)
        else:
            arr = np.asarray(base)
            if arr.ndim == 4 and arr.shape[1] == 1 and arr.shape[2] == A:
                counts = arr.astype(np.float64).sum(axis=(0, 1, 3))
            elif arr.shape in ((A,), (1, A)) and np.issubdtype(arr.dtype, np.number):
                cA = np.ascontiguousarray(arr.reshape(A), dtype=np.float32)
                if not np.all(np.isfinite(cA)):
                    raise ValueError("base must be finite")
                return cA
            else:
                raise ValueError("base must be None, a (1,%d) or (%d,) array of biases, (n,L) uint8 codes or one-hot "
                                 "data (n,1,%d,L); got shape %s" % (A, A, A, arr.shape))
        freq = (counts + 1.0) / (counts.sum() + A)
        return np.log(freq).astype(np.float32)

    def logPartition(self, L, runs=4096, betas=1000, base=None, seed=None, return_runs=False):
        """log Z of the model for sequences of length L by annealed importance sampling (Salakhutdinov & Murray
        2008): `runs` independent runs from a base-rate model (independent letters with bias cA, `base`) to the
        model over the ladder `betas` of inverse temperatures.  Returns dict(logZ, stderr, ess, logZ_base):
        logZ = logZ_base + log mean exp(logw), stderr its standard error by the delta method
        (std(w) / (mean(w) sqrt(runs))), ess = (sum w)^2 / sum w^2 the effective number of runs, logZ_base the exact
        log partition function of the base-rate model; with return_runs also logw (runs,) float32.
        `betas`: an int T (T equal steps) or an array from 0 to 1; `base`: None (the model's c), a (1,A) / (A,) array,
        or data whose letter frequencies give cA; `seed`: None takes the model's.  Z belongs to a length: the model
        is convolutional.  DNA models on the specialised kernels without pooling."""
        L, runs = int(L), int(runs)
        if runs < 1:
            raise ValueError("runs must be at least 1, got %d" % runs)
        if L < self.motif_length:
            raise ValueError("sequences of length %d are shorter than motif_length %d" % (L, self.motif_length))
        ladder = self._ais_ladder(betas)
        cA = self._ais_base(base)
        seed = self.seed if seed is None else int(seed)
        logw = np.empty(runs, dtype=np.float32)
        self._call("crbm_ais", L, runs, 0, fptr(ladder), ladder.size, 0, ladder.size - 1, fptr(cA),
                   seed & 0xFFFFFFFFFFFFFFFF, None, fptr(logw))
        base_c = (self.c.get_value().reshape(-1) if cA is None else cA).astype(np.float64)
        S = 2 if self.doublestranded else 1
        mx = base_c.max()
        logz_base = L * (mx + np.log(np.exp(base_c - mx).sum())) + S * self.num_motifs * (L - self.motif_length + 1) * np.log(2.0)
        lw = logw.astype(np.float64)
        w = np.exp(lw - lw.max())
        out = {"logZ": float(logz_base + lw.max() + np.log(w.mean())),
               "stderr": float(w.std() / (w.mean() * np.sqrt(runs))),
               "ess": float(w.sum() ** 2 / (w * w).sum()),
               "logZ_base": float(logz_base)}
        if return_runs:
            out["logw"] = logw
        return out

    def logLikelihood(self, data, logZ=None, **ais):
        """(n,) float32: the normalised log-likelihood of every sequence, -L * freeEnergy(v) - logZ.  `logZ`: that of
        logPartition(L) for the data's length L; None computes it (keyword arguments go to logPartition).
        `data`: one-hot or (n, L) uint8 codes."""
        suffix, args, n, L, _keep = self._sites_input(data)
        if logZ is None:
            logZ = self.logPartition(L, **ais)["logZ"]
        elif ais:
            raise TypeError("logZ is given: unexpected keyword arguments %s" % sorted(ais))
        fe = self.freeEnergy(data).astype(np.float64)
        return (-L * fe - float(logZ)).astype(np.float32)

    def getPFMs(self):
        """Position frequency matrices of the filters: per motif a (4,M) float64 array whose
        columns are the softmax of the filter column over the four letters (what
        convRBM.py:640-655 returns; host NumPy there too)."""
        W = self.motifs.get_value().astype(np.float64)[:, 0]      # (K,4,M)
        e = np.exp(W)
        pfm = e / e.sum(axis=1, keepdims=True)
        return [pfm[k] for k in range(self.num_motifs)]

    # --------------------------------------------------------------- training
    def gibbsSteps(self, k=1):
        """Advance the persistent chains by k Gibbs steps (convRBM.py:397-408)
        with the parameters frozen."""
        self._call("crbm_gibbs_steps", int(k))

    def _upload(self, data, slot):
        """Make a data set resident in HBM (packed letters) in the given slot; returns (n, L).  Letter codes travel as they
        are (one byte per base); a float one-hot array is streamed to the device in slabs and encoded -- and checked to be
        exactly one-hot -- there: the PCIe copy of 16 bytes per base is an order of magnitude cheaper than any pass over the
        array on the host (config #1: 3 ms of NumPy for 0.2 ms of copy)."""
        self._call("crbm_dataset_select", slot)
        if self._is_codes(data):
            codes = np.ascontiguousarray(data)
            self._call("crbm_dataset_upload_codes", codes.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)),
                       codes.shape[0], codes.shape[1])
            return codes.shape
        data = self._data(data)
        self._call("crbm_dataset_upload", fptr(data), data.shape[0], data.shape[3])
        return (data.shape[0], data.shape[3])

    def _truncate(self, data):
        """convRBM.py:586-599: truncate so that (L-M+1) % pooling == 0."""
        L = data.shape[-1]
        nseq = int((L - self.motif_length + 1) / self.pooling) * self.pooling + self.motif_length - 1
        return data[..., :nseq]

    def fit(self, training_data, test_data=None):
        """convRBM.py:570-634: epochs x sequential, unshuffled mini-batches;
        one status line per epoch.  Both sets are uploaded once (packed 2-bit)
        and the loops only pass row bounds.  Besides the reference's one-hot
        arrays, (n,L) uint8 letter codes are accepted."""
        training_data = self._truncate(training_data)
        same = test_data is None
        test_data = training_data if same else self._truncate(test_data)

        sharded = self.world_size > 1
        evaluates = self.rank == 0          # data-parallel: rank 0 alone evaluates and prints
        if evaluates:
            print(("BatchSize: " + str(self.batchsize)))
            print("Start training the model...")
        starttime = time.time()
        self._h()
        ntrain = ntest = 0
        if self.epochs > 0:
            ntrain = training_data.shape[0]
            if sharded:
                # each rank uploads only the rows it owns of every mini-batch (1/world of the set)
                from . import dist
                # every rank knows every share: all of them refuse together (a lone raise on the empty
                # rank would leave the others waiting in the all-reduce for ever)
                empty = dist.empty_shards(ntrain, self.batchsize, self.world_size)
                if empty:
                    raise Exception("fewer training rows than ranks: rank(s) %s would own none of the %d rows"
                                    % (empty, ntrain))
                mine = dist.shard_rows(ntrain, self.batchsize, self.rank, self.world_size)
                self._upload(training_data[mine], 0)
                if evaluates:
                    ntest = self._upload(test_data, 1)[0]
            else:
                self._upload(training_data, 0)
                ntest = ntrain if same else self._upload(test_data, 1)[0]
        test_slot = 1 if (sharded or not same) else 0
        for epoch in range(self.epochs):
            self._call("crbm_dataset_select", 0)
            # the batch loop of convRBM.py:612-615 runs inside the library: the steps are
            # enqueued back to back, with one host synchronisation per epoch
            if sharded:
                # All ranks enter an epoch together: rank 0 alone converts and uploads the test set before its first
                # step and alone evaluates after every epoch (below), while the other ranks come straight back here.
                # Without this barrier their update launches would spend that time waiting ON THE DEVICE for rank 0's
                # sums -- a wait that the mapped-buffer all-reduce bounds (CRBM_IPC_TIMEOUT_MS) so that a dead peer
                # cannot hang a GPU.  Host skew belongs on the host: the control plane waits (CRBM_CONTROL_TIMEOUT).
                if self._control is not None:
                    self._control.barrier()
                # (a wait that ran out inside the epoch comes back as CRBM_ERR_IPC_TIMEOUT: no update was applied
                #  after it, the parameters are those of the last complete step)
                self._call("crbm_train_epoch_sharded", self.batchsize, ntrain, int(training_data.shape[-1]))
            else:
                self._call("crbm_train_epoch_resident", self.batchsize)
            if not evaluates:
                continue
            # convRBM.py:616-625 on the resident test set: the loop over its mini-batches (mean free energy and mean
            # sampled activity per batch, averaged over the batches) runs inside the library with one synchronisation
            # -- 50 round trips per epoch at the reference's defaults were 4 of the 6 ms an epoch of config #1 took
            self._call("crbm_dataset_select", test_slot)
            mfe, nmh = ctypes.c_double(), ctypes.c_double()
            self._call("crbm_eval_epoch_resident", self.batchsize, ctypes.byref(mfe), ctypes.byref(nmh))
            self._call("crbm_dataset_select", 0)
            [twn_, ic_, medic_] = self._evaluateParams()
            print(("Epoch {:d}: ".format(epoch) +
                   "FE={:1.3f} ".format(mfe.value) +
                   "NumH={:1.4f} ".format(nmh.value) +
                   "WNorm={:2.2f} ".format(float(twn_)) +
                   "IC={:1.3f} medIC={:1.3f}".format(float(ic_), float(medic_))))
        if evaluates:
            print(("Training finished after: {:5.2f} seconds!".format(time.time() - starttime)))

    # the name BASELINE.json's north_star uses for the same entry point
    trainModel = fit

    def _shard_rows(self, start, end):
        """Rows of mini-batch [start,end) this rank owns (contiguous, balanced)."""
        if self.world_size == 1:
            return start, end
        n = end - start
        lo = start + (n * self.rank) // self.world_size
        hi = start + (n * (self.rank + 1)) // self.world_size
        return lo, hi

    def _iterateBatchIndices(self, totalsize, nbatchsize):
        """convRBM.py:722-726."""
        return [[i, i + nbatchsize] if i + nbatchsize <= totalsize
                else [i, totalsize] for i in range(totalsize)[0::nbatchsize]]

    def __repr__(self):
        """Same text as the reference prints (convRBM.py:704-720): two headed sections, the
        hyper-parameters run together without separators."""
        fields = [("input dims: {:d}", self.input_dims), ("doublestranded: {}", self.doublestranded),
                  ("batchsize: {:d}", self.batchsize), ("learning rate: {:1.3f}", self.learning_rate),
                  ("momentum: {:1.3f}", self.momentum), ("rho: {:1.4f}", self.rho),
                  ("lambda: {:1.3f}", self.lambda_rate), ("pooling: {:d}", self.pooling),
                  ("cd_k: {:d}", self.cd_k), ("epochs: {:d}", self.epochs)]
        head = "Parameters:\n\nNumber of motifs: %s\nMotif length: %s\n\nHyper-parameters:\n\n" \
            % (self.num_motifs, self.motif_length)
        return head + "".join(fmt.format(val) for fmt, val in fields)

    # ------------------------------------------- state the reference never saves
    def get_velocities(self):
        vW = np.empty((self.num_motifs, 1, self.input_dims, self.motif_length), dtype=np.float32)
        vb = np.empty((1, self.num_motifs), dtype=np.float32)
        vc = np.empty((1, self.input_dims), dtype=np.float32)
        self._call("crbm_get_velocities", fptr(vW), fptr(vb), fptr(vc))
        return vW, vb, vc

    def set_velocities(self, vW, vb, vc):
        vW, vb, vc = as_f32(vW), as_f32(vb), as_f32(vc)
        want = ((self.num_motifs, 1, self.input_dims, self.motif_length), (1, self.num_motifs), (1, self.input_dims))
        for name, arr, shape in zip(("vW", "vb", "vc"), (vW, vb, vc), want):
            if arr.shape != shape:          # the C side reads exactly these many floats
                raise ValueError("%s: expected shape %s, got %s" % (name, shape, arr.shape))
        self._call("crbm_set_velocities", fptr(vW), fptr(vb), fptr(vc))

    def get_fantasy(self):
        """(fantasy_h, fantasy_h_prime or None), dense float32 (convRBM.py:168-173)."""
        h = self._h()
        nb = self.batchsize // self.world_size
        shape = (nb, self.num_motifs, 1, self.fantasy_hidden_len)
        a = np.empty(shape, dtype=np.float32)
        b = np.empty(shape, dtype=np.float32) if self.doublestranded else None
        self._call("crbm_get_fantasy", fptr(a), fptr(b))
        return a, b

    def set_fantasy(self, hid, hid_prime=None):
        """This rank's chains: (batchsize / world_size, K, 1, fantasy_hidden_len), exactly 0/1."""
        self._h()
        shape = (self.batchsize // self.world_size, self.num_motifs, 1, self.fantasy_hidden_len)
        hid = as_f32(hid)
        hid_prime = None if hid_prime is None else as_f32(hid_prime)
        for name, arr in (("hid", hid), ("hid_prime", hid_prime)):
            if arr is not None and arr.shape != shape:      # the C side reads exactly B*K*Lf floats
                raise ValueError("%s: expected shape %s, got %s" % (name, shape, arr.shape))
        if self.doublestranded and hid_prime is None:
            raise ValueError("a doublestranded model needs hid_prime")
        self._call("crbm_set_fantasy", fptr(hid), fptr(hid_prime))

    def get_fantasy_visible(self):
        h = self._h()
        nb = self.batchsize // self.world_size
        v = np.empty((nb, 1, self.input_dims, self.fantasy_hidden_len + self.motif_length - 1), dtype=np.float32)
        self._call("crbm_get_fantasy_visible", fptr(v))
        return v

    def get_rng(self):
        """(seed, gibbs_step, eval_step): the sampler's seed and its two step counters (counter word 3 of the chain draws and
        of the evaluation draws)."""
        seed, gstep, estep = ctypes.c_uint64(), ctypes.c_uint32(), ctypes.c_uint32()
        self._call("crbm_get_rng", ctypes.byref(seed), ctypes.byref(gstep), ctypes.byref(estep))
        return seed.value, gstep.value, estep.value

    def set_rng(self, seed=None, gibbs_step=0, eval_step=0):
        if seed is not None:
            self.seed = int(seed)
        self._call("crbm_set_rng", self.seed & 0xFFFFFFFFFFFFFFFF, gibbs_step, eval_step)
