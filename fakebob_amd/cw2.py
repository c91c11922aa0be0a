"""CW2: Carlini-Wagner's L2 white-box attack (SpeakerGuard's CW2) on the engine's own systems, behind FakeBob's interface.

FakeBob's NES, the particle swarm and PGD spend a fixed epsilon budget; CW2 MINIMISES the distortion: it answers "how small
a perturbation breaks this system".  The attack runs in tanh space (x = tanh(w0 + mod) stays inside [-1, 1] without a clip),
descends c * max(loss, 0) + |x - a0|^2 with Adam on the analytic gradient of the loss (fb_attack_cw2; the contract and its
pseudo-code are in include/fakebob_hip.h), does not stop at the first success but keeps the smallest successful iterate, and
bisects the trade-off constant c over binary_search_steps runs of max_iter iterations each.  `confidence` is CW's kappa: it
is FakeBob's adver_thresh, inside loss_fn.  Success is FakeBob's own test, adver_loss < 0 on the int16 row that was scored.

Victims: an undefended GMM-UBM system; with ivector=True an i-vector-PLDA system (Engine.set_wb_ivector); with xvector=True an
x-vector (TDNN) system (Engine.set_wb_xvector; eot_size > 1 with bpda=True as on a GMM-UBM system); with bpda=True a
victim behind an input-transform chain or a codec, and with eot_size = r > 1 the expectation over r draws of its random
stages (Engine.set_wb_bpda, Engine.set_eot).  Companions, an air channel, feature compression and dither are refused by the
engine in this version, whatever the other white-box switches say.
"""
import functools
import math
import pickle
import time

import numpy as np

from .attack import FakeBob, _check_bits, _col
from .engine import cw2_params, nes_params


def check_cw2_params(initial_const, binary_search_steps, max_iter, lr, stop_early_iter, eot_size=1, bpda=False):
    """The limits of fb_attack_cw2 and of the constructor's switches, as ValueError before anything reaches the library."""
    if not 1 <= int(binary_search_steps) <= 32:
        raise ValueError("CW2: binary_search_steps %d outside 1 .. 32" % int(binary_search_steps))
    for name, v in (("initial_const", initial_const), ("lr", lr)):
        if not (math.isfinite(float(v)) and float(v) > 0.0):
            raise ValueError("CW2: %s must be finite and > 0 (got %r)" % (name, v))
    if int(max_iter) < 1:
        raise ValueError("CW2: max_iter must be >= 1")
    if int(binary_search_steps) * int(max_iter) > 2 ** 30:
        raise ValueError("CW2: binary_search_steps * max_iter above 2^30")
    if int(stop_early_iter) < 1:
        raise ValueError("CW2: stop_early_iter must be >= 1 (stop_early=False switches the rule off)")
    if not 1 <= int(eot_size) <= 32:
        raise ValueError("CW2: eot_size %d outside 1 .. 32" % int(eot_size))
    if int(eot_size) > 1 and not bpda:
        raise ValueError("CW2: eot_size %d needs bpda=True (expectation over transformation is part of the adaptive attack)"
                         % int(eot_size))


def snr_db(a0_i16, perturbation_i16):
    """10 log10(sum a0^2 / sum delta^2) of the int16 perturbation; +inf for an empty one."""
    s = float(np.sum(np.asarray(a0_i16, np.float64) ** 2))
    d = float(np.sum(np.asarray(perturbation_i16, np.float64) ** 2))
    if d == 0.0:
        return float("inf")
    return 10.0 * math.log10(s / d) if s > 0.0 else float("-inf")


def _takes_xvector(init):
    """CW2.__init__ with one more keyword, xvector=False.  The constructor's own parameter list is what callers and the host
    tests read with inspect.signature (functools.wraps keeps it so): the x-vector switch is a keyword-only extension to it."""
    @functools.wraps(init)
    def wrapper(self, *args, xvector=False, **kw):
        self.xvector = bool(xvector)
        return init(self, *args, **kw)
    return wrapper


class CW2(object):
    @_takes_xvector
    def __init__(self, task, attack_type, model, confidence=0., initial_const=1e-3, binary_search_steps=9, max_iter=10000, lr=1e-2,
                 stop_early=True, stop_early_iter=1000, bpda=False, eot_size=1, ivector=False, seed=None, verbose=True):
        if task not in ("OSI", "CSI", "SV"):
            raise ValueError("task must be OSI, CSI or SV")
        if not hasattr(model, "engine"):
            raise TypeError("CW2 differentiates this library's own systems: the model has no engine")
        if getattr(model, "task", task) != task:
            raise ValueError("model implements task %s, attack asked for %s" % (model.task, task))
        kind = getattr(model.engine, "kind", "gmm")
        xvector = getattr(self, "xvector", False)    # (_takes_xvector: the keyword-only xvector=True)
        if kind == "xv" and not xvector:
            raise ValueError("CW2: an x-vector system needs xvector=True (Engine.set_wb_xvector)")
        if kind not in ("gmm", "xv") and not ivector:
            raise ValueError("CW2: an i-vector system needs ivector=True (Engine.set_wb_ivector)")
        check_cw2_params(initial_const, binary_search_steps, max_iter, lr, stop_early_iter, eot_size, bpda)
        if kind not in ("gmm", "xv") and int(eot_size) > 1:
            raise ValueError("CW2: no expectation over transformation on an i-vector system (eot_size %d)" % int(eot_size))
        self.task = task
        self.attack_type = attack_type
        self.model = model
        self.adver_thresh = float(confidence)
        self.initial_const = float(initial_const)
        self.binary_search_steps = int(binary_search_steps)
        self.max_iter = int(max_iter)
        self.lr = float(lr)
        self.stop_early = bool(stop_early)
        self.stop_early_iter = int(stop_early_iter)
        self.bpda = bool(bpda)
        self.eot_size = int(eot_size)
        self.ivector = bool(ivector)
        self.threshold = 0.
        self.true = None
        self.target = None
        self.verbose = verbose
        self.epsilon = 0.002     # (not read by the attack: FakeBob's, for the threshold sweep)
        self.seed = int(np.random.randint(0, 2 ** 31 - 1)) if seed is None else int(seed)
        self._stream = 0
        if self.ivector:
            model.engine.set_wb_ivector(True)
        if self.xvector:
            model.engine.set_wb_xvector(True)
        if self.bpda:  # (left alone otherwise: the engine's own refusals then name what is set)
            model.engine.set_eot(self.eot_size)
            model.engine.set_wb_bpda(True)

    def estimate_threshold(self, audio, fs=16000, bits_per_sample=16, n_jobs=10, debug=False, **kw):
        """The sweep is FakeBob's (FAKEBOB.py:39-137), run by a FakeBob over the same model with its default NES
        hyper-parameters and this attack's seed and confidence, exactly as PGD.estimate_threshold does."""
        fb = FakeBob(self.task, self.attack_type, self.model, adver_thresh=self.adver_thresh, epsilon=self.epsilon,
                     seed=self.seed, verbose=self.verbose)
        fb._stream = self._stream
        eng = self.model.engine
        r = self.eot_size if self.bpda else 1
        if r > 1:
            eng.set_eot(1)
        try:
            res = fb.estimate_threshold(audio, fs=fs, bits_per_sample=bits_per_sample, n_jobs=n_jobs, debug=debug, **kw)
        finally:
            if r > 1:
                eng.set_eot(r)
        self._stream = fb._stream
        if res is not None:
            self.threshold = fb.threshold
        return res

    def _params(self, bits_per_sample=16):
        return nes_params(self.task, self.attack_type, adver_thresh=self.adver_thresh, max_iter=self.max_iter, samples_per_draw=0,
                          sigma=0.0, threshold=self.threshold, target=self.target, true=self.true,
                          seed=self.seed if self.bpda else 0, stream=self._stream if self.bpda else 0, bits_per_sample=bits_per_sample)

    def _cw2_params(self):
        return cw2_params(initial_const=self.initial_const, search_steps=self.binary_search_steps, lr=self.lr,
                          abort_every=self.stop_early_iter if self.stop_early else 0)

    # what a subclass with another distortion overrides (psy.Imperceptible): the trace columns of the checkpoint row's
    # distortion, of adver_loss and of the first score; the result's own fields; the distortion's parameters; the engine
    # call; the middle of the verbose line
    _COLS = (0, 1, 3)
    _FIELDS = ("best_l2",)

    def _distortion_params(self, audio):
        return None

    def _engine_attack(self, eng, p, q, d, audio):
        return eng.attack_cw2(p, q, audio)

    def _describe(self, out):
        return "l2:%g" % out.best_l2

    def attack(self, audio, checkpoint_path, threshold=0., true=None, target=None, fs=16000, bits_per_sample=16, n_jobs=10,
               debug=False):
        """FakeBob.attack's signature and pair: (int16 adversarial audio (N, 1), success_flag +-1) -- the successful iterate of
        the smallest distortion, or the cast of `audio` with flag -1 --, a companions.AttackResult that also carries the
        attack's own fields (_FIELDS), const (the constant after the last search step), snr_db (of the int16 perturbation) and
        rows_per_step.  CW2: the distortion is l2, the squared L2 distance in float audio units, and the field is best_l2.
        psy.Imperceptible: the distortion is dist = D + l2_weight * l2, and the fields are best_dist, best_l2 and n_over
        (bins of the returned iterate above the masking threshold).  The checkpoint pickled to checkpoint_path (protocol -1)
        is one [distortion, adver_loss, score, used_time] row per iteration, the search steps one after the other."""
        from . import companions as CP
        audio = _col(audio)
        bits = _check_bits(bits_per_sample)
        self.threshold = threshold
        self.true = true
        self.target = target
        eng = self.model.engine
        c_dist, c_loss, c_score = self._COLS
        d = self._distortion_params(audio[:, 0])          # (outside the timed call)
        t0 = time.time()
        res = self._engine_attack(eng, self._params(bits), self._cw2_params(), d, audio[:, 0])
        dt = time.time() - t0
        trace = res["trace"]
        n = trace.shape[0]
        used_time = eng.attack_iter_seconds(n)
        cp_global = []
        for r in range(n):
            sc = trace[r, c_score:]
            cp_global.append([trace[r, c_dist], np.array([trace[r, c_loss]]), sc[0] if self.task == "SV" else sc.copy(),
                              float(used_time[r])])
        if checkpoint_path:
            with open(checkpoint_path, "wb") as writer:
                pickle.dump(cp_global, writer, protocol=-1)
        adv = res["adv"]
        a0 = CP.cast_i16(audio[:, 0], bits)
        delta = adv.astype(np.int32) - a0.astype(np.int32)
        out = CP.AttackResult(adv[:, np.newaxis], res["success"], delta, bits, None)
        for k in self._FIELDS:
            setattr(out, k, res[k])
        out.const = res["const"]
        out.snr_db = snr_db(a0, delta)
        out.rows_per_step = res["rows_per_step"]
        if self.verbose:
            print("--- %d iters in %d search steps, success:%d, %s, snr:%.2f dB, c:%g, %.1f iters/s ---" %
                  (n, self.binary_search_steps, out[1], self._describe(out), out.snr_db, out.const, n / dt if dt > 0 else 0.0))
        return out
