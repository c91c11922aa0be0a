"""PGD: the white-box gradient attacks of SpeakerGuard's evaluation (FGSM, PGD, the margin-loss CW-inf) on the engine's own
GMM-UBM systems, behind FakeBob's interface.

The loop is FakeBob.attack's (FAKEBOB.py:139-221) with the analytic gradient of the loss in place of the NES estimate
(fb_attack_wb): momentum sign steps inside the epsilon ball, the plateau learning-rate rule on the clean loss, the early
stop on adver_loss < 0.  momentum = 0 is plain PGD with the margin loss; max_iter = 1 is the single-step attack.  There
is no random start, so a run is reproducible.  PGD's victim has to be undefended.  AdaptivePGD is the adaptive attack on a
defended one (Engine.set_wb_bpda): BPDA through the model's input-transform chain and codec, and with eot_size = r > 1 an
expectation over r draws of its random stages per iteration, keyed by the attack's seed and stream.  The air channel is
refused unless air=True (Engine.set_wb_air: the gradient through the drawn rooms, with eot_size = r the EOT-over-rooms
gradient of the robust over-the-air attack); feature compression and dither are refused unless frontend=True
(Engine.set_wb_frontend: the forward's final k-means assignment and its dither draws held constant); companions are refused
unless universal=True (Engine.set_wb_universal: attack(..., companions=[...]) then takes the gradient of the loss averaged over
the utterances -- the white-box twin of FakeBob.attack(..., companions=)); refused as well are i-vector
systems and foreign models -- the gradient is that of this library's own forward.  IvectorPGD is the same attack on an i-vector-PLDA system (Engine.set_wb_ivector): the
gradient through the PLDA back end, both length normalisations, the posterior solve and the full-covariance posteriors, with
the frames' component selection and pruned sets held constant; PGD and AdaptivePGD keep refusing such a system.  XvectorPGD
is the same attack on an x-vector (TDNN) system (Engine.set_wb_xvector): the gradient through the PLDA back end, the segment
affine, statistics pooling and every frame layer, with the forward's ReLU and variance-floor decisions held constant.
"""
import pickle
import time

import numpy as np

from .attack import FakeBob, _check_bits, _col
from .engine import nes_params


class PGD(object):
    KINDS = ("gmm",)   # engine kinds the class differentiates (IvectorPGD: the i-vector back end as well)

    def __init__(self, task, attack_type, model, adver_thresh=0., epsilon=0.002, max_iter=1000, max_lr=0.001, min_lr=1e-6,
                 momentum=0.9, plateau_length=5, plateau_drop=2., seed=None, verbose=True, play_offset=None):
        if task not in ("OSI", "CSI", "SV"):
            raise ValueError("task must be OSI, CSI or SV")
        if not hasattr(model, "engine"):
            raise TypeError("PGD differentiates this library's own GMM-UBM systems: the model has no engine")
        if getattr(model, "task", task) != task:
            raise ValueError("model implements task %s, attack asked for %s" % (model.task, task))
        if getattr(model.engine, "kind", "gmm") not in self.KINDS:
            if getattr(model.engine, "kind", "gmm") == "xv":
                raise ValueError("%s: an x-vector system needs XvectorPGD (Engine.set_wb_xvector)" % type(self).__name__)
            raise ValueError("PGD: i-vector systems are out of this version (GMM-UBM systems only)")
        self.bpda = False   # (AdaptivePGD: True -- the engine's switch is on and seed / stream key the victim's draws)
        self.air = False    # (air=True of AdaptivePGD / IvectorPGD: Engine.set_wb_air is on; seed / stream key the rooms)
        self.frontend = False   # (frontend=True of the two: Engine.set_wb_frontend is on; seed / stream key the k-means and dither draws)
        self.universal = False  # (universal=True of AdaptivePGD: Engine.set_wb_universal is on; attack() takes companions)
        self.play_offset = 0    # (play_offset=S of the two with universal=True: Engine.set_play_offset for the length of attack())
        from .play_offset import check_offset
        if check_offset(play_offset):   # (FakeBob's keyword; the subclasses take it themselves and do not hand it on)
            raise ValueError("PGD: play_offset %d needs universal=True (AdaptivePGD / IvectorPGD: Engine.set_wb_universal)" % int(play_offset))
        self.eot_size = 1
        self.task = task
        self.attack_type = attack_type
        self.model = model
        self.adver_thresh = adver_thresh
        self.epsilon = epsilon
        self.max_iter = max_iter
        self.max_lr = max_lr
        self.min_lr = min_lr
        self.momentum = momentum
        self.plateau_length = plateau_length
        self.plateau_drop = plateau_drop
        self.threshold = 0.
        self.true = None
        self.target = None
        self.verbose = verbose
        # an undefended attack draws nothing; the seed keys the threshold sweep, which is FakeBob's (estimate_threshold), and
        # in AdaptivePGD the draws of the victim's random stages
        self.seed = int(np.random.randint(0, 2 ** 31 - 1)) if seed is None else int(seed)
        self._stream = 0

    def estimate_threshold(self, audio, fs=16000, bits_per_sample=16, n_jobs=10, debug=False, **kw):
        """The white-box attack has no threshold sweep of its own: the sweep is FakeBob's (FAKEBOB.py:39-137), run by a
        FakeBob over the same model with its default NES hyper-parameters and this attack's seed, epsilon and adver_thresh.
        Returns what FakeBob.estimate_threshold returns and keeps the estimate in self.threshold."""
        fb = FakeBob(self.task, self.attack_type, self.model, adver_thresh=self.adver_thresh, epsilon=self.epsilon,
                     seed=self.seed, verbose=self.verbose)
        fb._stream = self._stream
        # (the sweep does not run under EOT: with bpda and eot_size > 1 it scores single draws, and the size is put back)
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
        return nes_params(self.task, self.attack_type, adver_thresh=self.adver_thresh, epsilon=self.epsilon,
                          max_iter=self.max_iter, max_lr=self.max_lr, min_lr=self.min_lr, samples_per_draw=0, sigma=0.0,
                          momentum=self.momentum, plateau_length=self.plateau_length, plateau_drop=self.plateau_drop,
                          threshold=self.threshold, target=self.target, true=self.true, seed=self.seed if (self.bpda or self.air or self.frontend or self.play_offset) else 0,
                          stream=self._stream if (self.bpda or self.air or self.frontend or self.play_offset) else 0, bits_per_sample=bits_per_sample)

    def get_grad(self, audio, fs=16000, bits_per_sample=16, n_jobs=10, debug=False):
        """-> (grad (N,1) = d loss / d audio, adver_loss (1,), score), the analytic twin of FakeBob.get_grad's last three."""
        audio = _col(audio)
        grad, al, sc = self.model.engine.get_grad_wb(self._params(_check_bits(bits_per_sample)), audio[:, 0])
        S = self.model.engine.n_speakers
        return grad[:, np.newaxis], np.array([al]), (sc[0] if self.task == "SV" else sc[:S].copy())

    def attack(self, audio, checkpoint_path, threshold=0., true=None, target=None, fs=16000, bits_per_sample=16, n_jobs=10,
               debug=False):
        """FakeBob.attack's signature and results: (int16 adversarial audio (N,1), success_flag +-1), and the trace
        [distance, adver_loss, score, used_time] per iteration pickled to checkpoint_path (protocol -1).  The pair is a
        companions.AttackResult, as FakeBob.attack's is: it also carries perturbation_i16 and apply_perturbation(wavs).  PGD
        The signature is FakeBob.attack's without its extensions: companions go through attack_universal."""
        return self._attack(audio, checkpoint_path, threshold, true, target, fs, bits_per_sample, n_jobs, debug, None)

    def attack_universal(self, audio, checkpoint_path, companions, threshold=0., true=None, target=None, fs=16000, bits_per_sample=16,
                         n_jobs=10, debug=False):
        """attack() with FakeBob.attack's companions, for the classes that take universal=True (AdaptivePGD, whose attack() also
        has the keyword, and IvectorPGD); ValueError without it."""
        return self._attack(audio, checkpoint_path, threshold, true, target, fs, bits_per_sample, n_jobs, debug, companions)

    def _attack(self, audio, checkpoint_path, threshold, true, target, fs, bits_per_sample, n_jobs, debug, companions):
        """attack() with FakeBob.attack's companions (universal=True only; ValueError otherwise): utterances as long as `audio`
        that ride along for this call, ONE perturbation over all of them, the loop's losses their means; the result then also
        carries per_utterance -- every composed utterance re-scored through model.make_decisions, with its success."""
        audio = _col(audio)
        bits = _check_bits(bits_per_sample)
        from . import companions as CP
        comp = None
        if companions is not None:
            if not self.universal:
                raise ValueError("PGD: companions need universal=True (AdaptivePGD / IvectorPGD: Engine.set_wb_universal)")
            comp = CP.as_companions(companions, audio.shape[0], bits)
        self.threshold = threshold
        self.true = true
        self.target = target
        eng = self.model.engine
        if self.play_offset >= audio.shape[0] > 0:
            raise ValueError("play_offset %d: the audio has %d samples, the offset must stay below that" % (self.play_offset, audio.shape[0]))
        t0 = time.time()
        # (an engine is asked for a setting only when this call changes it)
        before = eng.companions if companions is not None else None
        before_S = eng.play_offset if self.play_offset else 0
        try:
            if companions is not None:
                eng.set_companions(comp)
            if self.play_offset:
                eng.set_play_offset(self.play_offset)
            adv, flag, _advf, trace = eng.attack_wb(self._params(bits), audio[:, 0])
        finally:
            if self.play_offset:
                eng.set_play_offset(before_S)
            if companions is not None:
                eng.set_companions(before)
        dt = time.time() - t0
        n = trace.shape[0]
        used_time = eng.attack_iter_seconds(n)
        cp_global = []
        for r in range(n):
            used = 0. if (r == n - 1 and trace[r, 1] < 0) else float(used_time[r])  # the early-stop row stores 0. (:187)
            sc = trace[r, 3:]
            cp_global.append([trace[r, 0], np.array([trace[r, 1]]), sc[0] if self.task == "SV" else sc.copy(), used])
        if checkpoint_path:
            with open(checkpoint_path, "wb") as writer:
                pickle.dump(cp_global, writer, protocol=-1)
        if self.verbose:
            print("--- %d iters, distance:%f, loss:%f, %.1f iters/s ---" %
                  (n, trace[-1, 0], trace[-1, 1], n / dt if dt > 0 else 0.0))
        a0 = CP.cast_i16(audio[:, 0], bits)
        delta = adv.astype(np.int32) - a0.astype(np.int32)
        per = None
        kw = dict(fs=fs, bits_per_sample=bits_per_sample, n_jobs=n_jobs, debug=debug)
        if comp is not None:
            per = []
            for u, w in enumerate([adv] + CP.apply_perturbation(delta, list(comp))):
                dec, sc = self.model.make_decisions(w, **kw)
                per.append(dict(utterance=u, audio_i16=w, decision=dec, score=sc,
                                success=CP.succeeded(self.task, self.attack_type, dec, target=target, true=true)))
        per_off = None
        if self.play_offset:   # every utterance under the perturbation at each offset of the grid, as in FakeBob.attack
            from .play_offset import per_offset
            per_off = per_offset(self.model, self.task, self.attack_type, [a0] + ([] if comp is None else list(comp)), delta,
                                 self.play_offset, target=target, true=true, **kw)
        return CP.AttackResult(adv[:, np.newaxis], flag, delta, bits, per, per_off)

    def _set_play_offset(self, play_offset):
        """play_offset=S of AdaptivePGD / IvectorPGD: kept here, set on the engine for the length of an attack (fb_set_play_offset
        rides on the universal path: ValueError without universal=True)"""
        from .play_offset import check_offset
        S = check_offset(play_offset)
        if S and not self.universal:
            raise ValueError("%s: play_offset %d needs universal=True (Engine.set_wb_universal)" % (type(self).__name__, S))
        self.play_offset = S


class AdaptivePGD(PGD):
    """PGD on a DEFENDED victim: the adaptive white-box attack of SpeakerGuard's evaluation matrix.  bpda=True switches the
    engine to differentiate through the model's input-transform chain and codec (Engine.set_wb_bpda; the derivative rules are
    in include/fakebob_hip.h), eot_size = r takes the mean loss and gradient over r draws of the random stages per iteration
    (Engine.set_eot).  Everything else -- knobs, attack(), get_grad(), return pair, checkpoint layout -- is PGD's.  The
    constructor sets both on the model's engine and they stay set; bpda=False with eot_size=1 is PGD itself.  air=True also
    switches the engine to differentiate through the model's over-the-air channel (Engine.set_wb_air): each iteration then
    takes the gradient through the eot_size rooms its forward drew.  frontend=True switches it to differentiate through the
    model's feature compression and dither (Engine.set_wb_frontend): the gradient at the k-means assignment and the dither
    draws of each of the eot_size forwards.  universal=True switches it to take companions (Engine.set_wb_universal):
    attack(..., companions=[...]) then descends the loss averaged over the utterances (times the eot_size draws of each); it needs
    no other switch on an undefended victim (bpda=False).  play_offset=S (with universal=True; Engine.set_play_offset for the length of
    an attack) rotates the perturbation by an offset of its own in 0 .. S on every replica: the attack descends the loss
    averaged over playback timings, and the result carries per_offset."""

    def __init__(self, task, attack_type, model, bpda=True, eot_size=1, air=False, frontend=False, universal=False, play_offset=None,
                 **kw):
        eot_size = int(eot_size)
        if not 1 <= eot_size <= 32:
            raise ValueError("AdaptivePGD: eot_size %d outside 1 .. 32" % eot_size)
        if eot_size > 1 and not bpda:
            raise ValueError("AdaptivePGD: eot_size %d needs bpda=True (expectation over transformation is part of the "
                             "adaptive attack)" % eot_size)
        PGD.__init__(self, task, attack_type, model, **kw)
        self.bpda = bool(bpda)
        self.eot_size = eot_size
        if self.bpda:  # (left alone otherwise: the engine's own refusals then name what is set)
            model.engine.set_eot(eot_size)
            model.engine.set_wb_bpda(True)
        self.air = bool(air)
        if self.air:
            model.engine.set_wb_air(True)
        self.frontend = bool(frontend)
        if self.frontend:
            model.engine.set_wb_frontend(True)
        self.universal = bool(universal)
        if self.universal:
            model.engine.set_wb_universal(True)
        self._set_play_offset(play_offset)

    def attack(self, audio, checkpoint_path, threshold=0., true=None, target=None, fs=16000, bits_per_sample=16, n_jobs=10,
               debug=False, companions=None):
        """PGD.attack with FakeBob.attack's companions (universal=True; ValueError otherwise): the same setting and clearing of
        the engine's companions for this call, the same AttackResult with per_utterance."""
        return self._attack(audio, checkpoint_path, threshold, true, target, fs, bits_per_sample, n_jobs, debug, companions)


class IvectorPGD(PGD):
    """PGD on an i-vector-PLDA victim (and, unchanged, on a GMM-UBM one).  The constructor switches the model's engine to
    differentiate through the i-vector back end (Engine.set_wb_ivector; the rules are in include/fakebob_hip.h) and, with
    bpda=True, through an input-transform chain and a codec as well (Engine.set_wb_bpda); both stay set.  air=True: through the
    model's over-the-air channel too (Engine.set_wb_air); frontend=True: through feature compression and dither
    (Engine.set_wb_frontend).  universal=True (Engine.set_wb_universal): attack_universal(audio, cp, companions) descends the loss
    averaged over the utterances, and -- the forward then keeps every replica's i-vector state -- eot_size = r > 1 takes the expectation
    over r draws of the random stages per iteration (with bpda=True, as in AdaptivePGD).  Without it there is no expectation
    over transformation for an i-vector system.  Knobs, attack(), get_grad(), estimate_threshold(), the return pair and the
    checkpoint layout are PGD's."""
    KINDS = ("gmm", "iv")

    def __init__(self, task, attack_type, model, bpda=False, air=False, frontend=False, universal=False, eot_size=1, play_offset=None,
                 **kw):
        eot_size = int(eot_size)
        if not 1 <= eot_size <= 32:
            raise ValueError("IvectorPGD: eot_size %d outside 1 .. 32" % eot_size)
        if eot_size > 1 and not (universal and bpda):
            raise ValueError("IvectorPGD: eot_size %d needs universal=True (per-replica i-vector state) and bpda=True" % eot_size)
        PGD.__init__(self, task, attack_type, model, **kw)
        self.bpda = bool(bpda)
        model.engine.set_wb_ivector(True)
        if self.bpda:
            model.engine.set_wb_bpda(True)
        self.air = bool(air)
        if self.air:
            model.engine.set_wb_air(True)
        self.frontend = bool(frontend)
        if self.frontend:
            model.engine.set_wb_frontend(True)
        self.universal = bool(universal)
        if self.universal:
            model.engine.set_wb_universal(True)
            self.eot_size = eot_size
            if self.bpda:
                model.engine.set_eot(eot_size)
        self._set_play_offset(play_offset)


class XvectorPGD(PGD):
    """PGD on an x-vector (TDNN) victim (and, unchanged, on a GMM-UBM one).  The constructor switches the model's engine to
    differentiate through the TDNN (Engine.set_wb_xvector; the rules are in include/fakebob_hip.h) and, with bpda=True, through
    an input-transform chain and a codec as well (Engine.set_wb_bpda), eot_size = r then taking the mean loss and gradient over
    r draws of the random stages per iteration (Engine.set_eot); all stay set.  An air channel, dither, companions and a play
    offset are refused by the engine on this victim.  Knobs, attack(), get_grad(), estimate_threshold(), the return pair and the
    checkpoint layout are PGD's."""
    KINDS = ("gmm", "xv")

    def __init__(self, task, attack_type, model, bpda=False, eot_size=1, **kw):
        eot_size = int(eot_size)
        if not 1 <= eot_size <= 32:
            raise ValueError("XvectorPGD: eot_size %d outside 1 .. 32" % eot_size)
        if eot_size > 1 and not bpda:
            raise ValueError("XvectorPGD: eot_size %d needs bpda=True (expectation over transformation is part of the "
                             "adaptive attack)" % eot_size)
        PGD.__init__(self, task, attack_type, model, **kw)
        self.bpda = bool(bpda)
        model.engine.set_wb_xvector(True)
        if self.bpda:
            self.eot_size = eot_size
            model.engine.set_eot(eot_size)
            model.engine.set_wb_bpda(True)
