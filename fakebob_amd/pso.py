"""ParticleSwarm: SirenAttack's particle-swarm optimisation, the other score-based black-box attack of the evaluation this
package follows (SpeakerGuard runs it next to FAKEBOB), on the engine's own systems.

A swarm of `n_particles` candidate audios inside the epsilon ball is scored as one batch per iteration by the path that
scores every NES batch; one launch moves the swarm (fb_attack_pso; the arithmetic is written out in
include/fakebob_hip.h, "particle-swarm attack").  The surface is FakeBob's: the same `attack` arguments and return pair,
the same Philox stream handling (`seed`, one stream per attack() call), so a driver swaps one for the other.

Randomised victims and several utterances: `eot_size=` and `attack(..., companions=[...])` score every particle r' = K *
eot_size times and the swarm reads the mean loss, once `quorum=` switches that on (fakebob_amd.query_eot; "voted decisions"
in the header).  A foreign model -- any object with `score`, or `score_device` for a model on the same GPU -- is attacked by
the same swarm once the constructor is told `foreign=True` (fb_attack_pso_foreign; fakebob_amd.foreign): it scores the particles, the engine does the rest; eot_size,
quorum, companions and play_offset are refused for it by name.  Not in this version: swarm restarts.
"""
import math
import pickle
import time

import numpy as np

from .attack import FakeBob, _check_bits, _col
from .engine import nes_params, pso_params
from . import query_eot as QE
from . import foreign as FG

MAX_PARTICLES = 64


class ParticleSwarm(object):

    def __init__(self, task, attack_type, model, adver_thresh=0., epsilon=0.002, max_iter=300, n_particles=25,
                 w_init=0.9, w_end=0.1, c1=1.4961, c2=1.4961, v_max=None, seed=None, verbose=True, eot_size=None, quorum=None,
                 play_offset=None, foreign=False):
        """v_max=None: epsilon (a particle crosses the ball's radius in one step at most).  eot_size: every particle scored
        under that many draws of a randomised victim, the swarm reading the mean loss; it needs quorum= ("majority" or 1 ..
        32; None: off), the switch the three query attacks share -- PSO itself reads no votes."""
        if FG.is_foreign(model):    # (before the options' own rules: a foreign model takes none of them)
            FG.require_opt_in("ParticleSwarm", foreign)
            FG.refuse_options("ParticleSwarm", eot_size, quorum, None, play_offset)
        self.eot_size, self.quorum = QE.check_options("ParticleSwarm", eot_size, quorum)
        if task not in ("OSI", "CSI", "SV"):
            raise ValueError("task must be OSI, CSI or SV")
        if attack_type not in ("targeted", "untargeted"):
            raise ValueError("attack_type must be targeted or untargeted")
        self._victim = None
        if FG.is_foreign(model):    # the reference's plugin API: the model scores the swarm
            self._victim = FG.Victim("ParticleSwarm", task, model, decisions=False)
        elif play_offset:
            raise ValueError("ParticleSwarm does not run under a play offset: not in this version")
        if getattr(model, "task", task) != task:
            raise ValueError("model implements task %s, attack asked for %s" % (model.task, task))
        n_particles, max_iter = int(n_particles), int(max_iter)
        if not 2 <= n_particles <= MAX_PARTICLES:
            raise ValueError("n_particles=%d outside 2 .. %d" % (n_particles, MAX_PARTICLES))
        if max_iter < 1:
            raise ValueError("max_iter must be >= 1")
        epsilon = float(epsilon)
        if not (math.isfinite(epsilon) and epsilon > 0):
            raise ValueError("epsilon must be finite and > 0")
        v_max = epsilon if v_max is None else float(v_max)
        if not (math.isfinite(v_max) and v_max > 0):
            raise ValueError("v_max must be finite and > 0")
        for name, c in (("w_init", w_init), ("w_end", w_end), ("c1", c1), ("c2", c2)):
            if not (math.isfinite(float(c)) and float(c) >= 0):
                raise ValueError("%s must be finite and >= 0" % name)
        self.task = task
        self.attack_type = attack_type
        self.model = model
        self.adver_thresh = adver_thresh
        self.epsilon = epsilon
        self.max_iter = max_iter
        self.n_particles = n_particles
        self.w_init, self.w_end, self.c1, self.c2, self.v_max = float(w_init), float(w_end), float(c1), float(c2), v_max
        self.threshold = 0.
        self.true = None
        self.target = None
        self.seed = int(np.random.randint(0, 2 ** 31 - 1)) if seed is None else int(seed)
        self.verbose = verbose
        self._stream = 0  # Philox stream id: one per attack() call, as FakeBob counts them

    def estimate_threshold(self, audio, fs=16000, bits_per_sample=16, n_jobs=10, debug=False, **kw):
        """PSO has no threshold sweep of its own: the sweep is FakeBob's (FAKEBOB.py:39-137), run by a FakeBob over the same
        model with its default NES hyper-parameters and this attack's seed, epsilon and adver_thresh.  Returns what
        FakeBob.estimate_threshold returns and keeps the estimate in self.threshold."""
        fb = FakeBob(self.task, self.attack_type, self.model, adver_thresh=self.adver_thresh, epsilon=self.epsilon,
                     seed=self.seed, verbose=self.verbose)
        fb._stream = self._stream
        res = fb.estimate_threshold(audio, fs=fs, bits_per_sample=bits_per_sample, n_jobs=n_jobs, debug=debug, **kw)
        self._stream = fb._stream
        if res is not None:
            self.threshold = fb.threshold
        return res

    def attack(self, audio, checkpoint_path, threshold=0., true=None, target=None, fs=16000, bits_per_sample=16, n_jobs=10,
               debug=False, companions=None):
        """companions (needs quorum=): utterances as long as `audio` that ride along, as in FakeBob.attack -- one perturbation
        over all of them, the losses means over utterances and draws; the returned pair is a companions.AttackResult
        (perturbation_i16, apply_perturbation, per_utterance, votes = None).
        Returns (int16 adversarial audio (N, 1), success flag +-1), as FakeBob.attack does: the swarm's best position --
        a position that was scored -- and whether its loss fell below zero.  checkpoint_path (or None) receives a pickle
        (protocol -1) with one row per iteration, [array([gbest_loss]), gbest_score (a scalar for SV), used_time]: the
        layout is this attack's own (no distance column: the ball bounds it)."""
        audio = _col(audio)
        bits = _check_bits(bits_per_sample)
        self.threshold = threshold
        self.true = true
        self.target = target
        p = nes_params(self.task, self.attack_type, adver_thresh=self.adver_thresh, epsilon=self.epsilon,
                       max_iter=self.max_iter, threshold=threshold, target=target, true=true, seed=self.seed,
                       stream=self._stream, bits_per_sample=bits)
        q = pso_params(self.n_particles, self.w_init, self.w_end, self.c1, self.c2, self.v_max)
        self._stream += 1
        if self._victim is not None:
            FG.refuse_options("ParticleSwarm", companions=companions)
            return self._attack_foreign(p, q, audio, checkpoint_path, bits, fs, bits_per_sample, n_jobs, debug)
        eng = self.model.engine
        t0 = time.time()
        with QE.Settings("ParticleSwarm", eng, self.eot_size, self.quorum, companions, audio.shape[0], bits) as st:
            adv, flag, _advf, trace, _losses = eng.attack_pso(p, q, audio[:, 0])
        dt = time.time() - t0
        return self._finish(eng, adv, flag, trace, dt, audio, checkpoint_path, bits, st.comp, target, true, fs, bits_per_sample,
                            n_jobs, debug)

    def _attack_foreign(self, p, q, audio, checkpoint_path, bits, fs, bits_per_sample, n_jobs, debug):
        vic = self._victim
        eng = vic.engine()
        spec = vic.spec(self.n_particles, audio.shape[0], audio, fs, bits_per_sample, n_jobs, debug)
        t0 = time.time()
        adv, flag, _advf, trace, _losses = eng.attack_pso_foreign(p, q, spec, audio[:, 0])
        dt = time.time() - t0
        return self._finish(eng, adv, flag, trace, dt, audio, checkpoint_path, bits, None, self.target, self.true, fs,
                            bits_per_sample, n_jobs, debug)

    def _finish(self, eng, adv, flag, trace, dt, audio, checkpoint_path, bits, comp, target, true, fs, bits_per_sample, n_jobs,
                debug):
        n = trace.shape[0]
        used_time = eng.attack_iter_seconds(n)
        cp = []
        for r in range(n):
            sc = trace[r, 3:]
            cp.append([np.array([trace[r, 0]]), sc[0] if self.task == "SV" else sc.copy(), float(used_time[r])])
        if checkpoint_path:
            with open(checkpoint_path, "wb") as writer:
                pickle.dump(cp, writer, protocol=-1)
        if self.verbose:
            print("--- %d iters, %d particles, gbest loss:%f, %.1f iters/s ---" % (n, self.n_particles, trace[-1, 0], n / dt if dt > 0 else 0.0))
        return QE.result(self.model, self.task, self.attack_type, adv, flag, audio[:, 0], bits, comp, None, target=target,
                         true=true, fs=fs, bits_per_sample=bits_per_sample, n_jobs=n_jobs, debug=debug)
