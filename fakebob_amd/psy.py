"""Imperceptible: the CW attack that hides under the voice (Qin et al., "Imperceptible, robust and targeted adversarial
examples for ASR") on the engine's own systems, behind FakeBob's interface.

CW2 measures its distortion as |x - a0|^2; a listener does not.  This attack is CW2's loop -- tanh space, Adam, the search over
the constant c, the smallest successful iterate kept on the device -- with the perceptual distortion in its place: the part of
the perturbation's short-time power spectrum that rises above the masking threshold of the speech it rides on, frame by frame
and bin by bin (fb_attack_psy; the contract is in include/fakebob_hip.h, "masking").  The threshold is computed here, once per
attack, by fakebob_amd.masking at the front end's sample rate.  l2_weight > 0 adds that much of CW2's |x - a0|^2 to the
distortion (0: masking alone).  Qin's two-stage alpha schedule is not reproduced: the search over c plays that role.

Victims and refusals are CW2's.
"""
import pickle
import time

import numpy as np

from .attack import _check_bits, _col
from .cw2 import CW2, snr_db
from .engine import psy_params
from .masking import WINDOWS, masking_threshold


class Imperceptible(CW2):
    def __init__(self, task, attack_type, model, window=2048, l2_weight=0., **kw):
        CW2.__init__(self, task, attack_type, model, **kw)
        if int(window) not in WINDOWS:
            raise ValueError("Imperceptible: window %r is not one of %s" % (window, WINDOWS))
        if not (np.isfinite(float(l2_weight)) and float(l2_weight) >= 0.0):
            raise ValueError("Imperceptible: l2_weight must be finite and >= 0 (got %r)" % (l2_weight,))
        self.window = int(window)
        self.l2_weight = float(l2_weight)

    def _psy_params(self, audio):
        theta, psd_max = masking_threshold(audio, float(self.model.engine.cfg.sample_freq), self.window)
        return psy_params(theta, psd_max, self.window, self.l2_weight)

    def attack(self, audio, checkpoint_path, threshold=0., true=None, target=None, fs=16000, bits_per_sample=16, n_jobs=10,
               debug=False):
        """FakeBob.attack's signature and pair: (int16 adversarial audio (N, 1), success_flag +-1) -- the successful iterate of
        the smallest distortion, or the cast of `audio` with flag -1 --, a companions.AttackResult that also carries best_dist
        (D + l2_weight * l2), best_l2, n_over (bins of the returned iterate above the threshold), const, snr_db and
        rows_per_step.  The checkpoint is CW2's layout, one [dist, adver_loss, score, used_time] row per iteration."""
        from . import companions as CP
        audio = _col(audio)
        bits = _check_bits(bits_per_sample)
        self.threshold = threshold
        self.true = true
        self.target = target
        eng = self.model.engine
        psy = self._psy_params(audio[:, 0])
        t0 = time.time()
        res = eng.attack_psy(self._params(bits), self._cw2_params(), psy, audio[:, 0])
        dt = time.time() - t0
        trace = res["trace"]
        n = trace.shape[0]
        used_time = eng.attack_iter_seconds(n)
        cp_global = []
        for r in range(n):
            sc = trace[r, 5:]
            cp_global.append([trace[r, 0], np.array([trace[r, 3]]), sc[0] if self.task == "SV" else sc.copy(), float(used_time[r])])
        if checkpoint_path:
            with open(checkpoint_path, "wb") as writer:
                pickle.dump(cp_global, writer, protocol=-1)
        adv = res["adv"]
        a0 = CP.cast_i16(audio[:, 0], bits)
        delta = adv.astype(np.int32) - a0.astype(np.int32)
        out = CP.AttackResult(adv[:, np.newaxis], res["success"], delta, bits, None)
        out.best_dist = res["best_dist"]
        out.best_l2 = res["best_l2"]
        out.n_over = res["n_over"]
        out.const = res["const"]
        out.snr_db = snr_db(a0, delta)
        out.rows_per_step = res["rows_per_step"]
        if self.verbose:
            print("--- %d iters in %d search steps, success:%d, dist:%g, l2:%g, over:%d, snr:%.2f dB, c:%g, %.1f iters/s ---" %
                  (n, self.binary_search_steps, out[1], out.best_dist, out.best_l2, out.n_over, out.snr_db, out.const,
                   n / dt if dt > 0 else 0.0))
        return out
