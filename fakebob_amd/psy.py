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
import numpy as np

from .cw2 import CW2
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

    def _distortion_params(self, audio):
        theta, psd_max = masking_threshold(audio, float(self.model.engine.cfg.sample_freq), self.window)
        return psy_params(theta, psd_max, self.window, self.l2_weight)

    # CW2.attack (its docstring speaks for both) on this attack's trace layout {dist, l2, n_over, adver_loss, c, score0[S]}
    _COLS = (0, 3, 5)
    _FIELDS = ("best_dist", "best_l2", "n_over")

    def _engine_attack(self, eng, p, q, d, audio):
        return eng.attack_psy(p, q, d, audio)

    def _describe(self, out):
        return "dist:%g, l2:%g, over:%d" % (out.best_dist, out.best_l2, out.n_over)
