"""Foreign victims of ParticleSwarm, Kenansville and HopSkipJump: what the three classes share when `model` is not one of
this package's systems (fb_attack_pso_foreign, fb_attack_kenansville_foreign, fb_attack_hsj_foreign; the "foreign victims"
section of include/fakebob_hip.h).

The search stays the engine's; only who scores a batch differs.  A model is asked in this order:
  1. `score_device(x)` callable: on the GPU.  x is a torch tensor [B, N] of the model's `device_dtype` (torch.float32 by
     default, or torch.float64), the result [B, S] scores ([B] for SV), kept as float64: FakeBob's rule.
  2. the two decision-only attacks: `make_decisions(audios, fs=, bits_per_sample=, n_jobs=, debug=)` on the (N, B) float64
     batch -> decisions or (decisions, scores); scalars for B = 1.  A decision of -2 means "no decision".
  3. `score(audios, ...)` -> scores; the engine decides by the make_decisions rule of the system classes.
ParticleSwarm reads scores, so it skips step 2.  Every row the model sees is an int16 row scaled by 2^-(bits_per_sample - 1):
the audio an attacker would submit as a wav file.

The three constructors take such a model only with `foreign=True`; without it they refuse a model that has no engine, as before.
A foreign victim's randomness is its own: eot_size > 1, quorum, companions and play_offset are refused by name.  Nothing
here runs on the hot path."""
import numpy as np

DEVICE_SCORES, HOST_DECISIONS, HOST_SCORES = "device_scores", "host_decisions", "host_scores"


def is_foreign(model):
    """a model without an engine of this package is the reference's plugin API"""
    return not hasattr(model, "engine")


def pick_mode(model, decisions):
    """How a foreign model is asked (the order of the module's docstring); decisions: the attack reads decisions."""
    if callable(getattr(model, "score_device", None)):
        return DEVICE_SCORES
    if decisions and callable(getattr(model, "make_decisions", None)):
        return HOST_DECISIONS
    if callable(getattr(model, "score", None)):
        return HOST_SCORES
    raise TypeError("model must provide score_device(x), %sscore(audios, fs=, bits_per_sample=, n_jobs=, debug=)"
                    % ("make_decisions(audios, ...) or " if decisions else ""))


def require_opt_in(who, foreign):
    """A model without an engine is attacked only when the caller says so (`foreign=True`): none of the engine's systems,
    defences and options stand in front of such a model, and a system object that lost its engine by mistake is not taken
    for a plugin.  Without the keyword the constructors refuse it, as they always did."""
    if not foreign:
        raise ValueError("%s attacks the engine's own systems (fakebob_amd.systems); pass foreign=True to attack a foreign "
                         "model through its score_device / make_decisions / score" % who)


def refuse_options(who, eot_size=None, quorum=None, companions=None, play_offset=None):
    """The options a foreign model cannot take, refused by name (no engine is touched)."""
    if eot_size is not None and int(eot_size) > 1:
        raise ValueError("%s: eot_size applies to the engine's own systems, not to a foreign model" % who)
    if quorum is not None:
        raise ValueError("%s: quorum applies to the engine's own systems, not to a foreign model" % who)
    if companions is not None:
        raise ValueError("%s: companions apply to the engine's own systems, not to a foreign model" % who)
    if play_offset:
        raise ValueError("%s: play_offset applies to the engine's own systems, not to a foreign model" % who)


class Victim(object):
    """One foreign model behind one of the three attacks: its mode, the bare engine the search runs on (created on first
    use, as FakeBob._engine does: torch first for a device model) and the descriptor handed to Engine.attack_*_foreign."""

    def __init__(self, who, task, model, decisions):
        self.who, self.task, self.model = who, task, model
        self.mode = pick_mode(model, decisions)
        self._engine = None
        self._n_spk = None
        self._bufs = None

    @property
    def device(self):
        return self.mode == DEVICE_SCORES

    def engine(self):
        if self._engine is None:
            if self.device:
                from . import _native
                _native.torch_first()   # torch before the library: one HIP runtime for both
            from .engine import Engine
            from .systems import default_device
            self._engine = Engine(default_device())
        return self._engine

    def _torch(self):
        from . import _native
        return _native.torch_first()

    def _x_dtype(self):
        torch = self._torch()
        dt = getattr(self.model, "device_dtype", torch.float32)
        if dt not in (torch.float32, torch.float64):
            raise ValueError("model.device_dtype %s: torch.float32 or torch.float64" % (dt,))
        return dt

    def speakers(self, probe_audio, **score_kw):
        """FakeBob._speakers' rule (attack.model_speakers)"""
        if self._n_spk is None:
            from .attack import model_speakers
            probe = None
            if self.device:
                def probe(a):
                    torch = self._torch()
                    x = torch.as_tensor(np.ascontiguousarray(a[:, 0]), device=torch.device("cuda", self.engine().device))
                    return int(self.model.score_device(x.to(self._x_dtype()).reshape(1, -1)).numel())
            elif self.mode == HOST_SCORES:
                def probe(a):
                    return int(np.asarray(self.model.score(a, **score_kw)).size)
            self._n_spk = model_speakers(self.model, self.task, probe_audio, probe)
        return self._n_spk

    def _decide_fn(self, S, score_kw):
        def fn(audios):   # (N, B) float64 -> (decisions (B,), scores (B, S) or None)
            out = self.model.make_decisions(audios, **score_kw)
            dec, sc = out if isinstance(out, tuple) and len(out) == 2 else (out, None)
            return dec, sc
        return fn

    def _score_fn(self, score_kw):
        def fn(audios):
            return self.model.score(audios, **score_kw)
        return fn

    def spec(self, rows_max, n, probe_audio, fs, bits_per_sample, n_jobs, debug):
        """The keywords of Engine.attack_*_foreign's `victim` for batches of up to rows_max rows of n samples."""
        kw = dict(fs=fs, bits_per_sample=bits_per_sample, n_jobs=n_jobs, debug=debug)
        S = self.speakers(probe_audio, **kw)
        if self.mode == HOST_DECISIONS:
            return dict(mode=self.mode, S=S, fn=self._decide_fn(S, kw))
        if self.mode == HOST_SCORES:
            return dict(mode=self.mode, S=S, fn=self._score_fn(kw))
        torch = self._torch()
        dev, dt = torch.device("cuda", self.engine().device), self._x_dtype()
        b = self._bufs
        if b is None or b[0].shape != (rows_max, n) or b[0].dtype != dt or b[1].shape != (rows_max, S):
            b = (torch.empty((rows_max, n), dtype=dt, device=dev), torch.empty((rows_max, S), dtype=torch.float64, device=dev))
            self._bufs = b
        return dict(mode=self.mode, S=S, fn=self.model.score_device, x=b[0], scores=b[1])

    def decide_one(self, row, threshold, fs, bits_per_sample, n_jobs, debug):
        """The decision on ONE audio (N,) float64 outside an attack (HopSkipJump's noise starts): make_decisions where the
        model has it, else the make_decisions rule of the system classes on its score / score_device."""
        kw = dict(fs=fs, bits_per_sample=bits_per_sample, n_jobs=n_jobs, debug=debug)
        if not self.device and callable(getattr(self.model, "make_decisions", None)):
            out = self.model.make_decisions(row[:, np.newaxis], **kw)
            dec = out[0] if isinstance(out, tuple) and len(out) == 2 else out
            return int(np.asarray(dec).reshape(-1)[0])
        if self.device:
            torch = self._torch()
            x = torch.as_tensor(np.ascontiguousarray(row), device=torch.device("cuda", self.engine().device))
            sc = self.model.score_device(x.to(self._x_dtype()).reshape(1, -1)).double().cpu().numpy()
        else:
            sc = self.model.score(row[:, np.newaxis], **kw)
        return decide_scores(self.task, np.asarray(sc, np.float64).reshape(1, -1), threshold)[0]


def decide_scores(task, scores, threshold):
    """The make_decisions rule of the system classes on scores (B, S) float64 -> a list of decisions: SV s >= threshold ?
    1 : -1; OSI / CSI the first maximum by strict > in ascending m (a NaN never displaces the running maximum); OSI a
    maximum < threshold -> -1."""
    out = []
    for s in np.asarray(scores, np.float64):
        am = 0
        for m in range(1, s.size):
            if s[m] > s[am]:
                am = m
        if task == "SV":
            out.append(1 if s[0] >= threshold else -1)
        else:
            out.append(-1 if (task == "OSI" and s[am] < threshold) else am)
    return out
