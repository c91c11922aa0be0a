"""HopSkipJump (Chen, Jordan, Wainwright 2020): the decision-only attack that reaches a decision, on the engine's own systems.

Kenansville (kenansville.py) makes an enrolled speaker unrecognised; it cannot build someone else's voice.  HopSkipJump
starts from `init`, any audio the system ALREADY decides as wanted -- the target speaker's own voice, an accepted voice --
and walks along the decision boundary towards the attacked utterance, reading decisions only: a boundary search on the
line between the two, then per iteration a batch of Gaussian probes around the boundary point whose decisions give a
direction, a batch of step sizes along it, and a boundary search again.  Every batch is scored by the path that scores an
NES batch (fb_attack_hsj; the arithmetic is written out in include/fakebob_hip.h, "decision-only attack II").  The surface
is FakeBob's: the same `attack` arguments and return pair, plus `init`.

Randomised victims and several utterances: with `quorum=` set, `eot_size=` and `attack(..., companions=[...])` score every row
r' = K * eot_size times and a row counts as adversarial from `quorum` adversarial replicas on -- its votes
(fakebob_amd.query_eot; "voted decisions" in the header).  A foreign model -- any object with `make_decisions`, `score`, or
`score_device` for a model on the same GPU -- is attacked by the same walk once the constructor is told `foreign=True` (fb_attack_hsj_foreign; fakebob_amd.foreign): it
decides every row, the engine does the rest; eot_size, quorum, companions and play_offset are refused for it by name.
"""
import math
import pickle
import time

import numpy as np

from .attack import _check_bits, _col
from .companions import cast_i16
from . import query_eot as QE
from . import foreign as FG
from .engine import hsj_params, nes_params

MAX_GRID, MAX_ROUNDS, MAX_EVALS = 64, 32, 1024
NOISE_STARTS = 16           # rows of uniform noise an untargeted attack without `init` tries as its start


def fit_init(init, n):
    """`init` as N samples: a longer one is cropped, a shorter one tiled"""
    v = np.asarray(init, np.float64).reshape(-1)
    if v.size == 0:
        raise ValueError("init is empty")
    if v.size < n:
        v = np.tile(v, -(-n // v.size))
    return np.ascontiguousarray(v[:n])


class HopSkipJump(object):

    def __init__(self, task, attack_type, model, grid=15, max_rounds=8, num_evals_init=32, num_evals_max=256, max_queries=0,
                 sigma_min=2.0 ** -15, probe_scale=0.05, max_iter=20, seed=None, verbose=True, eot_size=None, quorum=None,
                 play_offset=None, foreign=False):
        """eot_size: every scored row under that many draws of a randomised victim; quorum ("majority" or 1 .. 32; None:
        off) is the number of adversarial draws a row needs -- its votes -- to count as adversarial."""
        if FG.is_foreign(model):    # (before the options' own rules: a foreign model takes none of them)
            FG.require_opt_in("HopSkipJump", foreign)
            FG.refuse_options("HopSkipJump", eot_size, quorum, None, play_offset)
        self.eot_size, self.quorum = QE.check_options("HopSkipJump", eot_size, quorum)
        if task not in ("OSI", "CSI", "SV"):
            raise ValueError("task must be OSI, CSI or SV")
        if attack_type not in ("targeted", "untargeted"):
            raise ValueError("attack_type must be targeted or untargeted")
        self._victim = None
        if FG.is_foreign(model):    # the reference's plugin API: the model decides every row
            self._victim = FG.Victim("HopSkipJump", task, model, decisions=True)
        elif play_offset:
            raise ValueError("HopSkipJump does not run under a play offset: not in this version")
        if getattr(model, "task", task) != task:
            raise ValueError("model implements task %s, attack asked for %s" % (model.task, task))
        grid, max_rounds, max_iter, max_queries = int(grid), int(max_rounds), int(max_iter), int(max_queries)
        b0, b1 = int(num_evals_init), int(num_evals_max)
        if not 1 <= grid <= MAX_GRID:
            raise ValueError("grid=%d outside 1 .. %d" % (grid, MAX_GRID))
        if not 1 <= max_rounds <= MAX_ROUNDS:
            raise ValueError("max_rounds=%d outside 1 .. %d" % (max_rounds, MAX_ROUNDS))
        if not 1 <= b0 <= b1 <= MAX_EVALS:
            raise ValueError("num_evals %d : %d outside 1 <= init <= max <= %d" % (b0, b1, MAX_EVALS))
        if max_queries < 0:
            raise ValueError("max_queries=%d < 0" % max_queries)
        if max_iter < 0:
            raise ValueError("max_iter=%d < 0" % max_iter)
        sigma_min, probe_scale = float(sigma_min), float(probe_scale)
        if not (math.isfinite(sigma_min) and sigma_min > 0.0):
            raise ValueError("sigma_min must be finite and > 0")
        if not (math.isfinite(probe_scale) and probe_scale >= 0.0):
            raise ValueError("probe_scale must be finite and >= 0")
        self.task = task
        self.attack_type = attack_type
        self.model = model
        self.grid, self.max_rounds, self.num_evals_init, self.num_evals_max = grid, max_rounds, b0, b1
        self.max_queries, self.sigma_min, self.probe_scale, self.max_iter = max_queries, sigma_min, probe_scale, max_iter
        self.threshold = 0.
        self.true = None
        self.target = None
        self.seed = int(np.random.randint(0, 2 ** 31 - 1)) if seed is None else int(seed)
        self.verbose = verbose
        self._stream = 0  # Philox stream id: one per attack() call, as FakeBob counts them
        # of the last attack(): the L2 distance of the boundary point, the returned audio's SNR in dB and its largest
        # sample difference in int16 steps (None: no start), and the rows it scored
        self.dist = None
        self.snr_db = None
        self.linf_lsb = None
        self.n_queries = 0

    def estimate_threshold(self, audio, fs=16000, bits_per_sample=16, n_jobs=10, debug=False, **kw):
        """HopSkipJump has no threshold sweep of its own (a decision-only attacker cannot run one): the sweep is FakeBob's
        (FAKEBOB.py:39-137), run by a FakeBob over the same model with its default hyper-parameters and this attack's seed, as
        Kenansville.estimate_threshold does.  Keeps the estimate in self.threshold."""
        from .attack import FakeBob
        fb = FakeBob(self.task, self.attack_type, self.model, seed=self.seed, verbose=self.verbose)
        fb._stream = self._stream
        res = fb.estimate_threshold(audio, fs=fs, bits_per_sample=bits_per_sample, n_jobs=n_jobs, debug=debug, **kw)
        self._stream = fb._stream
        if res is not None:
            self.threshold = fb.threshold
        return res

    def _wanted(self, d, true, target):
        d = int(d)
        return d == target if self.attack_type == "targeted" else (d != true and d != -2)

    def _noise_start(self, n, true, target, threshold=0., **score_kw):
        """the first of up to NOISE_STARTS rows of uniform noise in [-1, 1) that the system decides as wanted, or None"""
        rs = np.random.RandomState(self.seed & 0xFFFFFFFF)
        for _ in range(NOISE_STARTS):
            row = rs.uniform(-1.0, 1.0, n)
            if self._victim is not None:   # a foreign model: its make_decisions, or the score rule on score / score_device
                d = self._victim.decide_one(row, threshold, **score_kw)
            else:
                d = self.model.make_decisions(row[:, np.newaxis])[0]    # (decisions, scores), as the system classes return
            if self._wanted(np.asarray(d).reshape(-1)[0], true, target):
                return row
        return None

    def attack(self, audio, checkpoint_path, threshold=0., true=None, target=None, fs=16000, bits_per_sample=16, n_jobs=10,
               debug=False, init=None, companions=None):
        """companions (needs quorum=): utterances as long as `audio` that ride along, as in FakeBob.attack -- every scored
        row's perturbation is scored on all of them, each (utterance, draw) one vote.  The returned pair is a
        companions.AttackResult: perturbation_i16, apply_perturbation, per_utterance and votes -- the logged votes of every
        scored row in scoring order (None when the rows were scored once).
        Returns (int16 adversarial audio (N, 1), success flag +-1), as FakeBob.attack does: a row that was scored and
        decided as wanted, as close to `audio` as the walk came -- or the int16 cast of the audio with -1 when `init` (or, for
        an untargeted attack without one, every noise start) is not decided as wanted.  init: the starting audio, cropped or
        tiled to N samples; a targeted attack needs one.  checkpoint_path (or None) receives a pickle (protocol -1) with one
        row per trace row (the start search, then the iterations): [D2, B, n+, m, hi, rounds, queries so far, sigma,
        used_time]."""
        audio = _col(audio)
        bits = _check_bits(bits_per_sample)
        if self.task == "SV" and true is None:
            true = 1
        if self.task == "SV" and self.attack_type == "targeted" and target is None:
            target = 1                    # (the driver's SV attack: a rejected voice is to be accepted)
        if self.task == "OSI" and self.attack_type == "untargeted" and true is None:
            true = -1                     # (the driver's OSI voices are those the system rejects)
        if self.attack_type == "targeted" and target is None:
            raise ValueError("a targeted attack needs a target")
        if self.attack_type == "untargeted" and true is None:
            raise ValueError("an untargeted attack needs the true decision")
        if self.attack_type == "targeted" and init is None:
            raise ValueError("a targeted HopSkipJump needs init: an audio the system already decides as the target")
        self.threshold = threshold
        self.true = true
        self.target = target
        n = audio.shape[0]
        self.dist = self.snr_db = self.linf_lsb = None
        self.n_queries = 0
        x0 = cast_i16(audio[:, 0], bits)
        if self._victim is not None:
            FG.refuse_options("HopSkipJump", companions=companions)
            start = fit_init(init, n) if init is not None else self._noise_start(
                n, true, target, threshold, fs=fs, bits_per_sample=bits_per_sample, n_jobs=n_jobs, debug=debug)
        else:
            start = fit_init(init, n) if init is not None else self._noise_start(n, true, target)
        if start is None:
            if self.verbose:
                print("--- no noise start is decided as wanted ---")
            return QE.result(self.model, self.task, self.attack_type, x0, -1, audio[:, 0], bits, None, None)
        p = nes_params(self.task, self.attack_type, max_iter=self.max_iter, threshold=threshold, target=target, true=true,
                       seed=self.seed, stream=self._stream, bits_per_sample=bits)
        k = hsj_params(self.grid, self.max_rounds, self.num_evals_init, self.num_evals_max, self.max_queries, self.sigma_min,
                       self.probe_scale)
        self._stream += 1
        if self._victim is not None:
            eng = self._victim.engine()
            spec = self._victim.spec(max(self.grid, self.num_evals_max), n, audio, fs, bits_per_sample, n_jobs, debug)
            t0 = time.time()
            res = eng.attack_hsj_foreign(p, k, spec, audio[:, 0], start)
            st, rp = QE.Settings("HopSkipJump", eng, None, None, None, n, bits), 1
        else:
            eng = self.model.engine
            t0 = time.time()
            with QE.Settings("HopSkipJump", eng, self.eot_size, self.quorum, companions, n, bits) as st:
                res = eng.attack_hsj(p, k, audio[:, 0], start)
            rp = st.replicas if st.quorum is not None else 1
        dt = time.time() - t0
        rows = res["trace"].shape[0]
        used_time = eng.attack_iter_seconds(rows)
        cp = [res["trace"][r].tolist() + [float(used_time[r])] for r in range(rows)]
        if checkpoint_path:
            with open(checkpoint_path, "wb") as writer:
                pickle.dump(cp, writer, protocol=-1)
        self.n_queries = res["n_queries"]
        if res["success"] == 1:
            scale = float(2 ** (bits - 1))
            diff = res["adv"].astype(np.float64) - x0.astype(np.float64)
            noise_p, sig_p = float(np.sum((diff / scale) ** 2)), float(np.sum((x0.astype(np.float64) / scale) ** 2))
            self.dist = math.sqrt(res["dist2"])
            self.snr_db = float("inf") if noise_p == 0.0 else (10.0 * math.log10(sig_p / noise_p) if sig_p > 0.0 else float("-inf"))
            self.linf_lsb = int(np.abs(diff).max())
        if self.verbose:
            print("--- %d iterations, %d queries, success %d, |x - a| %s, SNR %s dB, %.3f s ---" % (
                res["n_iters"], self.n_queries, res["success"], self.dist, self.snr_db, dt))
        return QE.result(self.model, self.task, self.attack_type, res["adv"], res["success"], audio[:, 0], bits, st.comp,
                         res["decisions"] if rp > 1 else None, target=target, true=true, fs=fs, bits_per_sample=bits_per_sample,
                         n_jobs=n_jobs, debug=debug)
