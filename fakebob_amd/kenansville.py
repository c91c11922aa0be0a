"""Kenansville: the decision-only black-box attack of the evaluation this package follows (SpeakerGuard runs it next to
FAKEBOB and SirenAttack), on the engine's own systems.  It is the decision-only EVASION attack: the weakest spectral content
of short windows is removed until the system no longer gives the decision it gave, and the smallest removal that does so
is looked for.  It accepts a targeted call, but removing spectral content does not build someone else's voice: the
decision-only attack that reaches a chosen decision is HopSkipJump (hsj.py, `attack_main --attack hsj`).

Every candidate is a function of the audio and one integer factor q in 0 .. 65536; one launch analyses the utterance, one
launch per round writes a round's candidates into the batch the front end scores, and the host reads the decisions once
per round (fb_attack_kenansville; the arithmetic is written out in include/fakebob_hip.h, "decision-only attack").
`tables` builds the four integer tables the engine takes, `remove` is the contract's host twin in vectorised numpy, as
codec.py is for the codecs.  The surface is FakeBob's: the same `attack` arguments and return pair.

Randomised victims and several utterances: with `quorum=` set, `eot_size=` and `attack(..., companions=[...])` score every row
r' = K * eot_size times and a row counts as adversarial from `quorum` adversarial replicas on -- its votes
(fakebob_amd.query_eot; "voted decisions" in the header).  A foreign model -- any object with `make_decisions`, `score`, or
`score_device` for a model on the same GPU -- is attacked by the same search once the constructor is told `foreign=True` (fb_attack_kenansville_foreign;
fakebob_amd.foreign): it decides the candidates, the engine does the rest; eot_size, quorum, companions and play_offset are
refused for it by name.
"""
import math
import pickle
import time

import numpy as np

from .attack import _check_bits, _col
from .engine import kv_params, nes_params
from . import query_eot as QE
from . import foreign as FG

MIN_WINDOW, MAX_WINDOW = 8, 128
MAX_GRID, MAX_ROUNDS, Q_ONE = 64, 32, 65536


def _check_window(W):
    W = int(W)
    if not MIN_WINDOW <= W <= MAX_WINDOW:
        raise ValueError("window=%d outside %d .. %d" % (W, MIN_WINDOW, MAX_WINDOW))
    return W


def tables(W):
    """The tables of the contract, (4, W) int32: CF, SF = rint(cos, sin(2 pi j / W) 2^30), CI, SI = rint(.. 2^22)."""
    W = _check_window(W)
    ang = 2.0 * np.pi * np.arange(W, dtype=np.float64) / W
    c, s = np.cos(ang), np.sin(ang)
    return np.ascontiguousarray(np.stack([np.rint(c * 2.0 ** 30), np.rint(s * 2.0 ** 30), np.rint(c * 2.0 ** 22),
                                          np.rint(s * 2.0 ** 22)]).astype(np.int32))


def bin_weights(W):
    """m[k]: 1 for k = 0 and, W even, for k = W / 2; otherwise 2"""
    m = np.full(W // 2 + 1, 2, np.int64)
    m[0] = 1
    if W % 2 == 0:
        m[W // 2] = 1
    return m


def analyse(x_i16, W, tab=None):
    """The analysis of the contract -> (X (nw, W) int64, the zero-padded windows; a, b, cum (nw, K) int64; E (nw,) int64)."""
    W = _check_window(W)
    tab = tables(W) if tab is None else np.asarray(tab)
    x = np.asarray(x_i16, np.int16).reshape(-1).astype(np.int64)
    K, nw = W // 2 + 1, -(-x.size // W)
    X = np.zeros(nw * W, np.int64)
    X[:x.size] = x
    X = X.reshape(nw, W)
    idx = (np.arange(W)[:, None] * np.arange(K)[None, :]) % W          # (n k) mod W
    A = X @ tab[0].astype(np.int64)[idx]
    B = X @ tab[1].astype(np.int64)[idx]
    a, b = (A + (1 << 29)) >> 30, (B + (1 << 29)) >> 30
    p = a * a + b * b
    e = bin_weights(W)[None, :] * p
    order = np.argsort(p, axis=1, kind="stable")                        # ascending by (p, k)
    cs = np.cumsum(np.take_along_axis(e, order, 1), axis=1)
    cum = np.empty_like(cs)
    np.put_along_axis(cum, order, cs, 1)
    return X, a, b, cum, e.sum(axis=1)


def remove(x_i16, W, q, tab=None):
    """Candidate q (0 .. 65536) of the int16 samples x: the host twin of k_kv_analyse + k_kv_candidates, bit for bit."""
    W, q = _check_window(W), int(q)
    if not 0 <= q <= Q_ONE:
        raise ValueError("q=%d outside 0 .. %d" % (q, Q_ONE))
    tab = tables(W) if tab is None else np.asarray(tab)
    n = np.asarray(x_i16).size
    X, a, b, cum, E = analyse(x_i16, W, tab)
    K = W // 2 + 1
    thr = (E >> 16) * q + (((E & 0xFFFF) * q) >> 16)
    keep = (cum <= thr[:, None]).astype(np.int64) * bin_weights(W)[None, :]
    idx = (np.arange(K)[:, None] * np.arange(W)[None, :]) % W          # (k n) mod W
    R = (keep * a) @ tab[2].astype(np.int64)[idx] + (keep * b) @ tab[3].astype(np.int64)[idx]
    D = W << 22
    r = (2 * R + D) // (2 * D)                                          # numpy's // floors
    return np.clip(X - r, -32768, 32767).reshape(-1)[:n].astype(np.int16)


def q_of(max_factor):
    """max_factor in (0, 1] -> q_max = floor(max_factor 65536), at least 1"""
    f = float(max_factor)
    if not (math.isfinite(f) and 0.0 < f <= 1.0):
        raise ValueError("max_factor must be in (0, 1]")
    return max(int(math.floor(f * Q_ONE)), 1)


class Kenansville(object):

    def __init__(self, task, attack_type, model, window=100, grid=15, max_factor=1.0, max_rounds=32, seed=None, verbose=True,
                 eot_size=None, quorum=None, play_offset=None, foreign=False):
        """eot_size: every candidate scored under that many draws of a randomised victim; quorum ("majority" or 1 .. 32;
        None: off) is the number of adversarial draws a candidate needs -- its votes -- to count as succeeding."""
        if FG.is_foreign(model):    # (before the options' own rules: a foreign model takes none of them)
            FG.require_opt_in("Kenansville", foreign)
            FG.refuse_options("Kenansville", eot_size, quorum, None, play_offset)
        self.eot_size, self.quorum = QE.check_options("Kenansville", eot_size, quorum)
        if task not in ("OSI", "CSI", "SV"):
            raise ValueError("task must be OSI, CSI or SV")
        if attack_type not in ("targeted", "untargeted"):
            raise ValueError("attack_type must be targeted or untargeted")
        self._victim = None
        if FG.is_foreign(model):    # the reference's plugin API: the model decides the candidates
            self._victim = FG.Victim("Kenansville", task, model, decisions=True)
        elif play_offset:
            raise ValueError("Kenansville does not run under a play offset: not in this version")
        if getattr(model, "task", task) != task:
            raise ValueError("model implements task %s, attack asked for %s" % (model.task, task))
        self.window = _check_window(window)
        grid, max_rounds = int(grid), int(max_rounds)
        if not 1 <= grid <= MAX_GRID:
            raise ValueError("grid=%d outside 1 .. %d" % (grid, MAX_GRID))
        if not 1 <= max_rounds <= MAX_ROUNDS:
            raise ValueError("max_rounds=%d outside 1 .. %d" % (max_rounds, MAX_ROUNDS))
        self.q_max = q_of(max_factor)
        self.task = task
        self.attack_type = attack_type
        self.model = model
        self.grid, self.max_rounds, self.max_factor = grid, max_rounds, float(max_factor)
        self.threshold = 0.
        self.true = None
        self.target = None
        self.seed = int(np.random.randint(0, 2 ** 31 - 1)) if seed is None else int(seed)
        self.verbose = verbose
        self._stream = 0  # Philox stream id: one per attack() call, as FakeBob counts them
        self.factor = None      # of the last attack(): q of the returned audio (None: no candidate succeeded)
        self.n_queries = 0      # ... and the rows it scored

    def estimate_threshold(self, audio, fs=16000, bits_per_sample=16, n_jobs=10, debug=False, **kw):
        """Kenansville has no threshold sweep of its own (a decision-only attacker cannot run one): the sweep is FakeBob's
        (FAKEBOB.py:39-137), run by a FakeBob over the same model with its default hyper-parameters and this attack's seed, as
        ParticleSwarm.estimate_threshold does.  Keeps the estimate in self.threshold."""
        from .attack import FakeBob
        fb = FakeBob(self.task, self.attack_type, self.model, seed=self.seed, verbose=self.verbose)
        fb._stream = self._stream
        res = fb.estimate_threshold(audio, fs=fs, bits_per_sample=bits_per_sample, n_jobs=n_jobs, debug=debug, **kw)
        self._stream = fb._stream
        if res is not None:
            self.threshold = fb.threshold
        return res

    def attack(self, audio, checkpoint_path, threshold=0., true=None, target=None, fs=16000, bits_per_sample=16, n_jobs=10,
               debug=False, companions=None):
        """companions (needs quorum=): utterances as long as `audio` that ride along, as in FakeBob.attack -- every candidate's
        perturbation is scored on all of them, each (utterance, draw) one vote.  The returned pair is a
        companions.AttackResult: perturbation_i16, apply_perturbation, per_utterance and votes (n_rounds, G) -- the logged
        votes of every candidate (None when the rows were scored once: the checkpoint's decisions are decisions then).
        Returns (int16 adversarial audio (N, 1), success flag +-1), as FakeBob.attack does: the candidate with the smallest
        factor that was seen to succeed -- a row that was scored -- or the int16 cast of the audio with -1.  For SV
        true=None means 1 (the enrolled speaker speaks).  checkpoint_path (or None) receives a pickle (protocol -1) with one
        row per round: [qs, decisions, scores (rows, S), lo, hi, used_time]."""
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
        self.threshold = threshold
        self.true = true
        self.target = target
        p = nes_params(self.task, self.attack_type, threshold=threshold, target=target, true=true, seed=self.seed,
                       stream=self._stream, bits_per_sample=bits)
        k = kv_params(self.window, self.grid, self.q_max, self.max_rounds)
        self._stream += 1
        if self._victim is not None:
            FG.refuse_options("Kenansville", companions=companions)
            eng = self._victim.engine()
            spec = self._victim.spec(self.grid, audio.shape[0], audio, fs, bits_per_sample, n_jobs, debug)
            t0 = time.time()
            res = eng.attack_kenansville_foreign(p, k, spec, audio[:, 0])
            st, rp = QE.Settings("Kenansville", eng, None, None, None, audio.shape[0], bits), 1
        else:
            eng = self.model.engine
            t0 = time.time()
            with QE.Settings("Kenansville", eng, self.eot_size, self.quorum, companions, audio.shape[0], bits) as st:
                res = eng.attack_kenansville(p, k, audio[:, 0])
            rp = st.replicas if st.quorum is not None else 1
        dt = time.time() - t0
        n = res["trace"].shape[0]
        used_time = eng.attack_iter_seconds(n)
        cp = []
        for r in range(n):
            rows = int(res["trace"][r, 2]) // rp     # (the column counts victim queries: rows * r')
            cp.append([res["qs"][r, :rows].copy(), res["decisions"][r, :rows].copy(), res["scores"][r, :rows].copy(),
                       int(res["trace"][r, 0]), int(res["trace"][r, 1]), float(used_time[r])])
        if checkpoint_path:
            with open(checkpoint_path, "wb") as writer:
                pickle.dump(cp, writer, protocol=-1)
        self.factor = res["factor"] if res["success"] == 1 else None
        self.n_queries = res["n_queries"]
        if self.verbose:
            print("--- %d rounds, %d queries, factor %s / 65536, %.3f s ---" % (n, self.n_queries, self.factor, dt))
        return QE.result(self.model, self.task, self.attack_type, res["adv"], res["success"], audio[:, 0], bits, st.comp,
                         res["decisions"] if rp > 1 else None, target=target, true=true, fs=fs, bits_per_sample=bits_per_sample,
                         n_jobs=n_jobs, debug=debug)
