"""Voted decisions: what ParticleSwarm, Kenansville and HopSkipJump share when they attack a randomised victim or several
utterances at once (fb_set_query_eot; the "voted decisions" section of include/fakebob_hip.h).

Every candidate row is scored r' = K * eot_size times; PSO reads the mean loss, the decision-only attacks the number of
adversarial replicas -- the row's vote -- against a quorum.  Here: the argument rules of `eot_size=`, `quorum=` and
`attack(..., companions=[...])`, the engine settings around one attack() call, and the result FakeBob.attack returns.
Nothing here runs on the hot path."""
import numpy as np

from . import companions as CP

MAX_REPLICAS = CP.MAX_REPLICAS
MAJORITY = "majority"


def quorum_code(quorum):
    """`quorum` as fb_set_query_eot takes it: None -> 0 (off), "majority" or -1 -> -1, an int 1 .. 32 as it is."""
    if quorum is None:
        return 0
    if quorum == MAJORITY:
        return -1
    if isinstance(quorum, (bool, str)) or int(quorum) != quorum:
        raise ValueError("quorum %r: None, \"majority\" or 1 .. %d" % (quorum, MAX_REPLICAS))
    q = int(quorum)
    if q != -1 and not 1 <= q <= MAX_REPLICAS:
        raise ValueError("quorum %d outside 1 .. %d" % (q, MAX_REPLICAS))
    return q


def majority(replicas):
    """The majority quorum of r' replicas: r' // 2 + 1."""
    return int(replicas) // 2 + 1


def check_options(who, eot_size, quorum):
    """The constructor's check -> (eot_size or None, quorum): eot_size > 1 needs a quorum (None means the switch is off and
    the library would refuse the attack), and an explicit quorum cannot exceed 32.  Touches no engine."""
    quorum_code(quorum)
    if eot_size is not None:
        eot_size = int(eot_size)
        if not 1 <= eot_size <= MAX_REPLICAS:
            raise ValueError("eot_size %d outside 1 .. %d" % (eot_size, MAX_REPLICAS))
        if eot_size > 1 and quorum is None:
            raise ValueError("%s under eot_size=%d needs quorum= (\"majority\" or 1 .. %d): a row scored %d times has votes, "
                             "not a decision" % (who, eot_size, MAX_REPLICAS, eot_size))
    return eot_size, quorum


class Settings(object):
    """The engine's settings for ONE attack() call: the switch, the EOT size and the companions go on, the attack runs, and
    all three go back to what they were -- also when the attack raises.  Without a quorum nothing of the engine is read or
    set: the attack runs as it always did."""

    def __init__(self, who, engine, eot_size, quorum, companions, n, bits):
        if companions is not None and quorum is None:
            raise ValueError("%s with companions needs quorum= (\"majority\" or 1 .. %d)" % (who, MAX_REPLICAS))
        self.engine = engine
        self.eot_size = eot_size
        self.quorum = quorum
        self.comp = CP.as_companions(companions, n, bits) if companions is not None else None
        # (without companions= the engine keeps the companions it has: they count)
        held = self.comp if (self.comp is not None or quorum is None) else engine.companions
        K = 1 + (0 if held is None else held.shape[0])
        self.replicas = 1 if quorum is None else K * (eot_size if eot_size is not None else engine.eot)
        if self.replicas > MAX_REPLICAS:
            raise ValueError("%d utterances * eot %d: at most %d replicas per row" % (K, self.replicas // K, MAX_REPLICAS))

    @property
    def needed(self):
        """the votes a row needs (None: the switch is off)"""
        if self.quorum is None:
            return None
        q = quorum_code(self.quorum)
        return majority(self.replicas) if q == -1 else q

    def __enter__(self):
        if self.quorum is None:
            return self
        eng = self.engine
        self._before = (eng.query_eot, eng.eot, eng.companions)
        try:
            eng.set_query_eot(self.quorum)
            if self.comp is not None:
                eng.set_eot(1)                  # (the product K * eot is checked at every setting: through 1)
                eng.set_companions(self.comp)
            if self.eot_size is not None:
                eng.set_eot(self.eot_size)
        except Exception:
            self._restore()
            raise
        return self

    def _restore(self):
        eng = self.engine
        q, r, comp = self._before
        eng.set_eot(1)
        eng.set_companions(comp)
        eng.set_eot(r)
        eng.set_query_eot(q)

    def __exit__(self, *exc):
        if self.quorum is not None:
            self._restore()
        return False


def result(model, task, attack_type, adv, flag, audio, bits, comp, votes, target=None, true=None, **score_kw):
    """What FakeBob.attack returns -- a companions.AttackResult (it unpacks as the pair) with perturbation_i16,
    apply_perturbation and, with companions, per_utterance: every composed utterance re-scored through make_decisions --
    carrying `votes` as well (None when the rows were scored once)."""
    a0 = CP.cast_i16(audio, bits)
    adv = np.asarray(adv, np.int16).reshape(-1)
    delta = adv.astype(np.int32) - a0.astype(np.int32)
    per = None
    if comp is not None:
        per = []
        for u, w in enumerate([adv] + CP.apply_perturbation(delta, list(comp))):
            dec, sc = model.make_decisions(w, **score_kw)
            per.append(dict(utterance=u, audio_i16=w, decision=dec, score=sc,
                            success=CP.succeeded(task, attack_type, dec, target=target, true=true)))
    res = CP.AttackResult(adv[:, np.newaxis], flag, delta, bits, per)
    res.votes = votes
    return res
