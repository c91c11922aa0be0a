"""Foreign victims of the swarm and the decision-only attacks restated in numpy (the "foreign victims" section of
include/fakebob_hip.h): what the victim sees, the decision rule on its scores, and the three attacks driven against a victim
by the restatements the native attacks are pinned to (hsj_ref.drive, kenansville_ref.search / candidates, pso_ref.replay).
Not part of the product."""
import numpy as np

from tests import hsj_ref as HR
from tests import kenansville_ref as KR


def rows_to_model(q, bits=16, dtype=np.float64):
    """x = (double)q * 2^-(bits - 1), exact; a float32 victim gets the same value, exact too"""
    return (np.asarray(q, np.int16).astype(np.float64) * 2.0 ** -(bits - 1)).astype(dtype)


def decide_rows(task, scores, threshold):
    """scores (rows, S) float32 / float64 -> (decisions (rows,) int32, the scores widened to float64): SV s >= threshold ? 1 :
    -1; OSI / CSI the first maximum by strict > in ascending m, so a NaN never displaces the running maximum (and a NaN in
    column 0 stays it); OSI a maximum < threshold gives -1.  float32 is widened (exactly) before any comparison."""
    sc = np.asarray(scores)
    sc = sc.reshape(sc.shape[0], -1).astype(np.float64)
    thr = float(threshold)
    dec = np.empty(sc.shape[0], np.int32)
    for b, s in enumerate(sc):
        am, best = 0, s[0]
        for m in range(1, s.size):
            if s[m] > best:
                am, best = m, s[m]
        if task == "SV":
            dec[b] = 1 if best >= thr else -1
        else:
            dec[b] = -1 if (task == "OSI" and best < thr) else am
    return dec, sc


# ------------------------------------------------------------------------------------------------ victims
def model_victim(model, bits=16, every_odd_undecided=False):
    """victim(rows int16 (R, N)) -> R decisions, by the model's make_decisions on the audio the engine hands over: the (N, R)
    float64 batch.  every_odd_undecided: -2 for every row whose index in its batch is odd."""
    def victim(rows):
        rows = np.asarray(rows, np.int16)
        out = model.make_decisions(np.ascontiguousarray(rows_to_model(rows, bits).T), bits_per_sample=bits)
        dec = out[0] if isinstance(out, tuple) else out
        dec = [int(v) for v in np.asarray(dec).reshape(-1)]
        assert len(dec) == rows.shape[0]
        if every_odd_undecided:
            dec = [-2 if j % 2 else d for j, d in enumerate(dec)]
        return dec
    return victim


class ScoreOnly(object):
    """a foreign model that has score alone"""

    def __init__(self, model):
        self.m, self.task, self.spk_ids, self.n_calls = model, model.task, model.spk_ids, 0

    def score(self, audios, **kw):
        self.n_calls += 1
        return self.m.score(audios, **kw)


class DecisionsOnly(object):
    """a foreign model that has make_decisions alone; odd_undecided: -2 for every row whose index in its batch is odd;
    scores=False: it returns the decisions without scores"""

    def __init__(self, model, odd_undecided=False, scores=True):
        self.m, self.task, self.spk_ids = model, model.task, model.spk_ids
        self.odd, self.scores, self.n_calls, self.batches = odd_undecided, scores, 0, []

    def make_decisions(self, audios, **kw):
        self.n_calls += 1
        a = np.asarray(audios)
        self.batches.append(a.copy())
        dec, sc = self.m.make_decisions(a, **kw)
        dec = [int(v) for v in np.asarray(dec).reshape(-1)]
        if self.odd:
            dec = [-2 if j % 2 else d for j, d in enumerate(dec)]
        if len(dec) == 1:
            dec = dec[0]
        return (dec, sc) if self.scores else dec


# ------------------------------------------------------------------------------------------------ whole attacks
def drive_hsj(victim, a, init, params, attack_type, label, noise, seed, stream, max_iter, bits=16):
    """hsj_ref.drive against victim(rows) (noise: oracle.noise)"""
    return HR.drive(a, init, params, attack_type, label, noise, seed, stream, max_iter, victim=victim, bits=bits)


def drive_kenansville(victim, a, W, G, q_max, max_rounds, attack_type, label, bits=16):
    """kenansville_ref.search against victim(rows) -> dict(success, factor, n_queries, qs, decisions, trace, adv, x): the
    outputs of fb_attack_kenansville(_foreign), unused places -1 (qs) and -3 (decisions)"""
    x = HR.cast_i16(a, bits)
    log, kept = [], {}

    def ok(r, qs):
        rows = KR.candidates(x, W, qs)
        d = victim(rows)
        log.append([int(v) for v in d])
        flags = [KR.succeeds(v, attack_type, label) for v in d]
        if any(flags):
            kept["row"], kept["d"] = rows[flags.index(True)].copy(), d[flags.index(True)]
        return flags
    res = KR.search(ok, G, q_max, max_rounds)
    n = len(res["rounds"])
    qs, dec = np.full((n, G), -1, np.int32), np.full((n, G), -3, np.int32)
    trace = np.zeros((n, 3), np.int32)
    for r, rd in enumerate(res["rounds"]):
        qs[r, :rd["rows"]] = rd["qs"]
        dec[r, :rd["rows"]] = log[r]
        trace[r] = (rd["lo"], -1 if rd["hi"] is None else rd["hi"], rd["rows"])
    return dict(success=res["success"], factor=res["factor"], n_queries=res["n_queries"], qs=qs, decisions=dec, trace=trace,
                adv=kept["row"] if res["success"] == 1 else x, adopted=kept.get("d"), x=x)
