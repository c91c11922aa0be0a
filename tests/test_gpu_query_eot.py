"""Voted decisions on the device (fb_set_query_eot; the "voted decisions" section of include/fakebob_hip.h): k_vote alone against
the numpy restatement (tests/vote_ref.py) bit for bit, the three query attacks under EOT and companions on a deterministic
victim (nothing may change), on a randomised victim (row 0 pinned to the NES path, whole attacks replayed from their logged
votes and mean losses), a quorum that decides a round, companions, the refusals, and the driver.

Bit-exact checks use np.array_equal.  Every test here fails without the feature: the symbol is missing or the call is refused."""
import contextlib
import io
import os

import numpy as np
import pytest

from fakebob_amd import attack_main as AM
from fakebob_amd import companions as CP
from fakebob_amd._native import FB_E_ARG, FB_E_LIMIT, FB_E_STATE, NativeError
from fakebob_amd.engine import Engine, hsj_params, kv_params, nes_params, pso_params
from fakebob_amd.hsj import HopSkipJump
from fakebob_amd.models import synthetic_audio, synthetic_gmm_system
from fakebob_amd.pso import ParticleSwarm
from tests import hsj_ref as HR
from tests import kenansville_ref as KR
from tests import pso_ref as PR
from tests import test_gpu_hsj as TH
from tests import test_gpu_kenansville as TK
from tests import test_gpu_pso as TP
from tests import vote_ref as V
from tests.golden import driver_site as DS
from tests.test_gpu_input_transform import SCORE_TOL   # the bound between an NES batch's row and a scoring call

pytestmark = pytest.mark.gpu
N = 4000                                               # the utterance length of tests/test_gpu_pso.py
W0 = 100
HP = dict(HR.DEFAULTS, num_evals_init=8, num_evals_max=24, max_rounds=4)     # HopSkipJump at a size a test can afford
PSO_ITERS = 6


def _sub(tmp_path, name):
    d = tmp_path / name
    d.mkdir()
    return d


def _code(fn):
    with pytest.raises(NativeError) as ei:
        fn()
    return ei.value.code, str(ei.value)


# ------------------------------------------------------------------------------------- 1. the kernel alone, bit for bit
_engines = {}


@pytest.fixture(scope="module")
def vote_engines():
    """one engine per (S, task): a GMM system of S speakers -- the hook reads n_out, S and the z-norm tables from it"""
    made = []

    def get(S, task):
        if (S, task) not in _engines:
            ubm, spk = synthetic_gmm_system(n_speakers=S, C=64, D=72)
            e = Engine(0)
            if task == "CSI":
                zm = -80.0 + 0.5 * np.arange(S)
                zs = 2.0 + 0.25 * (np.arange(S) % 5)
                zm[1 % S], zs[1 % S] = zm[0], zs[0]                               # speakers 0 and 1 share a z-norm: raw ties are score ties
                e.load_gmm(spk)
                e.set_system("CSI", zm, zs)
                e.z = (zm, zs)
            else:
                e.load_gmm([ubm] + spk)
                e.set_system(task)
                e.z = (None, None)
            _engines[(S, task)] = e
            made.append(e)
        return _engines[(S, task)]
    yield get
    for e in made:
        e.close()
    _engines.clear()


def _planted_raw(task, rows, r, S, thr, rng):
    """raw scores (rows, r, M) and tv (rows, r): random, with planted ties between speakers 0 and 1, maxima that equal the
    threshold, replicas without voiced frames and (rows > 1) a row without any"""
    M = S if task == "CSI" else S + 1
    raw = np.round(rng.normal(-80.0, 3.0, (rows, r, M)) * 64.0) / 64.0              # (dyadic: differences are exact, ties abound)
    tv = rng.randint(1, 50, (rows, r)).astype(np.int32)
    first = 0 if task == "CSI" else 1                                             # the column of speaker 0
    for b in range(rows):
        for j in range(r):
            kind = (b * 7 + j * 3) % 5
            if kind == 0 and S >= 2:                                              # a tie at the top: the first maximum wins
                top = raw[b, j].max() + 1.0
                raw[b, j, first], raw[b, j, first + 1] = top, top
            elif kind == 1 and task != "CSI":                                     # the maximum equals the threshold exactly
                raw[b, j, 0] = 0.0
                raw[b, j, 1:] = np.minimum(raw[b, j, 1:], thr - 1.0)
                raw[b, j, 1 + (b + j) % S] = thr
            elif kind == 2:
                tv[b, j] = 0 if (b + j) % 2 else -3
    if rows > 1:
        tv[rows // 2, :] = 0                                                      # a row whose replicas all lack voiced frames
    else:
        tv[0, 0] = 0
    return raw, tv


SHAPES = [(1, 2, 1), (3, 3, 3), (64, 32, 3), (1023, 5, 1), (65, 7, 60)]           # odd sizes, tails of a 4-row workgroup, 60 speakers


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_k_vote_equals_the_restatement(vote_engines, shape):
    rows, r, S_shape = shape
    rng = np.random.RandomState(rows * 100 + r)
    thr = -77.5
    # (an engine takes 60 models: 60 speakers is CSI's limit, a UBM and 59 speakers OSI's)
    for task, S in {1: [("SV", 1)], 3: [("OSI", 3), ("CSI", 3)], 60: [("CSI", 60), ("OSI", 59)]}[S_shape]:
        e = vote_engines(S, task)
        assert e.n_speakers == S
        raw, tv = _planted_raw(task, rows, r, S, thr, rng)
        sc = V.system_scores(task, raw, *e.z)
        labels = {"SV": [1, -1], "OSI": [-1, 0, S - 1], "CSI": [0, 1 % S, S - 1]}[task]
        seen = set()
        for at in ("targeted", "untargeted"):
            for label in labels:
                votes, nodec, mean = e.debug_vote(raw, tv, task, thr, at, label)
                want = V.vote(task, at, label, thr, sc, tv)
                assert votes.dtype == np.int32 and nodec.dtype == np.int32 and mean.dtype == np.float64
                for g, w, what in zip((votes, nodec, mean), want, ("votes", "nodec", "mean")):
                    assert g.shape == w.shape and np.array_equal(g, w), (what, shape, task, at, label)
                seen.update(votes.tolist())
        assert nodec.max() == r or rows == 1
        assert len(seen) > 1 or rows * r <= 2, seen                               # the cases do vote differently
    # what the hook refuses
    assert _code(lambda: e.debug_vote(raw[:, :1].repeat(33, axis=1), np.ones(rows * 33), task, thr, "targeted", labels[-1]))[0] == FB_E_ARG
    assert _code(lambda: e.debug_vote(raw, tv, task, thr, "targeted", S + 5))[0] == FB_E_ARG
    wide = np.zeros((2048, 32, raw.shape[2]))                                     # 65536 replica rows: one more than a batch takes
    assert _code(lambda: e.debug_vote(wide, np.ones(2048 * 32), task, thr, "targeted", labels[-1]))[0] == FB_E_LIMIT


# ------------------------------------------------------------------------------------- the three attacks on small systems
def _pso_run(e, task, at, kw, audio, stream=1, max_iter=PSO_ITERS):
    p = nes_params(task, at, epsilon=TP.EPS, max_iter=max_iter, seed=5, stream=stream, **kw)
    adv, flag, adv_f, trace, losses = e.attack_pso(p, pso_params(**TP.PSO), audio)
    return dict(adv=adv, flag=flag, adv_f=adv_f, trace=trace, losses=losses)


def _pso_case(case, small_system, d, **kw):
    task, at, pk = TP.CASES[case]
    model = TP._system(case, small_system, d, **kw)
    audio = synthetic_audio(9, N)
    if task == "CSI":
        pk = dict(pk, true=2)
    return model, task, at, pk, audio


def _kv_case(case, small_system, d, targeted=False, **kw):
    """-> model, task, attack type, label, threshold, G, q_max, audio: the evasion settings of tests/test_gpu_kenansville.py.
    targeted=True (a deterministic victim): the target is the first decision of round 0's candidates, by scoring calls, that is
    a speaker other than the clean one."""
    task = case.split()[1]
    G, audio_seed, q_max = TK.CASES[case]
    G = max(G, 4)
    if task == "SV":        # (not monotone in q, and not the same under a defence: a round 0 of 15 rows up to a quarter)
        G, q_max = 15, 16384
    model = TK._system(case, small_system, d, **kw)
    audio = synthetic_audio(audio_seed, N)
    x = CP.cast_i16(audio, 16)
    thr, true = TK._goal(model.engine, task, x)
    if not targeted:
        return model, task, "untargeted", true, thr, G, q_max, audio
    qs, _last = KR.round_candidates(0, 0, None, G, q_max)
    sc = TK._scores_tolerant(model.engine, KR.candidates(x, W0, qs))
    others = [KR.decide(task, s, thr) for s in sc if s is not None]
    others = [v for v in others if v not in (true, -1)]
    assert others, "no candidate of round 0 is taken for another speaker"
    return model, task, "targeted", others[0], thr, G, q_max, audio


def _kv_run(e, task, at, label, thr, G, q_max, audio, stream=1, seed=5, max_rounds=6):
    key = "target" if at == "targeted" else "true"
    p = nes_params(task, at, threshold=thr, seed=seed, stream=stream, **{key: label})
    return e.attack_kenansville(p, kv_params(W0, G, q_max, max_rounds), audio)


def _hsj_case(case, small_system, d, **kw):
    """-> model, task, attack type, label, threshold, audio, init.  gmm OSI is TARGETED at the speaker the start is taken for."""
    task = case.split()[1]
    model = TH._system(case, small_system, str(d), **kw)
    audio, init, at, label, thr = TH._setting(model.engine, case)
    if task == "OSI":
        at, label = "targeted", KR.decide("OSI", TH._scores(model.engine, [CP.cast_i16(init, 16)])[0], thr)
        assert label >= 0
    return model, task, at, label, thr, audio, init


def _hsj_run(e, task, at, label, thr, audio, init, stream=1, max_iter=2, hp=HP, **kw):
    return e.attack_hsj(TH._params(at, label, thr, task, stream=stream, max_iter=max_iter), hsj_params(**hp), audio, init, **kw)


@contextlib.contextmanager
def _voted(e, quorum, eot=1, companions=None):
    e.set_query_eot(quorum)
    e.set_eot(1)
    e.set_companions(companions)
    e.set_eot(eot)
    try:
        yield
    finally:
        e.set_eot(1)
        e.set_companions(None)
        e.set_query_eot(None)


SETTINGS = [(2, 1, "majority"), (5, 1, 1), (5, 1, "majority"), (5, 1, 5), (1, 2, "majority"), (2, 2, 3)]   # (eot, K, quorum)


def _settings(audio):
    for eot, K, quorum in SETTINGS:
        yield eot, K, quorum, ([CP.cast_i16(audio, 16)] * (K - 1) if K > 1 else None)   # the companion is a_0: the composed row is the row


# ------------------------------------------------------------------------------------- 2. a deterministic victim: nothing changes
@pytest.mark.parametrize("case", sorted(TP.CASES))
def test_pso_on_a_deterministic_victim_is_the_plain_attack(small_system, tmp_path, case):
    model, task, at, pk, audio = _pso_case(case, small_system, tmp_path, input_transform="ms:3")
    e = model.engine
    try:
        base = _pso_run(e, task, at, pk, audio)
        with _voted(e, "majority"):                                                # the switch on with r' = 1: the same run
            same = _pso_run(e, task, at, pk, audio)
        assert all(np.array_equal(base[k], same[k]) for k in base)
        for eot, K, quorum, comp in _settings(audio):
            before = e.stats()
            with _voted(e, quorum, eot, comp):
                got = _pso_run(e, task, at, pk, audio)
            n = got["trace"].shape[0]
            assert e.stats()["scored_utts"] - before["scored_utts"] == 8 * n * eot * K
            if eot * K == 2:                                                       # (l + l) / 2 is exact
                for k in base:
                    assert np.array_equal(base[k], got[k]), (case, eot, K, k)
            else:                                                                  # a mean of five equal values may round
                assert np.allclose(base["losses"][:1], got["losses"][:1], rtol=0, atol=1e-9)
    finally:
        e.close()


@pytest.mark.parametrize("case", sorted(TK.CASES))
def test_kenansville_on_a_deterministic_victim_is_the_plain_attack(small_system, tmp_path, case):
    model, task, at, label, thr, G, q_max, audio = _kv_case(case, small_system, tmp_path, targeted=case == "gmm OSI",
                                                            input_transform="ms:3")
    e = model.engine
    try:
        base = _kv_run(e, task, at, label, thr, G, q_max, audio)
        print(case, at, label, "trace", base["trace"].tolist())
        flags = np.array([[KR.succeeds(int(d), at, label) if d != -3 else False for d in row] for row in base["decisions"]])
        assert base["success"] == 1 and base["trace"].shape[0] > 1
        with _voted(e, "majority"):
            same = _kv_run(e, task, at, label, thr, G, q_max, audio)
        assert all(np.array_equal(base[k], same[k], equal_nan=(k == "scores")) for k in base)
        for eot, K, quorum, comp in _settings(audio):
            rp = eot * K
            before = e.stats()
            with _voted(e, quorum, eot, comp):
                got = _kv_run(e, task, at, label, thr, G, q_max, audio)
            assert e.stats()["scored_utts"] - before["scored_utts"] == got["n_queries"] == rp * base["n_queries"]
            for k in ("qs", "adv", "factor", "success"):
                assert np.array_equal(base[k], got[k]), (case, eot, K, quorum, k)
            assert np.array_equal(got["trace"][:, :2], base["trace"][:, :2]) and np.array_equal(got["trace"][:, 2], rp * base["trace"][:, 2])
            used = base["decisions"] != -3
            assert np.array_equal(got["decisions"] != -3, used)
            assert np.array_equal(got["decisions"][used], rp * flags[used])          # votes: r' times the plain flag
            if rp == 2:
                assert np.array_equal(base["scores"], got["scores"], equal_nan=True)
    finally:
        e.close()


@pytest.mark.parametrize("case", ["gmm CSI", "gmm OSI", "ivector SV"])
def test_hsj_on_a_deterministic_victim_is_the_plain_attack(small_system, tmp_path, case):
    model, task, at, label, thr, audio, init = _hsj_case(case, small_system, tmp_path, input_transform="ms:3")
    e = model.engine
    try:
        base = _hsj_run(e, task, at, label, thr, audio, init)
        flags = np.array([HR.adversarial(int(d), at, label) for d in base["decisions"]])
        assert base["success"] == 1 and base["n_iters"] >= 1
        with _voted(e, "majority"):
            same = _hsj_run(e, task, at, label, thr, audio, init)
        assert all(np.array_equal(base[k], same[k]) for k in base)
        for eot, K, quorum, comp in _settings(audio):
            rp = eot * K
            before = e.stats()
            with _voted(e, quorum, eot, comp):
                got = _hsj_run(e, task, at, label, thr, audio, init)
            assert e.stats()["scored_utts"] - before["scored_utts"] == got["n_queries"] == rp * base["n_queries"]
            for k in ("adv", "adv_f64", "dist2", "success", "n_iters"):
                assert np.array_equal(base[k], got[k]), (case, eot, K, quorum, k)
            cols = [0, 1, 2, 3, 4, 5, 7]
            assert np.array_equal(got["trace"][:, cols], base["trace"][:, cols]) and np.array_equal(got["trace"][:, 6], rp * base["trace"][:, 6])
            assert np.array_equal(got["decisions"], rp * flags)                      # votes: r' times the plain flag
    finally:
        e.close()


# ------------------------------------------------------------------------------------- 3. a randomised victim: row 0 on the NES path
def _row0(e, task, at, kw, row, epoch, seed=5, stream=1):
    """Engine.get_grad of `row` (float64) at the epoch: the NES path's mean loss and mean scores of its row 0 under the engine's
    EOT and companions"""
    p = nes_params(task, at, samples_per_draw=2, sigma=1e-3, seed=seed, stream=stream, **kw)
    _fl, _g, al, sc0 = e.get_grad(p, row, it=epoch, want_grad=False)
    return al, sc0[:e.n_speakers]


@pytest.mark.parametrize("victim", [dict(input_transform="at:20"), dict(input_transform="at:20", air_channel="t60:200-600,drr:6")],
                         ids=["at", "at+air"])
def test_row_0_of_a_randomised_victim_is_the_nes_path(small_system, oracle, tmp_path, victim):
    worst = 0.0
    # PSO: particle 0's mean loss in every iteration
    model, task, at, pk, audio = _pso_case("gmm OSI targeted", small_system, _sub(tmp_path, "p"), **victim)
    e = model.engine
    try:
        with _voted(e, "majority", 3):
            got = _pso_run(e, task, at, pk, audio, max_iter=4)
            n = got["trace"].shape[0]
            rep = PR.replay(oracle.philox, audio, got["losses"], eps=TP.EPS, max_iter=4, P=8, w_init=TP.PSO["w_init"], w_end=TP.PSO["w_end"],
                            c1=TP.PSO["c1"], c2=TP.PSO["c2"], v_max=TP.PSO["v_max"], seed=5, stream=1, keep=tuple(range(n)))
            want = [_row0(e, task, at, pk, rep["positions"][k][0], k)[0] for k in range(n)]
        assert np.all(np.isfinite(got["losses"])) and np.all(np.isfinite(want))
        worst = max(worst, np.abs(got["losses"][:, 0] - want).max())
        assert np.array_equal(got["losses"][:, 0], np.asarray(want, np.float64))
        assert np.ptp(got["losses"][:, 0]) > 0                                      # the draws differ from epoch to epoch
    finally:
        e.close()
    # Kenansville: candidate 0's mean scores in every round
    model, task, at, label, thr, G, q_max, audio = _kv_case("gmm OSI", small_system, _sub(tmp_path, "k"), **victim)
    e = model.engine
    try:
        with _voted(e, "majority", 3):
            res = _kv_run(e, task, at, label, thr, G, q_max, audio)
            x = CP.cast_i16(audio, 16)
            means = []
            for r in range(res["trace"].shape[0]):
                row = KR.candidates(x, W0, [int(res["qs"][r, 0])])[0]
                _al, sc0 = _row0(e, task, "untargeted", dict(threshold=thr), row.astype(np.float64) / 32768.0, r)
                assert np.all(np.isfinite(res["scores"][r, 0])) and np.all(np.isfinite(sc0))
                worst = max(worst, np.abs(res["scores"][r, 0] - sc0).max())
                assert np.array_equal(res["scores"][r, 0], sc0), (r, res["scores"][r, 0], sc0)
                means.append(res["scores"][r, 0])
        print("Kenansville under", victim, "trace", res["trace"].tolist(), "votes", res["decisions"].tolist())
        assert res["trace"].shape[0] >= 2 and np.ptp(np.array(means)[:, 0]) > 0
    finally:
        e.close()
    print("row 0 against Engine.get_grad: max difference %.3g (the suite's bound 2 * SCORE_TOL = %.3g)" % (worst, 2 * SCORE_TOL))
    assert worst == 0.0


# ------------------------------------------------------------------------------------- 4. replays from the logged votes
def _as_decisions(votes, quorum, at, label):
    """votes -> stand-in decisions for the restatements' drivers: the label or not the label"""
    other = -2
    if at == "targeted":
        return [label if v >= quorum else other for v in votes]
    return [(label + 1 if label >= 0 else 0) if v >= quorum else label for v in votes]


def test_kenansville_replays_from_its_votes(small_system, tmp_path):
    runs = []
    for stream in (2, 2, 3):
        model, task, at, label, thr, G, q_max, audio = _kv_case("gmm OSI", small_system, tmp_path, input_transform="at:20")
        e = model.engine
        try:
            with _voted(e, "majority", 4):
                runs.append(_kv_run(e, task, at, label, thr, G, q_max, audio, stream=stream))
        finally:
            e.close()
    res, quorum = runs[0], V.majority(4)

    def ok(r, qs):
        rows = int(res["trace"][r, 2]) // 4
        assert rows == len(qs) and res["qs"][r, :rows].tolist() == qs and np.all(res["qs"][r, rows:] == -1)
        v = res["decisions"][r, :rows]
        assert np.all((v >= 0) & (v <= 4))
        return V.flags(v, quorum)
    want = KR.search(ok, G, q_max, 6)
    print("votes", res["decisions"].tolist(), "trace", res["trace"].tolist())
    assert len(want["rounds"]) == res["trace"].shape[0] and np.ptp(res["decisions"][res["decisions"] >= 0]) > 0
    for r, rd in enumerate(want["rounds"]):
        assert res["trace"][r].tolist() == [rd["lo"], -1 if rd["hi"] is None else rd["hi"], 4 * rd["rows"]]
    assert (res["success"], res["factor"], res["n_queries"]) == (want["success"], want["factor"], 4 * want["n_queries"])
    assert all(np.array_equal(res[k], runs[1][k], equal_nan=(k == "scores")) for k in res)   # (seed, stream) decide everything
    assert not np.array_equal(res["scores"][0], runs[2]["scores"][0], equal_nan=True)        # another stream: other draws


def test_hsj_replays_from_its_votes(small_system, oracle, tmp_path):
    runs = []
    for stream in (2, 2, 3):
        model, task, at, label, thr, audio, init = _hsj_case("gmm CSI", small_system, tmp_path, input_transform="at:20")
        e = model.engine
        try:
            with _voted(e, "majority", 4):
                runs.append(_hsj_run(e, task, at, label, thr, audio, init, stream=stream, keep_x=True))
        finally:
            e.close()
    res, quorum = runs[0], V.majority(4)
    assert res["decisions"].size * 4 == res["n_queries"] and np.all((res["decisions"] >= 0) & (res["decisions"] <= 4))
    want = HR.drive(audio, init, HP, at, label, oracle.noise, 5, 2, 2, decisions=_as_decisions(res["decisions"], quorum, at, label))
    assert (res["success"], res["n_iters"], res["n_queries"]) == (want["success"], want["n_iters"], 4 * want["n_queries"])
    cols = [0, 1, 2, 3, 4, 5, 7]
    assert np.array_equal(res["trace"][:, cols], want["trace"][:, cols]) and np.array_equal(res["trace"][:, 6], 4 * want["trace"][:, 6])
    assert res["dist2"] == want["dist2"] and np.array_equal(res["adv"], want["adv"]) and np.array_equal(res["adv_f64"], want["x"])
    for t, x in enumerate(want["xs"]):
        assert np.array_equal(res["xs"][t], x)
    assert all(np.array_equal(res[k], runs[1][k]) for k in res)
    assert not np.array_equal(res["decisions"], runs[2]["decisions"]) or not np.array_equal(res["adv"], runs[2]["adv"])


def test_pso_replays_from_its_mean_losses(small_system, philox_fn, tmp_path):
    runs = []
    for stream in (2, 2, 3):
        model, task, at, pk, audio = _pso_case("gmm CSI untargeted", small_system, tmp_path, input_transform="at:20")
        e = model.engine
        try:
            with _voted(e, "majority", 4):
                runs.append(_pso_run(e, task, at, pk, audio, stream=stream))
        finally:
            e.close()
    got = runs[0]
    n = got["trace"].shape[0]
    r = PR.replay(philox_fn, audio, got["losses"], eps=TP.EPS, max_iter=PSO_ITERS, P=8, w_init=TP.PSO["w_init"], w_end=TP.PSO["w_end"],
                  c1=TP.PSO["c1"], c2=TP.PSO["c2"], v_max=TP.PSO["v_max"], seed=5, stream=2)
    assert (r["n_iters"], r["success"]) == (n, got["flag"])
    assert np.array_equal(got["trace"][:, :3], r["trace"])
    assert np.array_equal(got["adv_f"], r["adv_f64"]) and np.array_equal(got["adv"], r["adv_i16"])
    assert all(np.array_equal(got[k], runs[1][k]) for k in got)
    assert not np.array_equal(got["losses"], runs[2]["losses"])


@pytest.fixture(scope="module")
def philox_fn(oracle):
    return oracle.philox


# ------------------------------------------------------------------------------------- 5. the quorum is live
QUORUM_SEED = 5          # a seed whose round 0 under at:20, eot = 8 logs a vote strictly between 0 and 8


def test_the_quorum_decides_a_round(small_system, tmp_path):
    """An OSI victim under at:20.  A first run without a threshold gives round 0's mean scores; the threshold is then put on
    the mean best score of a candidate, so that its eight replicas fall on both sides of it -- the draws depend on (seed,
    stream, epoch) alone, so every later run sees the same replicas."""
    model, task, _at, _label, _thr, _G, q_max, audio = _kv_case("gmm OSI", small_system, tmp_path, input_transform="at:20")
    e = model.engine
    G = 6
    try:
        with _voted(e, 1, 8):
            free = _kv_run(e, task, "targeted", -1, -1e9, G, q_max, audio, seed=QUORUM_SEED, max_rounds=1)
        rows = int(free["trace"][0, 2]) // 8
        best = free["scores"][0, :rows].max(axis=1)
        thr = float(best[rows // 2])                                               # the middle candidate's mean best score
        with _voted(e, 1, 8):
            probe = _kv_run(e, task, "targeted", -1, thr, G, q_max, audio, seed=QUORUM_SEED, max_rounds=1)
        assert np.array_equal(probe["scores"], free["scores"], equal_nan=True)       # the same draws
        votes = probe["decisions"][0, :rows]
        print("round 0 votes for a rejection at seed %d, threshold %.6f: %s" % (QUORUM_SEED, thr, votes.tolist()))
        split = [int(v) for v in votes if 0 < v < 8]
        assert split, "no candidate of round 0 splits its replicas: pick another QUORUM_SEED"
        first_at = lambda q: int(np.flatnonzero(votes >= q)[0]) if np.any(votes >= q) else -1   # noqa: E731
        pick = [v for v in sorted(set(split)) if first_at(v) != first_at(v + 1)]
        assert pick, "a row in front of every split one takes all eight votes: pick another QUORUM_SEED"
        v = pick[0]
        runs = {}
        for quorum in (v, v + 1):
            with _voted(e, quorum, 8):
                runs[quorum] = _kv_run(e, task, "targeted", -1, thr, G, q_max, audio, seed=QUORUM_SEED, max_rounds=1)
            assert np.array_equal(runs[quorum]["decisions"][0], probe["decisions"][0])    # the same draws, the same votes
            j = first_at(quorum)
            assert runs[quorum]["trace"][0, 1] == (probe["qs"][0, j] if j >= 0 else -1)     # hi: the first row that reaches the quorum
        assert first_at(v) != first_at(v + 1)
        assert runs[v]["trace"][0].tolist() != runs[v + 1]["trace"][0].tolist()             # the round brackets differently
    finally:
        e.close()


# ------------------------------------------------------------------------------------- 6. companions
def _check_result(res, model, e, comps, audio):
    adv, flag = res
    assert adv.shape == (N, 1) and flag in (1, -1)
    assert len(res.per_utterance) == len(comps) + 1
    rows = res.apply_perturbation([audio] + comps)
    assert np.array_equal(rows[0], adv[:, 0])
    for u, per in enumerate(res.per_utterance):
        assert per["utterance"] == u and np.array_equal(per["audio_i16"], rows[u])
        dec, _sc = model.make_decisions(rows[u])
        assert int(np.asarray(dec).reshape(-1)[0]) == int(np.asarray(per["decision"]).reshape(-1)[0])
    assert e.companions is None and e.eot == 1 and e.query_eot is None            # the engine is as it was


def test_companions_ride_along(small_system, tmp_path):
    comps = [synthetic_audio(u, N) for u in (1, 3, 7)]
    model, task, at, label, thr, audio, init = _hsj_case("gmm CSI", small_system, _sub(tmp_path, "h"))
    e = model.engine
    try:
        hsj = HopSkipJump(task, at, model, max_iter=1, seed=5, verbose=False, eot_size=2, quorum="majority", **HP)
        res = hsj.attack(audio, None, threshold=thr, target=label, init=init, companions=comps)
        _check_result(res, model, e, comps, audio)
        assert res.votes is not None and res.votes.size * 8 == hsj.n_queries and res.votes.max() <= 8
        with pytest.raises(ValueError):                                             # a companion of another length: raised ...
            hsj.attack(audio, None, threshold=thr, target=label, init=init, companions=[comps[0][:-1]])
        with pytest.raises(NativeError):                                            # ... and an error inside the attack:
            HopSkipJump(task, at, model, max_iter=1, seed=5, verbose=False, eot_size=2, quorum=32, **HP).attack(
                audio, None, threshold=thr, target=label, init=init, companions=comps)
        assert e.companions is None and e.eot == 1 and e.query_eot is None        # cleared both times
    finally:
        e.close()
    model, task, at, pk, audio = _pso_case("gmm OSI targeted", small_system, _sub(tmp_path, "p"))
    e = model.engine
    try:
        pso = ParticleSwarm(task, at, model, adver_thresh=pk["adver_thresh"], epsilon=TP.EPS, max_iter=3, n_particles=8, seed=5,
                            verbose=False, eot_size=2, quorum="majority")
        before = e.stats()
        res = pso.attack(audio, None, threshold=pk["threshold"], target=pk["target"], companions=comps)
        assert (e.stats()["scored_utts"] - before["scored_utts"] - 4) % (8 * 8) == 0   # (the four re-scored utterances)
        _check_result(res, model, e, comps, audio)
        assert res.votes is None
    finally:
        e.close()


# ------------------------------------------------------------------------------------- 7. refusals and state
def test_refusals_and_state(small_system, tmp_path):
    """(The header's FB_E_LIMIT for max(grid, num_evals_max) * r' > 65535 cannot be reached through the public ranges -- 1024
    probes * 32 replicas are 32768 rows -- so no call here can ask for it.)"""
    comp = [CP.cast_i16(synthetic_audio(3, N), 16)]
    model, task, at, label, thr, G, q_max, audio = _kv_case("gmm OSI", small_system, tmp_path)
    e = model.engine
    try:
        init = synthetic_audio(5, N)
        small = dict(HP, grid=3, max_rounds=1, num_evals_init=4, num_evals_max=4)
        calls = {"fb_attack_kenansville": lambda: _kv_run(e, task, at, label, thr, G, q_max, audio),
                 "fb_attack_hsj": lambda: _hsj_run(e, task, "untargeted", -1, thr, audio, init, max_iter=1, hp=small),
                 "fb_attack_pso": lambda: _pso_run(e, task, "targeted", dict(target=1, threshold=thr, adver_thresh=1e3), audio, max_iter=2)}
        plain = {k: fn() for k, fn in calls.items()}

        def unchanged():
            for k, fn in calls.items():
                got = fn()
                assert all(np.array_equal(got[key], plain[k][key], equal_nan=True) for key in got), k

        def refused_as_before():
            for name, fn in calls.items():
                e.set_eot(2)
                code, msg = _code(fn)
                assert code == FB_E_STATE and name in msg and "fb_set_eot(2)" in msg
                e.set_eot(1)
                e.set_companions(comp)
                code, msg = _code(fn)
                assert code == FB_E_STATE and name in msg and "fb_set_companions" in msg
                e.set_companions(None)
        refused_as_before()                                                       # the switch off: exactly today's refusals
        for bad in (33, -2, 100):                                                 # a bad quorum keeps the previous value: off ...
            assert e._L.fb_set_query_eot(e._h, bad) == FB_E_ARG
        refused_as_before()
        e.set_query_eot(2)
        for bad in (33, -2):                                                      # ... or on
            assert e._L.fb_set_query_eot(e._h, bad) == FB_E_ARG
        e.set_eot(2)
        for fn in calls.values():
            fn()                                                                  # quorum 2 of r' = 2: runs
        e.set_eot(1)
        for fn in calls.values():
            assert _code(fn)[0] == FB_E_ARG                                       # quorum 2 of r' = 1: no row can reach it
        e.set_query_eot(None)
        unchanged()
        with _voted(e, 3, 2):                                                     # quorum 3 of r' = 2, before anything runs
            before = e.stats()
            for fn in calls.values():
                assert _code(fn)[0] == FB_E_ARG
            assert e.stats()["scored_utts"] == before["scored_utts"]
        with _voted(e, 3, 1, comp):                                               # ... with companions: r' = 2 as well
            for fn in calls.values():
                assert _code(fn)[0] == FB_E_ARG
        unchanged()
        with _voted(e, "majority", 2):                                            # the threshold sweep stays out
            p = nes_params(task, "untargeted", seed=5, stream=1)
            assert _code(lambda: e.estimate_threshold(p, 0.0, audio))[0] == FB_E_STATE
        with _voted(e, "majority", 1, [comp[0][:-1]]):                            # companions of another length than the audio
            for fn in calls.values():
                assert _code(fn)[0] == FB_E_ARG
        with _voted(e, "majority"):                                               # on with r' = 1: nothing differs
            unchanged()
        with _voted(e, 1):
            unchanged()
        unchanged()
    finally:
        e.close()


# ------------------------------------------------------------------------------------- 8. the driver
def test_attack_main_takes_query_eot(small_system, tmp_path, capsys):
    for flags in (["--eot-size", "2"], ["--companions", "1"]):
        with pytest.raises(SystemExit):
            AM.main(["-spk_id", "a", "-task", "CSI", "-type", "untargeted", "--attack", "kenansville"] + flags)
        assert "--attack kenansville does not" in capsys.readouterr().err
    DS.make_site(str(tmp_path))
    names = list(DS.SPK_IDS)
    built = []

    def factory(archi, task, model_list, pre, th, gid):
        from fakebob_amd.systems import gmm_CSI
        _ubm, ml, d = TK._models(small_system, tmp_path, names)
        built.append(gmm_CSI(gid, ml, pre_model_dir=d, input_transform="at:20"))
        return built[-1]
    old = os.getcwd()
    os.chdir(str(tmp_path))
    out = io.StringIO()
    try:
        with contextlib.redirect_stdout(out):
            g, results, _thr = AM.main(["-spk_id"] + names + ["-task", "CSI", "-type", "untargeted", "--streams", "1", "--seed", "5",
                                       "--attack", "kenansville", "--kv-grid", "4", "--kv-window", "64", "--eot-size", "2",
                                       "--query-eot"], model_factory=factory)
    finally:
        os.chdir(old)
        for m in built:
            m.engine.close()
    text = out.getvalue()
    print(text)
    assert g[1] == len(results) >= 1 and all(f in (1, -1) for f in results.values())
    assert text.count("kenansville ") == g[1] and "votes of" in text
    assert g[3] % 2 == 0                                                          # every row was scored twice
