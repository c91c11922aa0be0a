"""The decision-only attack on the device (fb_attack_kenansville; the "decision-only attack" section of include/fakebob_hip.h):
the two kernels against the plain-integer restatement (tests/kenansville_ref.py) bit for bit through the hooks, whole attacks
replayed from the decisions they returned, a candidate that is silent, defended victims, the refusals, and Kenansville and the
driver on top.

Bit-exact checks use np.array_equal.  The one tolerance is the suite's bound between a row of an NES batch and a scoring call
of the same samples: SCORE_TOL of tests/test_gpu_input_transform.py."""
import contextlib
import io
import os
import pickle

import numpy as np
import pytest

from fakebob_amd import attack_main as AM
from fakebob_amd import companions as CP
from fakebob_amd import kenansville as KV
from fakebob_amd._native import FB_E_ARG, FB_E_STATE, NativeError
from fakebob_amd.engine import Engine, kv_params, nes_params, pso_params
from fakebob_amd.models import synthetic_audio, synthetic_ivector_system
from fakebob_amd.systems import gmm_CSI, gmm_OSI, iv_SV
from tests import kenansville_ref as R
from tests.golden import driver_site as DS
from tests.test_gpu_input_transform import SCORE_TOL   # the bound between an NES batch's row and a scoring call

pytestmark = pytest.mark.gpu
WINDOWS = [8, 9, 33, 100, 127, 128]
FACTORS = [0, 1, 64, 6554, 65535, 65536]
N = 4000                                               # the utterance length of tests/test_gpu_pso.py
W0 = 100


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, what
    assert np.array_equal(got, want), (what, int(np.flatnonzero((got != want).ravel())[0]))


# ------------------------------------------------------------------------------------- 1. the kernels, bit for bit
@pytest.mark.parametrize("W", WINDOWS)
def test_hooks_at_every_length(eng, W):
    tab = R.tables(W)
    for n in (1, W - 1, W, W + 1, 3 * W + 5, 4099):
        x = R.edge_audio(W, n)
        wins, ans = R.analyse(x, W, tab)
        a, b, cum, E = eng.debug_kv_analyse(x, W)
        assert a.dtype == np.int32 and cum.dtype == np.int64 and E.dtype == np.int64
        _same(a, [an["a"] for an in ans], ("a", W, n))
        _same(b, [an["b"] for an in ans], ("b", W, n))
        _same(cum, [an["cum"] for an in ans], ("cum", W, n))
        _same(E, [an["E"] for an in ans], ("E", W, n))
        y = eng.debug_kv_candidates(x, W, FACTORS)
        assert y.dtype == np.int16 and y.shape == (len(FACTORS), n)
        for j, q in enumerate(FACTORS):
            _same(y[j], R.candidate(n, W, wins, ans, q, tab), ("y", W, n, q))
        _same(y[0], x, ("q = 0 returns x", W, n))


@pytest.mark.parametrize("rows", [1, 2, 15, 64])
@pytest.mark.parametrize("W", [33, 128])
def test_hooks_at_every_row_count(eng, W, rows):
    n = 3 * W + 5
    x = R.edge_audio(W, n)
    qs = [65536] if rows == 1 else [int(v) for v in np.linspace(0, 65536, rows)]
    y = eng.debug_kv_candidates(x, W, qs)
    _same(y, R.candidates(x, W, qs), ("y", W, rows))
    _same(y, np.stack([KV.remove(x, W, q) for q in qs]), ("the host twin", W, rows))


def test_the_worst_inputs_are_exact(eng):
    """|A| = 2^52 is attained by a constant -32768 window at W = 128; full scale with alternating signs"""
    W = 128
    t = np.arange(3 * W)
    for x in (np.full(3 * W, -32768, np.int16), np.where(t % 2 == 0, -32768, 32767).astype(np.int16)):
        _wins, ans = R.analyse(x, W)
        a, b, cum, E = eng.debug_kv_analyse(x, W)
        _same(a, [an["a"] for an in ans], "a")
        _same(b, [an["b"] for an in ans], "b")
        _same(cum, [an["cum"] for an in ans], "cum")
        _same(E, [an["E"] for an in ans], "E")
        _same(eng.debug_kv_candidates(x, W, [65536, 32768, 1]), R.candidates(x, W, [65536, 32768, 1]), "y")


def test_hooks_refuse_what_the_attack_refuses(eng):
    x = np.zeros(64, np.int16)
    bad_tab = KV.tables(16).copy()
    bad_tab[0, 0] -= 1
    for fn in (lambda: eng.debug_kv_analyse(x, 7), lambda: eng.debug_kv_analyse(x, 129),
               lambda: eng.debug_kv_analyse(x, 16, bad_tab), lambda: eng.debug_kv_candidates(x, 16, [1], bad_tab),
               lambda: eng.debug_kv_candidates(x, 16, [-1]), lambda: eng.debug_kv_candidates(x, 16, [65537]),
               lambda: eng.debug_kv_candidates(x, 16, list(range(65))), lambda: eng.debug_kv_candidates(x, 16, [])):
        with pytest.raises(NativeError) as ex:
            fn()
        assert ex.value.code == FB_E_ARG


# ------------------------------------------------------------------------------------- 2. whole attacks
def _models(small_system, d, names=None):
    ubm, spk = small_system
    names = names or ["spk%d" % i for i in range(len(spk))]
    return ubm, [[names[i], "utt%d" % i, g, -80.0 + 5.0 * i, 3.0 + 0.5 * i] for i, g in enumerate(spk)], str(d)


def _system(case, small_system, d, **kw):
    if case == "gmm OSI":
        ubm, ml, d = _models(small_system, d)
        return gmm_OSI(d + "/osi", ml, ubm, pre_model_dir=d, threshold=0.0, **kw)
    if case == "gmm CSI":
        _ubm, ml, d = _models(small_system, d)
        return gmm_CSI(d + "/csi", ml, pre_model_dir=d, **kw)
    sy = synthetic_ivector_system(C=96, D=72, R=48, L=24, n_speakers=1, seed=11)
    return iv_SV(str(d) + "/sv", ["spk0", "utt0", sy.enrolled[0].copy(), -40.0, 10.0], pre_model_dir=str(d), threshold=0.0,
                 system=sy, **kw)


def _scores(e, rows):
    """ordinary scoring calls of int16 rows -> (system scores (B, S), tv)"""
    raw, tv = e.score_raw([np.ascontiguousarray(r, np.int16) for r in rows])
    return e.system_scores(raw), tv


def _scores_tolerant(e, rows):
    """... of rows some of which may have no voiced frames (the scoring call refuses such a batch): one call per row"""
    out = []
    for r in rows:
        try:
            out.append(_scores(e, [r])[0][0])
        except NativeError:
            out.append(None)
    return out


def _goal(e, task, x):
    """a threshold under which the clean audio is accepted, and its clean decision: the `true` of an evasion attack"""
    sc = _scores(e, [x])[0][0]
    if task == "CSI":
        return 0.0, R.decide("CSI", sc, 0.0)
    thr = float(sc.max()) - 0.25 * max(abs(float(sc.max())), 1.0)
    return thr, R.decide(task, sc, thr)


def _replay(res, task, at, label, thr, G, q_max, max_rounds):
    """the returned decisions drive the restatement's search; every round's candidates must be the returned ones"""
    def ok(r, qs):
        rows = int(res["trace"][r, 2])
        assert rows == len(qs) and res["qs"][r, :rows].tolist() == qs and np.all(res["qs"][r, rows:] == -1)
        return [R.succeeds(int(d), at, label) for d in res["decisions"][r, :rows]]
    want = R.search(ok, G, q_max, max_rounds)
    assert len(want["rounds"]) == res["trace"].shape[0]
    for r, rd in enumerate(want["rounds"]):
        assert res["trace"][r].tolist() == [rd["lo"], -1 if rd["hi"] is None else rd["hi"], rd["rows"]]
        for j in range(rd["rows"]):                                           # the make_decisions rule on the returned scores
            d = int(res["decisions"][r, j])
            assert d == -2 or d == R.decide(task, res["scores"][r, j], thr)
    assert (res["success"], res["factor"], res["n_queries"]) == (want["success"], want["factor"], want["n_queries"])
    return want


# The settings come from a scan of the three systems' decisions over q (ordinary scoring calls of the host twin's candidates):
#  - gmm CSI, synthetic_audio(5): the decision is 2 up to q = 32768 and 0 from 49152 on -- an evasion the grid of 15 finds;
#  - gmm OSI, synthetic_audio(9): the accepted speaker's score falls below a threshold a quarter under it at q near 1100;
#  - i-vector SV, synthetic_audio(9): NOT monotone -- with the threshold 0.25 under the clean score 0.567 the voice is rejected
#    at q = 1000 (-0.070), accepted at 4369 (0.378), rejected at 8738 (0.314) and accepted from 16384 on; q_max = 8738 starts
#    the bisection on a success, and the invariant "lo failed, hi succeeded" has to hold without monotonicity.
# The margins are three orders above SCORE_TOL.
CASES = {"gmm CSI": (15, 5, 65536), "gmm OSI": (4, 9, 65536), "ivector SV": (1, 9, 8738)}


@pytest.mark.parametrize("case", sorted(CASES))
def test_a_whole_attack_is_its_replay(small_system, tmp_path, case):
    task = case.split()[1]
    G, audio_seed, q_max = CASES[case]
    model = _system(case, small_system, tmp_path)
    e = model.engine
    try:
        audio = synthetic_audio(audio_seed, N)
        x = CP.cast_i16(audio, 16)
        thr, true = _goal(e, task, x)
        assert true != -1                                                     # an enrolled speaker, accepted
        p = nes_params(task, "untargeted", threshold=thr, true=true, seed=5, stream=1)
        before = e.stats()
        res = e.attack_kenansville(p, kv_params(W0, G, q_max, 32), audio)
        after = e.stats()
        n = res["trace"].shape[0]
        print("%s, G = %d: %d rounds, %d queries, success %d, factor %d; lo/hi/rows %s" % (
            case, G, n, res["n_queries"], res["success"], res["factor"], res["trace"].tolist()))
        assert after["scored_utts"] - before["scored_utts"] == res["n_queries"] and after["nes_iters"] == before["nes_iters"]
        secs = e.attack_iter_seconds(n)
        assert secs.shape == (n,) and np.all(secs > 0)
        _replay(res, task, "untargeted", true, thr, G, q_max, 32)
        assert res["success"] == 1 and n > 1 and 1 <= res["factor"] <= q_max  # (see CASES)
        if G == 1:
            assert n <= 17 and np.all(res["trace"][:, 2] == 1)
        want_adv = R.remove(x, W0, res["factor"]) if res["success"] == 1 else x
        _same(res["adv"], want_adv, "adv")
        if res["success"] == 1:
            rr, jj = [(r, j) for r in range(n) for j in range(int(res["trace"][r, 2])) if res["qs"][r, j] == res["factor"]][0]
            sc, tv = _scores(e, [res["adv"]])
            err = np.abs(sc[0] - res["scores"][rr, jj]).max()
            print("  the winning row against a scoring call of adv: %.3g (bound %.3g)" % (err, SCORE_TOL))
            assert tv[0] > 0 and err <= SCORE_TOL
    finally:
        e.close()


def test_a_targeted_attack_replays_too(small_system, tmp_path):
    model = _system("gmm CSI", small_system, tmp_path)
    e = model.engine
    try:
        audio = synthetic_audio(5, N)                                         # decided 2 when clean, 0 from q near 40000 on
        x = CP.cast_i16(audio, 16)
        assert R.decide("CSI", _scores(e, [x])[0][0], 0.0) == 2
        p = nes_params("CSI", "targeted", target=0, seed=5, stream=1)
        res = e.attack_kenansville(p, kv_params(W0, 6, 65536, 3), audio)      # round 0's last row is silent; max_rounds stops it
        print("targeted CSI: success %d, factor %d, %s" % (res["success"], res["factor"], res["trace"].tolist()))
        _replay(res, "CSI", "targeted", 0, 0.0, 6, 65536, 3)
        assert res["decisions"][0, 5] == -2 and res["success"] == 1 and res["trace"].shape[0] == 3
        _same(res["adv"], R.remove(x, W0, res["factor"]), "adv")
        assert R.decide("CSI", _scores(e, [res["adv"]])[0][0], 0.0) == 0
    finally:
        e.close()


# ------------------------------------------------------------------------------------- 3. a silent candidate
def test_a_silent_candidate_is_no_decision_and_no_error(small_system, tmp_path):
    model = _system("gmm CSI", small_system, tmp_path)
    e = model.engine
    try:
        audio = synthetic_audio(9, N)
        x = CP.cast_i16(audio, 16)
        assert not KV.remove(x, W0, 65536).any()                              # q = 65536 removes everything
        true = R.decide("CSI", _scores(e, [x])[0][0], 0.0)
        p = nes_params("CSI", "untargeted", true=true, seed=5, stream=1)
        res = e.attack_kenansville(p, kv_params(W0, 4, 65536, 1), audio)      # FB_OK
        assert res["qs"][0].tolist() == [16384, 32768, 49152, 65536] and res["n_queries"] == 4
        assert res["decisions"][0, 3] == -2
        rows = R.candidates(x, W0, [16384, 32768, 49152])
        sc, tv = _scores(e, rows)
        err = np.abs(sc - res["scores"][0, :3]).max()
        print("  three rows next to a silent one against scoring calls: %.3g (bound %.3g)" % (err, SCORE_TOL))
        assert np.all(tv > 0) and err <= SCORE_TOL
        assert [int(d) for d in res["decisions"][0, :3]] == [R.decide("CSI", s, 0.0) for s in res["scores"][0, :3]]
        # targeted at the silent row's "decision": never a success
        for target in range(3):
            r2 = e.attack_kenansville(nes_params("CSI", "targeted", target=target, seed=5, stream=1), kv_params(W0, 1, 65536, 1), audio)
            assert r2["decisions"][0, 0] == -2 and (r2["success"], r2["factor"]) == (-1, -1)
            _same(r2["adv"], x, "adv of a failed attack is x")
    finally:
        e.close()


# ------------------------------------------------------------------------------------- 4. defended victims
def test_row_scores_of_a_defended_victim_match_scoring_calls(small_system, tmp_path):
    model = _system("gmm CSI", small_system, tmp_path, input_transform="ms:7,qt:512", codec="ulaw")
    e = model.engine
    try:
        audio = synthetic_audio(9, N)
        x = CP.cast_i16(audio, 16)
        true = R.decide("CSI", _scores(e, [x])[0][0], 0.0)
        res = e.attack_kenansville(nes_params("CSI", "untargeted", true=true, seed=5, stream=1), kv_params(W0, 5, 40000, 2), audio)
        _replay(res, "CSI", "untargeted", true, 0.0, 5, 40000, 2)
        worst = 0.0
        for r in range(res["trace"].shape[0]):
            rows = int(res["trace"][r, 2])
            want = _scores_tolerant(e, R.candidates(x, W0, res["qs"][r, :rows].tolist()))
            for j in range(rows):
                if want[j] is None:
                    assert res["decisions"][r, j] == -2
                else:
                    worst = max(worst, float(np.abs(want[j] - res["scores"][r, j]).max()))
        print("  defended rows against scoring calls under the same defence: %.3g (bound %.3g)" % (worst, SCORE_TOL))
        assert worst <= SCORE_TOL
        plain = _system("gmm CSI", small_system, tmp_path)
        try:
            r0 = plain.engine.attack_kenansville(nes_params("CSI", "untargeted", true=true, seed=5, stream=1),
                                                 kv_params(W0, 5, 40000, 1), audio)
        finally:
            plain.engine.close()
        assert not np.array_equal(r0["scores"][0], res["scores"][0])          # the defence does act on the candidates
    finally:
        e.close()


def _noisy(small_system, d, stream):
    model = _system("gmm CSI", small_system, d, input_transform="noise:30")
    try:
        p = nes_params("CSI", "untargeted", true=0, seed=5, stream=stream)
        return model.engine.attack_kenansville(p, kv_params(W0, 4, 30000, 3), synthetic_audio(9, N))
    finally:
        model.engine.close()


def test_an_attack_on_a_randomised_victim_depends_on_seed_and_stream_only(small_system, tmp_path):
    a, b, c = _noisy(small_system, tmp_path, 2), _noisy(small_system, tmp_path, 2), _noisy(small_system, tmp_path, 3)
    assert sorted(a) == sorted(b)
    for key in a:                                                             # (unused places of `scores` hold NaN)
        assert np.array_equal(a[key], b[key], equal_nan=(key == "scores")), key
    assert not np.array_equal(a["scores"][0], c["scores"][0])                 # another stream: other draws
    rows = int(a["trace"][0, 2])
    assert np.all(np.isfinite(a["scores"][0, :rows]))


# ------------------------------------------------------------------------------------- 5. refusals
def _code(fn):
    with pytest.raises(NativeError) as ex:
        fn()
    return ex.value.code


def test_refusals_leave_the_engine_usable(small_system, tmp_path):
    audio = synthetic_audio(9, N)
    x = CP.cast_i16(audio, 16)
    bare = Engine(0)
    try:
        assert _code(lambda: bare.attack_kenansville(nes_params("OSI", "untargeted", true=0), kv_params(), audio)) == FB_E_STATE
    finally:
        bare.close()
    for case, labels_bad, labels_ok in (("gmm OSI", [-2, 3], [-1, 0, 2]), ("gmm CSI", [-1, 3], [0, 2]), ("ivector SV", [0, 2, -2], [1, -1])):
        task = case.split()[1]
        model = _system(case, small_system, tmp_path)
        e = model.engine
        try:
            pso = nes_params(task, "targeted", epsilon=0.002, max_iter=2, target=0 if task != "SV" else 0, threshold=1e3, seed=5, stream=1)
            swarm = pso_params(particles=4, v_max=0.002)
            want_pso = e.attack_pso(pso, swarm, audio)
            want_sc = e.score_raw([x])

            def unchanged():
                got = e.attack_pso(pso, swarm, audio)
                sc = e.score_raw([x])
                return (got[1] == want_pso[1] and all(np.array_equal(g, w) for g, w in zip((got[0],) + got[2:], (want_pso[0],) + want_pso[2:]))
                        and np.array_equal(sc[0], want_sc[0]) and np.array_equal(sc[1], want_sc[1]))
            run = lambda pk, kk, tab=None: e.attack_kenansville(                # noqa: E731
                nes_params(task, **dict(dict(attack_type="untargeted", true=labels_ok[0], seed=5, stream=1), **pk)),
                kv_params(**dict(dict(window=W0, grid=3, q_max=20000, max_rounds=1), **kk)), audio, tab)
            ok = run({}, {})
            bad = [({}, dict(window=7)), ({}, dict(window=129)), ({}, dict(window=0)), ({}, dict(grid=0)), ({}, dict(grid=65)),
                   ({}, dict(q_max=0)), ({}, dict(q_max=65537)), ({}, dict(max_rounds=0)), ({}, dict(max_rounds=33)),
                   (dict(bits_per_sample=1), {}), (dict(bits_per_sample=17), {})]
            bad += [(dict(true=v), {}) for v in labels_bad] + [(dict(attack_type="targeted", target=v), {}) for v in labels_bad]
            for pk, kk in bad:
                assert _code(lambda: run(pk, kk)) == FB_E_ARG, (case, pk, kk)
            assert unchanged(), case
            for v in labels_ok:                                                # every decision value is a label
                run(dict(true=v), {})
                run(dict(attack_type="targeted", target=v), {})
            other = "CSI" if task != "CSI" else "OSI"
            assert _code(lambda: e.attack_kenansville(nes_params(other, "untargeted", true=0), kv_params(W0, 3, 20000, 1), audio)) == FB_E_ARG
            # wrong tables: another window's, and each of the four checked entries
            assert _code(lambda: run({}, {}, np.zeros((4, W0), np.int32))) == FB_E_ARG
            for row in range(4):
                t = KV.tables(W0).copy()
                t[row, 0] += 1
                assert _code(lambda: run({}, {}, t)) == FB_E_ARG, row
            assert unchanged(), case
            # adver_thresh and the NES-only fields are not read
            nan = float("nan")
            junk = dict(adver_thresh=nan, epsilon=nan, max_iter=-1, samples_per_draw=-7, sigma=-1.0, max_lr=nan, min_lr=nan, momentum=nan,
                        plateau_length=-3, plateau_drop=0.0)
            got = run(junk, {})
            assert all(np.array_equal(got[k], ok[k], equal_nan=True) if k == "scores" else np.array_equal(got[k], ok[k]) for k in ok)
            e.set_eot(2)
            assert _code(lambda: run({}, {})) == FB_E_STATE
            e.set_eot(1)
            assert unchanged(), case
            e.set_companions([CP.cast_i16(synthetic_audio(3, N), 16)])
            assert _code(lambda: run({}, {})) == FB_E_STATE
            e.set_companions(None)
            assert unchanged(), case
        finally:
            e.close()


# ------------------------------------------------------------------------------------- 6. Kenansville and the driver
def test_kenansville_on_top(small_system, tmp_path):
    model = _system("gmm CSI", small_system, tmp_path)
    e = model.engine
    try:
        audio = synthetic_audio(5, N)                                         # (CASES: an evasion the grid finds)
        x = CP.cast_i16(audio, 16)
        true = int(model.make_decisions(audio)[0])
        kv = KV.Kenansville("CSI", "untargeted", model, window=W0, grid=6, seed=5, verbose=False)
        kv._stream = 1
        cp = str(tmp_path / "kv.cp")
        adv, flag = kv.attack(audio, cp, true=true)
        assert adv.dtype == np.int16 and adv.shape == (N, 1) and flag == 1 and kv._stream == 2
        assert int(model.make_decisions(adv)[0]) != true                      # the speaker is no longer recognised
        direct = e.attack_kenansville(nes_params("CSI", "untargeted", true=true, seed=5, stream=1), kv_params(W0, 6, 65536, 32), audio)
        assert np.array_equal(adv[:, 0], direct["adv"]) and flag == direct["success"]
        assert kv.n_queries == direct["n_queries"] and kv.factor == (direct["factor"] if flag == 1 else None)
        _same(adv[:, 0], R.remove(x, W0, kv.factor), "adv")
        with open(cp, "rb") as r:
            rows = pickle.load(r)
        assert len(rows) == direct["trace"].shape[0]                           # one row per round
        for k, row in enumerate(rows):
            n = int(direct["trace"][k, 2])
            assert len(row) == 6 and np.array_equal(row[0], direct["qs"][k, :n]) and np.array_equal(row[1], direct["decisions"][k, :n])
            assert row[2].shape == (n, 3) and row[3:5] == direct["trace"][k, :2].tolist() and row[5] > 0
    finally:
        e.close()


def test_attack_main_runs_kenansville_on_the_driver_site(small_system, tmp_path):
    """the driver site's voices (tests/golden/driver_site.py), a real CSI system: the voices the system assigns to their own
    speaker are attacked, each attack is Kenansville's"""
    DS.make_site(str(tmp_path))
    from scipy.io.wavfile import read
    voices = [(spk, name, read(os.path.join(str(tmp_path), "data", sub, spk, name))[1]) for sub, spk, name, _c in DS.VOICES
              if sub == "test-set"]
    probe = _system("gmm CSI", small_system, tmp_path)
    try:
        dec = [R.decide("CSI", _scores(probe.engine, [v[2]])[0][0], 0.0) for v in voices]
    finally:
        probe.engine.close()
    # the speakers' names go to the models so that some voice is its own speaker's: the (model, name) pair with most voices
    best = max(((sum(1 for v, d in zip(voices, dec) if d == j and v[0] == s), j, s) for j in range(3) for s in DS.SPK_IDS))
    names = [None] * 3
    names[best[1]] = best[2]
    rest = [s for s in DS.SPK_IDS if s != best[2]]
    names = [s if s is not None else rest.pop(0) for s in names]
    expect = sum(1 for v, d in zip(voices, dec) if names[d] == v[0])
    assert expect >= 1
    built = []

    def factory(archi, task, model_list, pre, th, gid):
        _ubm, ml, d = _models(small_system, tmp_path, names)
        built.append(gmm_CSI(gid, ml, pre_model_dir=d))
        return built[-1]
    old = os.getcwd()
    os.chdir(str(tmp_path))
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            g, results, _thr = AM.main(["-spk_id"] + names + ["-task", "CSI", "-type", "untargeted", "--streams", "1", "--seed", "5",
                                       "--attack", "kenansville", "--kv-grid", "4", "--kv-window", "64"], model_factory=factory)
    finally:
        os.chdir(old)
        for m in built:
            m.engine.close()
    print("driver: %d attacks, %d succeeded, %d utterances scored" % (g[1], g[0], g[3]))
    assert g[1] == len(results) == expect and all(f in (1, -1) for f in results.values())
    wavs = [os.path.join(dp, f) for dp, _dn, fn in os.walk(os.path.join(str(tmp_path), "adversarial-audio")) for f in fn]
    cps = [os.path.join(dp, f) for dp, _dn, fn in os.walk(os.path.join(str(tmp_path), "checkpoint")) for f in fn]
    assert len(wavs) == len(cps) == expect
    with open(cps[0], "rb") as r:
        rows = pickle.load(r)
    assert len(rows) >= 1 and len(rows[0]) == 6 and len(rows[0][0]) <= 4
