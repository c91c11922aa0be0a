"""HopSkipJump on the device (fb_attack_hsj; the "decision-only attack II" section of include/fakebob_hip.h): the kernels
against the numpy restatement (tests/hsj_ref.py) bit for bit through the hooks, whole attacks replayed from the decision logs
they returned, defended victims, a stall, the query cap, the refusals, and HopSkipJump on top.

Bit-exact checks use np.array_equal.  The one tolerance is the suite's bound between a row of an NES batch and a scoring call
of the same samples (SCORE_TOL of tests/test_gpu_input_transform.py): the returned audio stands ON the decision boundary, so
where a scoring call of it decides otherwise than the batch did, the score must lie within that bound of the boundary."""
import math
import pickle

import numpy as np
import pytest

from fakebob_amd import companions as CP
from fakebob_amd import hsj as H
from fakebob_amd._native import FB_E_ARG, FB_E_STATE, NativeError
from fakebob_amd.engine import Engine, hsj_params, nes_params
from fakebob_amd.models import synthetic_audio, synthetic_ivector_system
from fakebob_amd.systems import gmm_CSI, gmm_OSI, gmm_SV, iv_SV
from tests import hsj_ref as R
from tests.kenansville_ref import decide
from tests.test_gpu_input_transform import SCORE_TOL   # the bound between an NES batch's row and a scoring call

pytestmark = pytest.mark.gpu
LENGTHS = [1, 2, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, 4099]
ROWS = [1, 2, 63, 64, 65]
SEEDS = [(0x9E3779B97F4A7C15, 3), (0xFFFFFFFF00000001, 0xFFFFFFFE), (5, 1)]   # (seed, stream): high bits set, stream != 0
N = 4000                                               # the utterance length of tests/test_gpu_pso.py
VOICES = [synthetic_audio(u, N) for u in (0, 3, 5, 9, 1, 7)]


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, what
    assert np.array_equal(got, want), (what, int(np.flatnonzero((got != want).ravel())[0]))


def _rail_audio(n, seed):
    """float64 audio in [-1, 1] whose samples cycle through +-1.0, values an ulp and an int16 step inside the rails, zeros and
    ordinary values: both clips act on what is added to it"""
    rs = np.random.RandomState(seed)
    x = rs.uniform(-0.9, 0.9, n)
    special = [1.0, -1.0, np.nextafter(1.0, 0.0), np.nextafter(-1.0, 0.0), 1.0 - 2.0 ** -15, -1.0 + 2.0 ** -15, 0.0, -0.0]
    for i in range(0, n, 3):
        x[i] = special[(i // 3) % len(special)]
    return x


def _noise(oracle, seed, t, stream, n, B):
    return oracle.noise((seed ^ R.KEY) & 0xFFFFFFFFFFFFFFFF, t, stream, n, B)


# ------------------------------------------------------------------------------------- 1. the kernels, bit for bit
@pytest.mark.parametrize("n", LENGTHS)
def test_line_and_adopt_hooks(eng, n):
    a, y = _rail_audio(n, 11 + n), _rail_audio(n, 12 + n)[::-1].copy()
    for bits, qs in ((16, [0, 1, R.Q // 3, R.Q - 1, R.Q]), (8, [R.Q // 2]), (16, [((j + 1) * R.Q) // 64 for j in range(64)])):
        rows, x, D2 = eng.debug_hsj_line(a, y, qs, bits)
        _same(rows, np.stack([R.cast_i16(R.line(a, y, q), bits) for q in qs]), ("rows", n, bits))
        _same(x, R.line(a, y, qs[0]), ("x", n))
        assert D2 == R.ssq(R.line(a, y, qs[0]) - a), ("D2", n)
    rows, x, D2 = eng.debug_hsj_line(a, y, [0])
    _same(x, a, "line(y, 0) is a")
    assert D2 == 0.0


@pytest.mark.parametrize("n", LENGTHS)
def test_probes_and_direction_hooks(eng, oracle, n):
    x = _rail_audio(n, 21 + n)
    rs = np.random.RandomState(n)
    for k, B in enumerate(ROWS + ([1024] if n == 257 else [])):
        seed, stream = SEEDS[k % len(SEEDS)]
        t, bits, sigma = 1 + k, (8 if k == 1 else 16), [2.0 ** -15, 0.013, 0.4][k % 3]
        z = _noise(oracle, seed, t, stream, n, B)
        _same(eng.debug_hsj_probes(x, sigma, seed, stream, t, B, bits), R.probes(x, sigma, z, bits), ("probes", n, B))
        for w in (rs.randint(-2 * B, 2 * B + 1, B), R.weights(rs.rand(B) < 0.4)[0], np.zeros(B, np.int32)):
            v, S = eng.debug_hsj_dir(w, seed, stream, t, n)
            want_v, want_S = R.direction(w, z)
            _same(v, want_v, ("v", n, B))
            assert S == want_S, ("S", n, B)
        assert S == 0.0 and not v.any()                                        # all weights zero


def test_both_key_words_and_every_counter_word_matter(eng, oracle):
    n, B, x = 257, 3, _rail_audio(257, 5)
    base = eng.debug_hsj_probes(x, 0.01, 0x1234567800000009, 2, 1, B)
    for seed, stream, t in ((0x1234567800000008, 2, 1), (0x1234567900000009, 2, 1), (0x1234567800000009, 3, 1),
                            (0x1234567800000009, 2, 2)):
        other = eng.debug_hsj_probes(x, 0.01, seed, stream, t, B)
        assert not np.array_equal(other, base), (hex(seed), stream, t)
        _same(other, R.probes(x, 0.01, _noise(oracle, seed, t, stream, n, B)), "probes")
    assert not np.array_equal(base[0], base[1])                                 # the row index is a counter word
    # the probes' normals are not the NES batch's of the same seed
    assert not np.array_equal(base, R.probes(x, 0.01, oracle.noise(0x1234567800000009, 1, 2, n, B)))


@pytest.mark.parametrize("G", [1, 15, 64])
def test_step_hook(eng, G):
    for n in LENGTHS:
        x = _rail_audio(n, 31 + n)
        v = np.random.RandomState(n + G).normal(0.0, 3.0, n)
        for bits, S, xi in ((16, R.ssq(v), 2.5), (8, R.ssq(v), 1e-3), (16, 0.0, 2.5), (16, 7.0, 0.0)):
            rows, y = eng.debug_hsj_step(x, v, S, xi, G, bits)
            want = [R.step(x, v, S, xi, m) for m in range(G)]
            _same(y, np.stack(want), ("y", n, G, S, xi))
            _same(rows, np.stack([R.cast_i16(w, bits) for w in want]), ("rows", n, G, S, xi))
        _same(y, np.stack([R.clip1(x)] * G), "xi = 0 leaves x")


def test_hooks_refuse_bad_arguments(eng):
    a = np.zeros(8)
    for fn in (lambda: eng.debug_hsj_line(a, a, []), lambda: eng.debug_hsj_line(a, a, list(range(65))),
               lambda: eng.debug_hsj_line(a, a, [-1]), lambda: eng.debug_hsj_line(a, a, [R.Q + 1]),
               lambda: eng.debug_hsj_line(a, a, [1], 17), lambda: eng.debug_hsj_probes(a, 0.1, 1, 0, 1, 0),
               lambda: eng.debug_hsj_probes(a, 0.1, 1, 0, 1, 1025), lambda: eng.debug_hsj_dir(np.zeros(0, np.int32), 1, 0, 1, 8),
               lambda: eng.debug_hsj_dir(np.zeros(1025, np.int32), 1, 0, 1, 8), lambda: eng.debug_hsj_dir([4096], 1, 0, 1, 8),
               lambda: eng.debug_hsj_step(a, a, 1.0, 1.0, 0), lambda: eng.debug_hsj_step(a, a, 1.0, 1.0, 65)):
        with pytest.raises(NativeError) as ex:
            fn()
        assert ex.value.code == FB_E_ARG


# ------------------------------------------------------------------------------------- 2. whole attacks
def _models(small_system, d):
    ubm, spk = small_system
    return ubm, [["spk%d" % i, "utt%d" % i, g, -80.0 + 5.0 * i, 3.0 + 0.5 * i] for i, g in enumerate(spk)], str(d)


_csi_norm = {}


def _csi_models(small_system, d):
    """the CSI system's z-norm: every speaker's mean is its mean raw score over VOICES (deviation 1), so that the decision is
    the speaker a voice scores best on RELATIVE to the other voices -- with the stock constants one speaker takes them all,
    and a targeted attack needs a start that is decided otherwise than the attacked voice"""
    _ubm, ml, d = _models(small_system, d)
    if "zm" not in _csi_norm:
        probe = gmm_CSI(d + "/csi_probe", ml, pre_model_dir=d)
        try:
            raw, _tv = probe.engine.score_raw([CP.cast_i16(v, 16) for v in VOICES])
        finally:
            probe.engine.close()
        _csi_norm["zm"] = [float(v) for v in raw.mean(axis=0)]
    return [[m[0], m[1], m[2], _csi_norm["zm"][i], 1.0] for i, m in enumerate(ml)]


def _system(case, small_system, d, **kw):
    ubm, ml, d = _models(small_system, d)
    if case == "gmm CSI":
        return gmm_CSI(d + "/csi", _csi_models(small_system, d), pre_model_dir=d, **kw)
    if case == "gmm OSI":
        return gmm_OSI(d + "/osi", ml, ubm, pre_model_dir=d, threshold=0.0, **kw)
    if case == "gmm SV":
        return gmm_SV(d + "/gsv", ml[0], ubm, pre_model_dir=d, threshold=0.0, **kw)
    sy = synthetic_ivector_system(C=96, D=72, R=48, L=24, n_speakers=1, seed=11)
    return iv_SV(d + "/sv", ["spk0", "utt0", sy.enrolled[0].copy(), -40.0, 10.0], pre_model_dir=d, threshold=0.0, system=sy, **kw)


def _scores(e, rows):
    """ordinary scoring calls of int16 rows -> system scores (B, S)"""
    raw, _tv = e.score_raw([np.ascontiguousarray(r, np.int16) for r in rows])
    return e.system_scores(raw)




def _setting(e, case):
    """(audio, init, attack type, label, threshold) on the system of `case`, from scoring calls of four synthetic voices.
    CSI: two voices that are decided differently, the second one's decision is the target.  The threshold tasks: the two
    voices whose best scores lie furthest apart, the threshold half way between -- the lower one is rejected and attacked, the
    higher one is accepted and the start (SV: "a rejected voice is accepted"; OSI untargeted: true = -1, rejected)."""
    task = case.split()[1]
    sc = _scores(e, [CP.cast_i16(v, 16) for v in VOICES])
    if task == "CSI":
        d = [decide("CSI", s, 0.0) for s in sc]
        others = [k for k in range(len(d)) if d[k] != d[0]]
        assert others, ("every voice is decided %d" % d[0], sc.tolist())
        top = np.sort(sc, axis=1)
        assert min(top[0, -1] - top[0, -2], top[others[0], -1] - top[others[0], -2]) > 1e3 * SCORE_TOL
        return VOICES[0], VOICES[others[0]], "targeted", d[others[0]], 0.0
    best = sc.max(axis=1)
    lo, hi = int(np.argmin(best)), int(np.argmax(best))
    thr = 0.5 * (float(best[lo]) + float(best[hi]))
    assert best[hi] - best[lo] > 1e3 * SCORE_TOL
    return (VOICES[lo], VOICES[hi], "targeted", 1, thr) if task == "SV" else (VOICES[lo], VOICES[hi], "untargeted", -1, thr)


def _params(at, label, thr, task, **kw):
    key = "target" if at == "targeted" else "true"
    return nes_params(task, at, threshold=thr, seed=kw.pop("seed", 5), stream=kw.pop("stream", 1), max_iter=kw.pop("max_iter", 3),
                      **dict({key: label}, **kw))


def _replay(oracle, res, audio, init, hp, at, label, seed=5, stream=1, max_iter=3, bits=16):
    """the returned decision log drives the restatement: every x_t, D2, trace row and the returned row, bit for bit"""
    want = R.drive(audio, init, hp, at, label, oracle.noise, seed, stream, max_iter, decisions=res["decisions"], bits=bits)
    assert (res["success"], res["n_iters"], res["n_queries"]) == (want["success"], want["n_iters"], want["n_queries"])
    assert res["n_queries"] == len(want["decisions"]) == res["decisions"].size
    _same(res["trace"], want["trace"], "trace")
    assert res["dist2"] == want["dist2"]
    _same(res["adv"], want["adv"], "adv")
    _same(res["adv_f64"], want["x"], "x")
    if "xs" in res:
        assert len(want["xs"]) == res["xs"].shape[0]
        for t, x in enumerate(want["xs"]):
            _same(res["xs"][t], x, ("x_t", t))
    return want


def _rescored_is_adversarial(model, task, adv, at, label, thr):
    """adv through the system class's make_decisions, an ordinary scoring call.  On an undefended victim it is the same int16
    row through the same front end and back end.  It is also, by construction, one step of q from a row that was NOT decided
    adversarial, and the NES-batch path and the scoring-call path agree on a score only to SCORE_TOL: where make_decisions
    decides otherwise, the score must lie that close to the boundary, and only such a row is not held against the attack."""
    e = model.engine
    model.threshold = thr
    d = int(np.asarray(model.make_decisions(adv[:, np.newaxis])[0]).reshape(-1)[0])
    s = _scores(e, [adv])[0]
    assert d == decide(task, s, thr)
    if R.adversarial(d, at, label):
        return
    top = np.sort(s)[::-1]
    margin = abs(float(top[0]) - thr) if task != "CSI" else float(top[0] - top[1])
    if task == "OSI":
        margin = min(margin, float(top[0] - top[1])) if s.size > 1 else margin
    print("  the scoring call decides %d at a margin of %.3g (bound %.3g): such a row is not held against the attack" % (d, margin, SCORE_TOL))
    assert margin <= SCORE_TOL


CASES = ["gmm CSI", "gmm SV", "gmm OSI", "ivector SV"]


@pytest.mark.parametrize("case", CASES)
def test_a_whole_attack_is_its_replay(small_system, oracle, tmp_path, case):
    task = case.split()[1]
    model = _system(case, small_system, tmp_path)
    e = model.engine
    try:
        audio, init, at, label, thr = _setting(e, case)
        hp = dict(R.DEFAULTS)
        before = e.stats()
        res = e.attack_hsj(_params(at, label, thr, task), hsj_params(**hp), audio, init, keep_x=True)
        after = e.stats()
        tr = res["trace"]
        print("%s %s, label %d, threshold %.4g: success %d, %d queries; dist per trace row %s; m %s, hi %s" % (
            case, at, label, thr, res["success"], res["n_queries"], [float("%.4g" % math.sqrt(v)) for v in tr[:, 0]],
            tr[:, 3].astype(int).tolist(), tr[:, 4].astype(int).tolist()))
        assert after["scored_utts"] - before["scored_utts"] == res["n_queries"] and after["nes_iters"] == before["nes_iters"]
        secs = e.attack_iter_seconds(tr.shape[0])
        assert secs.shape == (tr.shape[0],) and np.all(secs > 0)
        want = _replay(oracle, res, audio, init, hp, at, label)
        assert res["success"] == 1 and res["n_iters"] == 3 and tr.shape == (4, 8)
        assert all(R.adversarial(d, at, label) for d in want["adopted"])
        assert res["dist2"] <= tr[0, 0] and np.count_nonzero(tr[1:, 4] < 0) <= 1    # it walks: at most one stall in three
        _rescored_is_adversarial(model, task, res["adv"], at, label, thr)
    finally:
        e.close()


# ------------------------------------------------------------------------------------- 3. defended victims
def _defended(small_system, d, kw, stream, max_iter=2):
    model = _system("gmm CSI", small_system, d, **kw)
    e = model.engine
    try:
        audio, init, at, label, thr = _setting(e, "gmm CSI")
        res = e.attack_hsj(_params(at, label, thr, "CSI", stream=stream, max_iter=max_iter), hsj_params(grid=8, num_evals_init=16),
                           audio, init, keep_x=True)
        return res, (audio, init, at, label)
    finally:
        e.close()


@pytest.mark.parametrize("kw", [dict(input_transform="ms:7,qt:512"), dict(codec="ulaw"), dict(input_transform="noise:40")],
                         ids=["chain", "codec", "noise"])
def test_an_attack_on_a_defended_victim_depends_on_seed_and_stream_only(small_system, oracle, tmp_path, kw):
    a, setting = _defended(small_system, tmp_path, kw, 2)
    b, _ = _defended(small_system, tmp_path, kw, 2)
    assert sorted(a) == sorted(b)
    for key in a:
        assert np.array_equal(a[key], b[key]), key
    assert a["success"] == 1 and a["n_iters"] == 2
    _replay(oracle, a, setting[0], setting[1], dict(R.DEFAULTS, grid=8, num_evals_init=16), setting[2], setting[3], stream=2, max_iter=2)
    plain, _ = _defended(small_system, tmp_path, {}, 2)
    assert not np.array_equal(plain["adv"], a["adv"])                           # the defence does act on the rows' decisions
    if "noise" in str(kw):
        c, _ = _defended(small_system, tmp_path, kw, 3)
        assert not np.array_equal(c["adv"], a["adv"])                           # another stream: other draws


# ------------------------------------------------------------------------------------- 4. a stall, the query cap
def test_a_stall_leaves_the_boundary_point(small_system, oracle, tmp_path):
    """grid = 1, max_rounds = 1: the start search scores `init` itself (q = Q), every step batch is the one full step of
    length |x - a| along the estimated direction and every search the one row q = Q.  The threshold stands 2 % under the
    start's score, so such a step usually leaves the accepted side (here all three do; with another pair of voices the first
    of three was accepted): an iteration that stalls leaves D2, x and the returned row as they were"""
    model = _system("gmm SV", small_system, tmp_path)
    e = model.engine
    try:
        audio, init, at, label, _thr = _setting(e, "gmm SV")
        s = _scores(e, [CP.cast_i16(audio, 16), CP.cast_i16(init, 16)])[:, 0]
        thr = float(s[1] - 0.02 * (s[1] - s[0]))
        hp = dict(R.DEFAULTS, grid=1, max_rounds=1)
        res = e.attack_hsj(_params(at, label, thr, "SV"), hsj_params(**hp), audio, init, keep_x=True)
        print("stall: trace %s" % res["trace"].tolist())
        _replay(oracle, res, audio, init, hp, at, label)
        tr = res["trace"]
        assert res["success"] == 1 and res["n_iters"] == 3 and tr[0, 4] == R.Q and tr[0, 5] == 1
        stalled = [t for t in range(1, 4) if tr[t, 4] < 0]
        assert stalled                                                          # the path is taken
        for t in stalled:
            assert tr[t, 3] == -1 and tr[t, 5] == 0                             # (with one row per search, only the step can stall)
            assert tr[t, 0] == tr[t - 1, 0] and np.array_equal(res["xs"][t], res["xs"][t - 1])
            assert tr[t, 6] == tr[t - 1, 6] + tr[t, 1] + 1                      # its probes and its one step row were scored
        if not any(tr[t, 4] >= 0 for t in range(1, 4)):                         # (the replay above has checked the row otherwise)
            _same(res["adv"], R.cast_i16(R.line(audio, init, R.Q)), "adv is the start's row")
    finally:
        e.close()


def test_max_queries_is_honoured_exactly(small_system, oracle, tmp_path):
    model = _system("gmm CSI", small_system, tmp_path)
    e = model.engine
    try:
        audio, init, at, label, thr = _setting(e, "gmm CSI")
        free = e.attack_hsj(_params(at, label, thr, "CSI", max_iter=2), hsj_params(), audio, init)
        marks = free["trace"][:, 6].astype(int).tolist()                         # rows scored after the start and each iteration
        cut = {}
        for cap in (1, marks[0] - 1, marks[0] + 31, marks[0] + 32, marks[0] + 46, marks[0] + 47, marks[1] - 1, marks[2]):
            hp = dict(R.DEFAULTS, max_queries=cap)
            res = e.attack_hsj(_params(at, label, thr, "CSI", max_iter=2), hsj_params(**hp), audio, init, keep_x=True)
            _replay(oracle, res, audio, init, hp, at, label, max_iter=2)
            assert res["n_queries"] <= max(cap, 15) and res["success"] == 1
            assert np.array_equal(res["decisions"], free["decisions"][:res["n_queries"]])   # the same attack, cut short
            print("cap %d: %d queries, %d iterations" % (cap, res["n_queries"], res["n_iters"]))
            cut[cap] = res["n_queries"]
        # what the cap cuts: the probes (32 rows at t = 1) and the step batch (15) are scored whole or not at all
        assert [cut[marks[0] + k] for k in (31, 32, 46, 47)] == [marks[0], marks[0] + 32, marks[0] + 32, marks[0] + 47]
        assert cut[1] == 15 and cut[marks[2]] == marks[2]                       # round 0 of the start is exempt; a cap that fits
    finally:
        e.close()


# ------------------------------------------------------------------------------------- 5. refusals
def _code(fn):
    with pytest.raises(NativeError) as ex:
        fn()
    return ex.value.code


def test_refusals_leave_the_engine_usable(small_system, tmp_path):
    audio, init = VOICES[0], VOICES[2]
    bare = Engine(0)
    try:
        assert _code(lambda: bare.attack_hsj(nes_params("OSI", "untargeted", true=0, max_iter=1), hsj_params(), audio, init)) == FB_E_STATE
    finally:
        bare.close()
    for case, labels_bad, labels_ok in (("gmm OSI", [-2, 3], [-1, 0, 2]), ("gmm CSI", [-1, 3], [0, 2]), ("ivector SV", [0, 2, -2], [1, -1])):
        task = case.split()[1]
        model = _system(case, small_system, tmp_path)
        e = model.engine
        try:
            run = lambda pk, kk, a=audio, i=init, **extra: e.attack_hsj(        # noqa: E731
                nes_params(task, **dict(dict(attack_type="untargeted", true=labels_ok[0], seed=5, stream=1, max_iter=1), **pk)),
                hsj_params(**dict(dict(grid=3, max_rounds=1, num_evals_init=4, num_evals_max=4), **kk)), a, i, **extra)
            ok = run({}, {})
            nan, inf = float("nan"), float("inf")
            bad = [({}, dict(grid=0)), ({}, dict(grid=65)), ({}, dict(max_rounds=0)), ({}, dict(max_rounds=33)),
                   ({}, dict(num_evals_init=0)), ({}, dict(num_evals_init=5)), ({}, dict(num_evals_max=1025)),
                   ({}, dict(max_queries=-1)), ({}, dict(sigma_min=0.0)), ({}, dict(sigma_min=-1.0)), ({}, dict(sigma_min=nan)),
                   ({}, dict(sigma_min=inf)), ({}, dict(probe_scale=-1.0)), ({}, dict(probe_scale=nan)), ({}, dict(probe_scale=inf)),
                   (dict(bits_per_sample=1), {}), (dict(bits_per_sample=17), {}), (dict(max_iter=-1), {})]
            bad += [(dict(true=v), {}) for v in labels_bad] + [(dict(attack_type="targeted", target=v), {}) for v in labels_bad]
            for pk, kk in bad:
                assert _code(lambda: run(pk, kk)) == FB_E_ARG, (case, pk, kk)
            assert _code(lambda: run({}, {}, i=None)) == FB_E_ARG               # a null init
            assert _code(lambda: run({}, {}, a=audio[:50], i=init[:50])) == FB_E_ARG   # shorter than one frame
            assert _code(lambda: run({}, {}, log_capacity=3 + 4 + 3 + 3 - 1)) == FB_E_ARG   # a decision log one entry short
            run({}, {}, log_capacity=3 + 4 + 3 + 3)
            for v in labels_ok:                                                # every decision value is a label
                run(dict(true=v), {})
                run(dict(attack_type="targeted", target=v), {})
            other = "CSI" if task != "CSI" else "OSI"
            assert _code(lambda: e.attack_hsj(nes_params(other, "untargeted", true=0, max_iter=1), hsj_params(), audio, init)) == FB_E_ARG
            # adver_thresh and the NES-only fields are not read
            junk = dict(adver_thresh=nan, epsilon=nan, samples_per_draw=-7, sigma=-1.0, max_lr=nan, min_lr=nan, momentum=nan,
                        plateau_length=-3, plateau_drop=0.0)
            got = run(junk, {})
            assert all(np.array_equal(got[k], ok[k]) for k in ok)
            e.set_eot(2)
            assert _code(lambda: run({}, {})) == FB_E_STATE
            e.set_eot(1)
            e.set_companions([CP.cast_i16(synthetic_audio(3, N), 16)])
            assert _code(lambda: run({}, {})) == FB_E_STATE
            e.set_companions(None)
            got = run({}, {})                                                   # the engine is as it was
            assert all(np.array_equal(got[k], ok[k]) for k in ok)
        finally:
            e.close()


# ------------------------------------------------------------------------------------- 6. HopSkipJump on top
def test_hopskipjump_on_top(small_system, tmp_path):
    model = _system("gmm CSI", small_system, tmp_path)
    e = model.engine
    try:
        audio, init, at, label, _thr = _setting(e, "gmm CSI")
        assert int(np.asarray(model.make_decisions(init)[0]).reshape(-1)[0]) == label
        h = H.HopSkipJump("CSI", "targeted", model, max_iter=2, seed=5, verbose=False)
        h._stream = 1
        cp = str(tmp_path / "hsj.cp")
        adv, flag = h.attack(audio, cp, target=label, init=np.concatenate([init, init]))   # a longer init is cropped
        assert adv.dtype == np.int16 and adv.shape == (N, 1) and flag == 1 and h._stream == 2
        direct = e.attack_hsj(_params(at, label, 0.0, "CSI", max_iter=2), hsj_params(), audio, init)
        assert np.array_equal(adv[:, 0], direct["adv"]) and h.n_queries == direct["n_queries"]
        assert h.dist == math.sqrt(direct["dist2"]) and h.linf_lsb >= 1 and np.isfinite(h.snr_db)
        print("HopSkipJump: |x - a| %.4g, SNR %.1f dB, Linf %d LSB, %d queries" % (h.dist, h.snr_db, h.linf_lsb, h.n_queries))
        with open(cp, "rb") as r:
            rows = pickle.load(r)
        assert len(rows) == 3 and all(len(row) == 9 and row[8] > 0 for row in rows)
        assert [row[:8] for row in rows] == direct["trace"].tolist()
        with pytest.raises(ValueError):
            h.attack(audio, None, target=label)                                 # targeted needs init
    finally:
        e.close()
