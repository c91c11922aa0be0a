"""ParticleSwarm, Kenansville and HopSkipJump against foreign victims on the device (fb_attack_pso_foreign,
fb_attack_kenansville_foreign, fb_attack_hsj_foreign; the "foreign victims" section of include/fakebob_hip.h).

The two kernels through their hooks against tests/foreign_attack_ref.py, bit for bit; then whole attacks, which ARE their
numpy drives: the victim is tests/golden/synth_model.SynthModel -- integer-exact, identical on every machine -- so the
restatements the native attacks are pinned to (hsj_ref.drive, kenansville_ref.search / candidates, pso_ref.replay), run against
the same victim, must give every output bit for bit, in every mode (host decisions, host scores, device float32 / float64).
Every comparison is np.array_equal: there is no tolerance in this file."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")   # ahead of the library: the model on the GPU and the engine share one HIP runtime

from fakebob_amd import foreign as FG  # noqa: E402
from fakebob_amd import companions as CP  # noqa: E402
from fakebob_amd._native import FB_E_ARG, FB_E_CALLBACK, FB_E_STATE, NativeError  # noqa: E402
from fakebob_amd.attack import FakeBob  # noqa: E402
from fakebob_amd.engine import Engine, hsj_params, kv_params, nes_params, pso_params  # noqa: E402
from fakebob_amd.hsj import HopSkipJump  # noqa: E402
from fakebob_amd.pso import ParticleSwarm  # noqa: E402
from tests import foreign_attack_ref as FR  # noqa: E402
from tests import hsj_ref as HR  # noqa: E402
from tests import kenansville_ref as KR  # noqa: E402
from tests import pso_ref as PR  # noqa: E402
from tests.foreign_models import TorchSynthModel  # noqa: E402
from tests.golden.synth_model import SynthModel, synth_audio  # noqa: E402

pytestmark = pytest.mark.gpu
N = 4000                                               # the utterance length of tests/test_gpu_hsj.py
HP = dict(HR.DEFAULTS, grid=5, num_evals_init=8, num_evals_max=16)
MAX_ITER, SEED, STREAM = 3, 7, 2
KV = dict(window=64, grid=4, q_max=65536, max_rounds=32)
PSO = dict(particles=4, w_init=0.9, w_end=0.4, c1=1.4961, c2=1.4961, v_max=0.002)
EPS = 0.002
SCORE_KW = dict(fs=16000, bits_per_sample=16, n_jobs=1, debug=False)


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    assert np.array_equal(got, want, equal_nan=got.dtype.kind == "f"), (what, int(np.flatnonzero((got != want).ravel())[0]))


# ------------------------------------------------------------------------------------- 1. the kernels, bit for bit
@pytest.mark.parametrize("bits", [16, 8])
@pytest.mark.parametrize("rows", [1, 3, 65])
def test_rows_to_model_hook(eng, rows, bits):
    for n in (1, 7, 8, 9, 1023, 4001):
        q = np.random.RandomState(rows * 7919 + n).randint(-32768, 32768, (rows, n)).astype(np.int16)
        q.reshape(-1)[:: max(q.size // 9, 1)] = np.resize(np.array([-32768, -1, 0, 32767], np.int16), q.reshape(-1)[:: max(q.size // 9, 1)].size)
        q.reshape(-1)[-1] = -32768                                               # the tail's last sample
        want = q.astype(np.float64) * 2.0 ** -(bits - 1)
        _same(eng.debug_rows_to_model(q, bits, np.float64), want, ("float64", rows, n, bits))
        _same(eng.debug_rows_to_model(q, bits, np.float32), want.astype(np.float32), ("float32", rows, n, bits))
        assert np.array_equal(want.astype(np.float32).astype(np.float64), want)   # the float32 value is exact too
    if rows == 1:
        q = np.array([[-32768, -1, 0, 32767]], np.int16)
        _same(eng.debug_rows_to_model(q, bits), q.astype(np.float64) * 2.0 ** -(bits - 1), "the four values")


def _score_rows(rows, S, dtype, thr):
    """random rows, and in fixed places: all scores equal, a maximum exactly at the threshold, a NaN in column 0, a NaN
    elsewhere, a tie of two maxima"""
    rs = np.random.RandomState(rows * 131 + S)
    sc = rs.normal(thr, 0.3, (rows, S))
    k = 0
    for fill in ("equal", "at_thr", "nan0", "nan_else", "tie"):
        for r in range(k, rows, 11):
            if fill == "equal":
                sc[r] = 0.25
            elif fill == "at_thr":
                sc[r] = rs.uniform(thr - 1.0, thr - 0.1, S); sc[r, S // 2] = thr
            elif fill == "nan0":
                sc[r, 0] = np.nan
            elif fill == "nan_else":
                sc[r, S - 1] = np.nan
            else:
                sc[r, S - 1] = sc[r, S // 3] = thr + 2.0
        k += 1
    return sc.astype(dtype)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("rows", [1, 65, 1024])
def test_decide_foreign_hook(eng, rows, dtype):
    thr = 0.5                                                                    # (exact in float32: "at the threshold" stays there)
    for task, sizes in (("SV", [1]), ("OSI", [1, 2, 61]), ("CSI", [1, 2, 61])):
        for S in sizes:
            sc = _score_rows(rows, S, dtype, thr)
            dec, wide = eng.debug_decide_foreign(sc, task, thr)
            want_dec, want_wide = FR.decide_rows(task, sc, thr)
            _same(wide, want_wide, ("scores", task, rows, S))
            _same(dec, want_dec, ("decisions", task, rows, S))
            if rows >= 65 and S > 1:
                assert len(set(dec.tolist())) >= 2                               # the data decides in more than one way
    for bad in (lambda: eng.debug_decide_foreign(np.zeros((1, 2)), "SV", 0.0), lambda: eng.debug_decide_foreign(np.zeros((1, 63)), "CSI", 0.0),
                lambda: eng.debug_rows_to_model(np.zeros((1, 4), np.int16), 17), lambda: eng.debug_rows_to_model(np.zeros((1, 4), np.int16), 1)):
        with pytest.raises(NativeError) as ex:
            bad()
        assert ex.value.code == FB_E_ARG


# ------------------------------------------------------------------------------------- 2. whole attacks are their drives
def _model(task, kind, **kw):
    """the victim of a case: SynthModel of a fixed seed per task; kind "host" or a torch dtype (the model on the GPU)"""
    args = (task, 3, N)
    seed = {"SV": 1, "CSI": 2}[task]
    if kind == "host":
        return SynthModel(*args, seed=seed, **kw)
    return TorchSynthModel(*args, seed=seed, device="cuda:0", device_dtype=kind, **kw)


_cases = {}


def _hsj_case(task):
    """SV: the threshold half way between the two clean scores, so that `init` is accepted and `audio` rejected, target 1.
    CSI, S = 3: target = the decision on `init`; the seeds were chosen on the CPU so that `audio` is decided otherwise."""
    if task not in _cases:
        m = _model(task, "host")
        if task == "SV":
            a, i = synth_audio(N, 1), synth_audio(N, 2)
            sa, si = float(m.score(a)), float(m.score(i))
            if si < sa:
                a, i, sa, si = i, a, si, sa
            thr, label = 0.5 * (sa + si), 1
            m.threshold = thr
            assert m.make_decisions(i)[0] == 1 and m.make_decisions(a)[0] == -1
        else:
            a, i, thr = synth_audio(N, 3), synth_audio(N, 4), 0.0
            label = int(m.make_decisions(i)[0])
            assert int(m.make_decisions(a)[0]) != label                          # nothing to do otherwise
        _cases[task] = (a, i, thr, label)
    return _cases[task]


def _spec(eng, task, model, rows_max, decisions, n=N):
    """(the victim dict of Engine.attack_*_foreign, the Victim) as the attack classes build it, on the shared engine"""
    vic = FG.Victim("test", task, model, decisions)
    vic._engine = eng
    return vic.spec(rows_max, n, None, **SCORE_KW), vic


def _run_hsj(eng, task, model, hp=HP, max_iter=MAX_ITER, **kw):
    a, i, thr, label = _hsj_case(task)
    spec, vic = _spec(eng, task, model, max(hp["grid"], hp["num_evals_max"]), True)
    p = nes_params(task, "targeted", threshold=thr, target=label, seed=SEED, stream=STREAM, max_iter=max_iter)
    return eng.attack_hsj_foreign(p, hsj_params(**hp), spec, a, i, keep_x=True, **kw), vic


_drives = {}


def _hsj_drive(oracle, task, odd=False, hp=HP, max_iter=MAX_ITER):
    key = ("hsj", task, odd, tuple(sorted(hp.items())), max_iter)
    if key not in _drives:
        a, i, thr, label = _hsj_case(task)
        m = _model(task, "host", threshold=thr)
        _drives[key] = FR.drive_hsj(FR.model_victim(m, every_odd_undecided=odd), a, i, hp, "targeted", label, oracle.noise, SEED,
                                    STREAM, max_iter)
    return _drives[key]


def _check_hsj(res, want):
    assert (res["success"], res["n_iters"], res["n_queries"]) == (want["success"], want["n_iters"], want["n_queries"])
    _same(res["decisions"], np.array(want["decisions"], np.int32), "decisions")
    _same(res["trace"], want["trace"], "trace")
    _same(res["adv"], want["adv"], "adv_i16")
    _same(res["adv_f64"], want["x"], "x")
    assert res["dist2"] == want["dist2"] and res["xs"].shape[0] == len(want["xs"])
    for t, x in enumerate(want["xs"]):
        _same(res["xs"][t], x, ("x_t", t))


@pytest.mark.parametrize("task", ["SV", "CSI"])
def test_hopskipjump_is_its_drive_in_every_mode(eng, oracle, task):
    _a, _i, thr, label = _hsj_case(task)
    want = _hsj_drive(oracle, task)
    # by construction the case cannot be vacuous: both sides of the boundary are scored, and the walk leaves the start
    assert want["success"] == 1 and len(set(want["decisions"])) >= 2 and label in want["decisions"]
    assert (want["trace"][1:, 4] >= 0).any()
    m1 = _model(task, "host", threshold=thr)                                     # 1: host decisions (make_decisions wins over score)
    r1, vic = _run_hsj(eng, task, m1)
    assert vic.mode == FG.HOST_DECISIONS
    _check_hsj(r1, want)
    info = eng.debug_foreign_path()
    assert info["path"] == "host" and info["model_calls"] == len(want["batches"]) == m1.n_calls
    assert info["batch_bytes_d2h"] == 8 * N * want["n_queries"] and m1.n_scored == want["n_queries"]
    secs = eng.attack_iter_seconds(r1["trace"].shape[0])
    assert secs.shape == (r1["trace"].shape[0],) and np.all(secs > 0)
    m2 = FR.ScoreOnly(_model(task, "host"))                                      # 2: host scores, the rule on the device
    r2, vic = _run_hsj(eng, task, m2)
    assert vic.mode == FG.HOST_SCORES and m2.n_calls == len(want["batches"])
    for key in r1:
        _same(r2[key], r1[key], ("host scores", key))
    for dt in (torch.float32, torch.float64):                                    # 3: the model on the GPU
        m3 = _model(task, dt)
        r3, vic = _run_hsj(eng, task, m3)
        assert vic.mode == FG.DEVICE_SCORES
        for key in r2:
            _same(r3[key], r2[key], ("device", dt, key))
        info = eng.debug_foreign_path()
        assert info["path"] == "device" and info["x_dtype"] == str(dt).split(".")[1] and info["score_dtype"] == "float64"
        assert m3.n_dev_calls == len(want["batches"]) == info["model_calls"] and m3.n_dev_scored == want["n_queries"]
        assert info["batch_bytes_d2h"] == 0 and m3.n_calls == 0


def _kv_case():
    if "kv" not in _cases:
        a = synth_audio(N, 2)
        x = HR.cast_i16(a)
        m = _model("SV", "host")
        c0, c1 = float(m.score(x)), float(m.score(KR.remove(x, KV["window"], KV["q_max"])))
        thr = 0.5 * (c0 + c1)
        m.threshold = thr
        true = int(m.make_decisions(x)[0])
        assert int(m.make_decisions(KR.remove(x, KV["window"], KV["q_max"]))[0]) != true     # q_max is a success, q = 0 is not
        _cases["kv"] = (a, thr, true)
    return _cases["kv"]


def _run_kv(eng, model):
    a, thr, true = _kv_case()
    spec, vic = _spec(eng, "SV", model, KV["grid"], True)
    p = nes_params("SV", "untargeted", threshold=thr, true=true, seed=SEED, stream=STREAM)
    return eng.attack_kenansville_foreign(p, kv_params(**KV), spec, a), vic


def _kv_drive(odd=False):
    if ("kv", odd) not in _drives:
        a, thr, true = _kv_case()
        m = _model("SV", "host", threshold=thr)
        _drives[("kv", odd)] = FR.drive_kenansville(FR.model_victim(m, every_odd_undecided=odd), a, KV["window"], KV["grid"],
                                                    KV["q_max"], KV["max_rounds"], "untargeted", true)
    return _drives[("kv", odd)]


def _check_kv(res, want):
    assert (res["success"], res["factor"], res["n_queries"]) == (want["success"], want["factor"], want["n_queries"])
    for key in ("qs", "decisions", "trace", "adv"):
        _same(res[key], want[key], key)


def test_kenansville_is_its_drive_in_every_mode(eng):
    a, thr, true = _kv_case()
    want = _kv_drive()
    assert want["success"] == 1 and want["trace"].shape[0] >= 2                  # not vacuous: the bracket narrows
    m1 = _model("SV", "host", threshold=thr)
    r1, vic = _run_kv(eng, m1)
    assert vic.mode == FG.HOST_DECISIONS and r1["success"] == 1 and r1["trace"].shape[0] >= 2
    _check_kv(r1, want)
    n_rounds = want["trace"].shape[0]
    assert m1.n_calls == n_rounds == eng.debug_foreign_path()["model_calls"]
    # the score log holds the model's scores of the rows it was handed: the candidates, cast back
    ref = _model("SV", "host")
    for r in (0, n_rounds - 1):
        rows = int(want["trace"][r, 2])
        sc = ref.raw(list(KR.candidates(want["x"], KV["window"], want["qs"][r, :rows])))
        _same(r1["scores"][r, :rows], sc, ("scores", r))
        assert np.all(np.isnan(r1["scores"][r, rows:]))
    m0 = FR.DecisionsOnly(_model("SV", "host", threshold=thr), scores=False)     # decisions without scores: NaN in the log
    r0, vic = _run_kv(eng, m0)
    assert vic.mode == FG.HOST_DECISIONS and np.all(np.isnan(r0["scores"]))
    _check_kv(r0, want)
    for b in m0.batches:                                                         # what the victim saw: int16 rows, scaled exactly
        assert b.dtype == np.float64 and b.shape[0] == N and b.flags["C_CONTIGUOUS"]
        assert np.array_equal(b * 32768.0, np.trunc(b * 32768.0)) and np.abs(b).max() <= 1.0
    _same(m0.batches[0].T, FR.rows_to_model(KR.candidates(want["x"], KV["window"], want["qs"][0])), "the first batch")
    m2 = FR.ScoreOnly(_model("SV", "host"))
    r2, vic = _run_kv(eng, m2)
    assert vic.mode == FG.HOST_SCORES
    for key in r1:
        _same(r2[key], r1[key], ("host scores", key))
    for dt in (torch.float32, torch.float64):
        m3 = _model("SV", dt)
        r3, vic = _run_kv(eng, m3)
        assert vic.mode == FG.DEVICE_SCORES and eng.debug_foreign_path()["path"] == "device"
        for key in r2:
            _same(r3[key], r2[key], ("device", dt, key))
        assert m3.n_dev_calls == n_rounds and m3.n_dev_scored == want["n_queries"]
    # x off every 16-byte boundary: the conversion goes element by element, to the same bits
    m4 = _model("SV", torch.float32)
    spec, _vic = _spec(eng, "SV", m4, KV["grid"], True)
    spec["x"] = torch.empty(KV["grid"] * N + 1, dtype=torch.float32, device="cuda:0")[1:]
    assert spec["x"].data_ptr() % 16 == 4 and spec["x"].is_contiguous()
    r4 = eng.attack_kenansville_foreign(nes_params("SV", "untargeted", threshold=thr, true=true, seed=SEED, stream=STREAM),
                                        kv_params(**KV), spec, a)
    for key in r2:
        _same(r4[key], r2[key], ("device, x unaligned", key))


def _run_pso(eng, model, thr):
    a = synth_audio(N, 1)
    spec, vic = _spec(eng, "SV", model, PSO["particles"], False)
    p = nes_params("SV", "targeted", epsilon=EPS, max_iter=3, threshold=thr, seed=SEED, stream=STREAM)
    return eng.attack_pso_foreign(p, pso_params(**PSO), spec, a), vic


def test_particle_swarm_is_its_replay_in_every_mode(eng, oracle):
    a = synth_audio(N, 1)
    ref = _model("SV", "host")
    thr = float(ref.score(a)) + 0.5                                              # out of the ball's reach: all three iterations run
    fb = FakeBob("SV", "targeted", ref, verbose=False)
    fb.threshold = thr
    log = []

    def losses(k, x):                                                            # the model's own losses of the swarm's rows
        l, sc = fb.loss_fn([PR.cast_i16(row) for row in x])
        log.append(np.asarray(sc, np.float64).reshape(len(x), 1))
        return l.reshape(-1)
    want = PR.replay(oracle.philox, a, losses, eps=EPS, max_iter=3, P=PSO["particles"], w_init=PSO["w_init"], w_end=PSO["w_end"],
                     c1=PSO["c1"], c2=PSO["c2"], v_max=PSO["v_max"], seed=SEED, stream=STREAM, scores=log)
    assert want["n_iters"] == 3 and want["success"] == -1
    m2 = FR.ScoreOnly(_model("SV", "host"))
    (adv, flag, adv_f, trace, got_l), vic = _run_pso(eng, m2, thr)
    assert vic.mode == FG.HOST_SCORES and m2.n_calls == 3 and eng.debug_foreign_path()["path"] == "host"
    assert (trace.shape[0], flag) == (want["n_iters"], want["success"])
    _same(trace, want["trace"], "trace")
    _same(adv_f, want["adv_f64"], "adv_f64")
    _same(adv, want["adv_i16"], "adv_i16")
    assert len({float(v) for v in got_l.reshape(-1)}) == got_l.size             # twelve different rows were scored
    # (the losses drove the replay: recomputed here from the model on the rows the replay wrote)
    _same(got_l, np.stack([fb.threshold - log[k][:, 0] for k in range(3)]), "losses")
    for dt in (torch.float32, torch.float64):
        m3 = _model("SV", dt)
        got, vic = _run_pso(eng, m3, thr)
        assert vic.mode == FG.DEVICE_SCORES and m3.n_dev_calls == 3 and eng.debug_foreign_path()["path"] == "device"
        for k, (g, w) in enumerate(zip(got, (adv, flag, adv_f, trace, got_l))):
            _same(g, w, ("device", dt, k))
    # a model with make_decisions as well is still asked for scores: PSO reads no decisions
    assert _spec(eng, "SV", _model("SV", "host"), 4, False)[1].mode == FG.HOST_SCORES


# ------------------------------------------------------------------------------------- 3. no decision (-2)
def test_rows_without_a_decision_are_never_adopted(eng, oracle):
    _a, _i, thr, _label = _hsj_case("SV")
    want = _hsj_drive(oracle, "SV", odd=True)
    m = FR.DecisionsOnly(_model("SV", "host", threshold=thr), odd_undecided=True)
    res, vic = _run_hsj(eng, "SV", m)
    assert vic.mode == FG.HOST_DECISIONS
    _check_hsj(res, want)
    assert -2 in want["decisions"] and want["success"] == 1 and -2 not in want["adopted"] and want["adopted"]
    a, thr, true = _kv_case()
    want = _kv_drive(odd=True)
    m = FR.DecisionsOnly(_model("SV", "host", threshold=thr), odd_undecided=True)
    res, _vic = _run_kv(eng, m)
    _check_kv(res, want)
    assert -2 in want["decisions"] and want["success"] == 1 and want["adopted"] not in (-2, None)
    hit = np.argwhere(res["qs"] == res["factor"])
    assert all(res["decisions"][r, j] != -2 for r, j in hit)                     # the returned candidate was decided


# ------------------------------------------------------------------------------------- 4. the same rows as the native attack
class _SystemAsForeign(object):
    """one of the package's systems behind the plugin API: score / make_decisions of a SECOND system object of the same
    models (no defences), so that the attack's engine holds no model at all"""

    def __init__(self, system):
        self.sys, self.task, self.spk_ids, self.rows = system, system.task, system.spk_ids, []

    def _rows(self, audios):
        a = np.asarray(audios, np.float64)
        q = CP.cast_i16(a.T.reshape(-1), 16).reshape(a.shape[1], a.shape[0])
        assert np.array_equal(q.astype(np.float64) * 2.0 ** -15, a.T)            # the rows cast back to the same int16
        self.rows.append(q)
        return a

    def score(self, audios, **kw):
        return self.sys.score(self._rows(audios), **kw)

    def make_decisions(self, audios, **kw):
        return self.sys.make_decisions(self._rows(audios), **kw)


def test_the_rows_are_the_native_attacks(small_system, tmp_path):
    from tests.test_gpu_hsj import _params, _setting, _system
    (tmp_path / "a").mkdir()
    (tmp_path / "b").mkdir()
    native, twin = _system("gmm CSI", small_system, tmp_path / "a"), _system("gmm CSI", small_system, tmp_path / "b")
    h1 = s1 = None
    try:
        audio, init, at, label, thr = _setting(native.engine, "gmm CSI")
        hp = dict(HR.DEFAULTS, grid=5, num_evals_init=8, num_evals_max=16)
        want = native.engine.attack_hsj(_params(at, label, thr, "CSI", max_iter=2), hsj_params(**hp), audio, init, keep_x=True)
        assert want["success"] == 1 and -2 not in want["decisions"]              # no row is unvoiced
        h0 = HopSkipJump("CSI", at, native, max_iter=2, seed=5, verbose=False, **{k: hp[k] for k in ("grid", "num_evals_init", "num_evals_max")})
        h1 = HopSkipJump("CSI", at, _SystemAsForeign(twin), max_iter=2, seed=5, verbose=False, foreign=True,
                         **{k: hp[k] for k in ("grid", "num_evals_init", "num_evals_max")})
        h0._stream = h1._stream = 1
        (adv0, flag0), (adv1, flag1) = h0.attack(audio, None, target=label, init=init), h1.attack(audio, None, target=label, init=init)
        assert h1._victim.mode == FG.HOST_DECISIONS and flag0 == flag1 == 1
        _same(adv1, adv0, "HopSkipJump's audio")
        assert (h1.n_queries, h1.dist) == (h0.n_queries, h0.dist)
        _same(adv0[:, 0], want["adv"], "the class is the engine call")
        spec, _vic = _spec(h1._victim.engine(), "CSI", _SystemAsForeign(twin), 16, True)
        got = h1._victim.engine().attack_hsj_foreign(_params(at, label, thr, "CSI", max_iter=2), hsj_params(**hp), spec, audio, init,
                                                     keep_x=True)
        for key in want:
            _same(got[key], want[key], ("hsj", key))
        spec, _vic = _spec(h1._victim.engine(), "CSI", FR.ScoreOnly(_SystemAsForeign(twin)), 16, True)
        got = h1._victim.engine().attack_hsj_foreign(_params(at, label, thr, "CSI", max_iter=2), hsj_params(**hp), spec, audio, init,
                                                     keep_x=True)
        for key in want:
            _same(got[key], want[key], ("hsj, scores", key))
        # ParticleSwarm: the swarm's rows and losses
        true = int(native.make_decisions(audio)[0])
        kw = dict(adver_thresh=1e3, epsilon=EPS, max_iter=3, n_particles=4, seed=5, verbose=False)
        s0, s1 = ParticleSwarm("CSI", "untargeted", native, **kw), ParticleSwarm("CSI", "untargeted", _SystemAsForeign(twin), foreign=True, **kw)
        (p0, f0), (p1, f1) = s0.attack(audio, None, true=true), s1.attack(audio, None, true=true)
        assert s1._victim.mode == FG.HOST_SCORES and f0 == f1
        _same(p1, p0, "ParticleSwarm's audio")
        p = nes_params("CSI", "untargeted", adver_thresh=1e3, epsilon=EPS, max_iter=3, true=true, seed=5, stream=0)
        q = pso_params(4, 0.9, 0.1, 1.4961, 1.4961, EPS)
        spec, _vic = _spec(s1._victim.engine(), "CSI", _SystemAsForeign(twin), 4, False)
        for k, (g, w) in enumerate(zip(s1._victim.engine().attack_pso_foreign(p, q, spec, audio), native.engine.attack_pso(p, q, audio))):
            _same(g, w, ("pso", k))
    finally:
        native.engine.close()
        twin.engine.close()
        for h in (h1, s1):
            if h is not None and h._victim._engine is not None:
                h._victim._engine.close()


# ------------------------------------------------------------------------------------- 5. refusals and recovery
def _code(fn):
    with pytest.raises(NativeError) as ex:
        fn()
    return ex.value


class _Boom(Exception):
    pass


def test_refusals_leave_the_engine_usable(oracle):
    _a, _i, thr, label = _hsj_case("SV")
    want = _hsj_drive(oracle, "SV")
    e = Engine(0)
    try:
        def good():
            res, _vic = _run_hsj(e, "SV", _model("SV", "host", threshold=thr))
            _check_hsj(res, want)                                                # (a fresh engine gives the drive as well: section 2)

        good()

        class Bad(FR.DecisionsOnly):
            def make_decisions(self, audios, **kw):
                dec, sc = FR.DecisionsOnly.make_decisions(self, audios, **kw)
                return [7] * np.asarray(audios).shape[1], sc
        ex = _code(lambda: _run_hsj(e, "SV", Bad(_model("SV", "host", threshold=thr))))
        assert ex.code == FB_E_CALLBACK and "returned 7" in str(ex)                       # a decision outside the task's values, named
        good()

        class Raises(FR.DecisionsOnly):
            def make_decisions(self, audios, **kw):
                if self.n_calls >= 2:
                    raise _Boom("the model's own")
                return FR.DecisionsOnly.make_decisions(self, audios, **kw)
        with pytest.raises(_Boom):
            _run_hsj(e, "SV", Raises(_model("SV", "host", threshold=thr)))
        good()

        class RaisesOnDevice(TorchSynthModel):
            def score_device(self, x):
                if self.n_dev_calls >= 1:
                    raise _Boom("the model's own")
                return TorchSynthModel.score_device(self, x)
        with pytest.raises(_Boom):
            _run_hsj(e, "SV", RaisesOnDevice("SV", 3, N, seed=1, device="cuda:0", device_dtype=torch.float32))
        good()
        # the engine's own randomness and utterances are not a foreign victim's
        for on, off, name in ((lambda: e.set_eot(2), lambda: e.set_eot(1), "fb_set_eot"),
                              (lambda: e.set_companions([HR.cast_i16(synth_audio(N, 9))]), lambda: e.set_companions(None), "fb_set_companions"),
                              (lambda: e.set_play_offset(100), lambda: e.set_play_offset(0), "fb_set_play_offset"),
                              (lambda: e.set_query_eot("majority"), lambda: e.set_query_eot(None), "fb_set_query_eot")):
            on()
            try:
                for run in (lambda: _run_hsj(e, "SV", _model("SV", "host", threshold=thr)), lambda: _run_kv(e, _model("SV", "host")),
                            lambda: _run_pso(e, _model("SV", "host"), 0.0)):
                    ex = _code(run)
                    assert ex.code == FB_E_STATE and name in str(ex), (name, str(ex))
            finally:
                off()
            good()
        # a device x buffer one row too small.  The library checks against the extent of the ALLOCATION, and torch rounds
        # an allocation of 10 MiB or more up to a multiple of 2 MiB of its own: 393 rows of 4000 float64 are 12 576 000 bytes
        # in an allocation of 6 * 2 MiB = 12 582 912, and 394 rows need 12 608 000
        a, i, _thr, _label = _hsj_case("SV")
        m = _model("SV", torch.float64)
        spec, _vic = _spec(e, "SV", m, 394, True)
        del spec["x"]
        torch.cuda.empty_cache()                                                # (no larger cached block to be handed out)
        small = dict(spec, x=torch.empty((393, N), dtype=torch.float64, device="cuda:0"), check_extent=False)
        p = nes_params("SV", "targeted", threshold=thr, target=label, seed=SEED, stream=STREAM, max_iter=MAX_ITER)
        ex = _code(lambda: e.attack_hsj_foreign(p, hsj_params(**dict(HP, num_evals_max=394)), small, a, i))
        assert ex.code == FB_E_ARG and "x:" in str(ex) and m.n_dev_calls == 0, str(ex)
        del small
        good()
        # PSO reads scores
        spec, _vic = _spec(e, "SV", _model("SV", "host"), 4, True)
        assert spec["mode"] == FG.HOST_DECISIONS
        pp = nes_params("SV", "targeted", epsilon=EPS, max_iter=3, threshold=thr, seed=SEED, stream=STREAM)
        assert _code(lambda: e.attack_pso_foreign(pp, pso_params(**PSO), spec, a)).code == FB_E_ARG
        # the descriptor's own rules
        ok_spec, _vic = _spec(e, "SV", FR.ScoreOnly(_model("SV", "host")), 16, True)
        for bad in (dict(ok_spec, mode=9), dict(ok_spec, fn=None), dict(ok_spec, S=0), dict(ok_spec, S=63), dict(ok_spec, S=2)):
            assert _code(lambda: e.attack_hsj_foreign(p, hsj_params(**HP), bad, a, i)).code == FB_E_ARG, bad
        assert _code(lambda: e.attack_hsj_foreign(nes_params("SV", "targeted", target=0), hsj_params(**HP), ok_spec, a, i)).code == FB_E_ARG
        tiny, _vic = _spec(e, "SV", FR.ScoreOnly(SynthModel("SV", 1, 1, seed=1)), 1, True, n=1)
        one = e.attack_hsj_foreign(nes_params("SV", "targeted", threshold=-1e9, target=1, max_iter=0), hsj_params(grid=1, max_rounds=1),
                                   tiny, a[:1], i[:1])                           # N = 1 suffices: there is no front end
        assert (one["n_queries"], one["success"], one["decisions"].tolist()) == (1, 1, [1])
        _same(one["adv"], HR.cast_i16(i[:1]), "the one sample")
        good()
    finally:
        e.close()


def test_max_queries_is_honoured_exactly(eng, oracle):
    """tests/test_gpu_hsj.py's construction, in host-decisions mode: round 0 of the start is exempt, the probes (8 rows at t =
    1) and the step batch (5 rows) are scored whole or not at all, and a cut attack is the free one cut short"""
    _a, _i, thr, _label = _hsj_case("CSI")
    free, _vic = _run_hsj(eng, "CSI", _model("CSI", "host"), max_iter=2)
    marks = free["trace"][:, 6].astype(int).tolist()                            # rows scored after the start and each iteration
    cut = {}
    for cap in (1, marks[0] - 1, marks[0] + 7, marks[0] + 8, marks[0] + 12, marks[0] + 13, marks[1] - 1, marks[2]):
        hp = dict(HP, max_queries=cap)
        m = _model("CSI", "host")
        res, _vic = _run_hsj(eng, "CSI", m, hp=hp, max_iter=2)
        _check_hsj(res, _hsj_drive(oracle, "CSI", hp=hp, max_iter=2))
        assert res["n_queries"] <= max(cap, 5) and res["success"] == 1 and m.n_scored == res["n_queries"]
        _same(res["decisions"], free["decisions"][:res["n_queries"]], "the same attack, cut short")
        cut[cap] = res["n_queries"]
    assert [cut[marks[0] + k] for k in (7, 8, 12, 13)] == [marks[0], marks[0] + 8, marks[0] + 8, marks[0] + 13]
    assert cut[1] == 5 and cut[marks[2]] == marks[2]


# ------------------------------------------------------------------------------------- 6. the classes on top
def test_the_classes_run_on_an_engine_of_their_own(oracle):
    a, i, thr, label = _hsj_case("SV")
    want = _hsj_drive(oracle, "SV")
    m = _model("SV", torch.float32)
    h = HopSkipJump("SV", "targeted", m, max_iter=MAX_ITER, seed=SEED, verbose=False, foreign=True, grid=5, num_evals_init=8, num_evals_max=16)
    try:
        h._stream = STREAM
        adv, flag = h.attack(a, None, threshold=thr, target=label, init=i)
        assert h._victim.mode == FG.DEVICE_SCORES and flag == 1 and h.n_queries == want["n_queries"]
        _same(adv[:, 0], want["adv"], "adv")
        # a model with score_device alone: the noise start takes its decisions through the score rule
        only = type("DeviceOnly", (object,), dict(task="SV", spk_ids=m.spk_ids, device_dtype=torch.float32,
                                                  score_device=lambda self, x: m.score_device(x)))()
        u = HopSkipJump("SV", "untargeted", only, max_iter=1, seed=SEED, verbose=False, foreign=True, grid=5, num_evals_init=8, num_evals_max=16)
        try:
            rs = np.random.RandomState(SEED & 0xFFFFFFFF)
            row = rs.uniform(-1.0, 1.0, N)
            d0 = FR.decide_rows("SV", [[float(m.score(row))]], thr)[0][0]
            start = u._noise_start(N, -d0, None, thr, **SCORE_KW)                # true = the other decision: the first row is wanted
            _same(start, row, "the first noise row")
        finally:
            if u._victim._engine is not None:
                u._victim._engine.close()
        # estimate_threshold still delegates to FakeBob, which takes foreign models
        k = HopSkipJump("SV", "targeted", _model("SV", "host", threshold=thr), seed=SEED, verbose=False, foreign=True)
        assert k.estimate_threshold.__func__ is HopSkipJump.estimate_threshold
    finally:
        if h._victim._engine is not None:
            h._victim._engine.close()
