"""HopSkipJump without a GPU: the restatement of the header's "decision-only attack II" section (tests/hsj_ref.py) against
plain arithmetic, its bracket on synthetic decision tables, one whole attack with the CPU oracle's GMM scoring as the victim,
and the rules of fakebob_amd.hsj.HopSkipJump and of the driver."""
import contextlib
import io
import math
import os
import pickle

import numpy as np
import pytest

from fakebob_amd import attack_main as AM
from fakebob_amd import hsj as H
from fakebob_amd.models import stack_models, synthetic_audio, synthetic_gmm_system
from tests import hsj_ref as R
from tests.golden import driver_site as DS


# ------------------------------------------------------------------------------------------------ the arithmetic
@pytest.mark.parametrize("n", [1, 1023, 1024, 1025, 4099])
def test_ssq_is_a_sum_of_squares_to_4_ulp(n):
    """fixed order, float64: against the exactly rounded sum of the exact squares (math.fsum of fractions would be exact; the
    squares as float64 products carry half an ulp each, far inside the bound at these lengths)"""
    v = np.random.RandomState(n).uniform(-1.0, 1.0, n)
    want = math.fsum(float(t) * float(t) for t in v)
    got = R.ssq(v)
    print("n = %d: ssq %.17g, fsum %.17g, %.2f ulp" % (n, got, want, abs(got - want) / math.ulp(want)))
    assert abs(got - want) <= 4 * math.ulp(want)
    assert R.ssq_parts(v).shape == (-(-n // 1024),)
    assert R.ssq(np.zeros(n)) == 0.0


def test_line_ends():
    rs = np.random.RandomState(3)
    a, y = rs.uniform(-1, 1, 4099), rs.uniform(-1, 1, 4099)
    assert np.array_equal(R.line(a, y, 0), a)                                  # bit for bit
    assert np.abs(R.line(a, y, R.Q) - y).max() <= 2.0 ** -52                   # a + (y - a): y up to one rounding
    assert np.array_equal(R.line(a, y, R.Q // 2), a + 0.5 * (y - a))


def test_evals_and_weights():
    p = dict(R.DEFAULTS)
    assert [R.num_evals(p, t) for t in (1, 2, 3, 4, 63, 64, 65, 1000)] == [32, 45, 55, 64, 253, 256, 256, 256]
    assert R.num_evals(dict(p, num_evals_init=1, num_evals_max=1024), 10 ** 6) == 1000
    B = 6
    for n_plus in (0, 1, B - 1, B):
        flags = [j < n_plus for j in range(B)]
        w, got = R.weights(flags)
        assert got == n_plus and w.dtype == np.int32
        if n_plus in (0, B):
            assert w.tolist() == [1 if f else -1 for f in flags]              # all alike: phi itself
        else:
            assert w.tolist() == [(1 if f else -1) * B - (2 * n_plus - B) for f in flags]
            assert int(w.sum()) == 0 and all((v > 0) == f for v, f in zip(w.tolist(), flags))   # B (phi - mean(phi))
    assert R.sigma_of(p, 0.0, 4000) == 2.0 ** -15 and R.sigma_of(p, 2.43, 4000) == (0.05 * 2.43) / math.sqrt(4000.0)


# ------------------------------------------------------------------------------------------------ the bracket
def _check_bracket(truth, G, max_rounds):
    seen = {}

    def ok(qs):
        assert qs == sorted(set(qs)) and all(0 < q <= R.Q for q in qs) and len(qs) <= G
        for q in qs:
            seen[q] = truth(q)
        return [truth(q) for q in qs]
    hi, rounds, hist = R.bracket(ok, G, max_rounds)
    assert rounds == len(hist) <= max_rounds
    for lo_r, hi_r in hist:                                                    # lo always fails, hi always succeeds
        assert lo_r == 0 or seen[lo_r] is False
        assert hi_r == -1 or seen[hi_r] is True
        assert hi_r == -1 or lo_r < hi_r
    assert hi == hist[-1][1]
    return hi, rounds, hist


@pytest.mark.parametrize("G", [1, 2, 15, 64])
def test_bracket_on_a_monotone_table_finds_the_edge(G):
    for edge in (1, 2, 1000, 349525, R.Q - 1, R.Q):
        hi, rounds, hist = _check_bracket(lambda q: q >= edge, G, 32)
        assert hi == edge and hist[-1][0] in (edge - 1, 0)
        assert hist[0][1] != -1                                                # q = Q is scored in round 0
    assert _check_bracket(lambda q: q >= 1000, 1, 32)[1] <= 21                 # G = 1 is plain bisection of 2^20


def test_bracket_on_non_monotone_tables_keeps_its_invariant():
    rs = np.random.RandomState(5)
    for G in (1, 3, 15):
        for _ in range(20):
            cuts = sorted(rs.randint(1, R.Q, 5).tolist())
            truth = lambda q, c=cuts: (sum(1 for v in c if q >= v) % 2) == 1   # noqa: E731
            hi, _rounds, _hist = _check_bracket(truth, G, 32)
            assert hi == -1 or truth(hi)


def test_bracket_fails_in_round_0_and_stops_at_max_rounds():
    hi, rounds, hist = _check_bracket(lambda q: False, 15, 8)
    assert (hi, rounds, hist) == (-1, 1, [(0, -1)])
    hi, rounds, hist = _check_bracket(lambda q: q >= 12345, 2, 3)
    assert rounds == 3 and hi >= 12345 and hi - hist[-1][0] > 1
    calls = []
    hi, rounds, _ = R.bracket(lambda qs: [True] * len(qs), 4, 8, may_score=lambda r, rows: calls.append((r, rows)) or r == 0)
    assert rounds == 1 and hi == R.Q // 4 and calls == [(0, 4), (1, 4)]        # a refused round ends the search where it stands


# ------------------------------------------------------------------------------------------------ a whole attack
N = 4000


def _victim(oracle):
    _ubm, spk = synthetic_gmm_system(n_speakers=3, C=64, D=72)
    gc, miv, iv = stack_models(spk)
    cfg = oracle.default_cfg()

    def decide(rows):
        rows = [np.ascontiguousarray(r, np.int16) for r in rows]
        try:
            raw, _tv = oracle.gmm_score_batch(cfg, rows, gc, miv, iv, nthreads=4)
            return [int(np.argmax(r)) for r in raw]                            # CSI, z-norm (0, 1): the first maximum
        except RuntimeError:                                                   # some row has no voiced frames: one by one
            out = []
            for r in rows:
                try:
                    out.append(int(np.argmax(oracle.gmm_score_batch(cfg, [r], gc, miv, iv)[0][0])))
                except RuntimeError:
                    out.append(-2)
            return out
    return decide


def test_a_whole_attack_on_the_oracles_gmm_scoring(oracle):
    """3-speaker CSI, C = 64, N = 4000: from another utterance's decision towards utterance 0, six iterations"""
    decide = _victim(oracle)
    a = synthetic_audio(0, N)
    d0 = decide([R.cast_i16(a)])[0]
    start = None
    for seed in (1234, 99, 7):
        for u in (1, 2, 3):
            cand = synthetic_audio(u, N, seed)
            d = decide([R.cast_i16(cand)])[0]
            if d not in (d0, -2) and start is None:
                start, target = cand, d
    assert start is not None
    res = R.drive(a, start, dict(R.DEFAULTS), "targeted", target, oracle.noise, 1234, 0, 6, victim=decide)
    tr = res["trace"]
    scale = math.sqrt(N)
    print("clean decision %d, target %d; first boundary point |x - a| = %.4g" % (d0, target, math.sqrt(tr[0, 0])))
    for t in range(tr.shape[0]):
        print("  t = %d: dist %.4g (%.3g LSB rms), B %d, n+ %d, m %d, hi %d, rounds %d, queries %d, sigma %.3g" % (
            t, math.sqrt(tr[t, 0]), math.sqrt(tr[t, 0]) / scale * 32768, tr[t, 1], tr[t, 2], tr[t, 3], tr[t, 4], tr[t, 5], tr[t, 6], tr[t, 7]))
    assert res["success"] == 1 and tr[0, 4] >= 1                               # the start search succeeds
    assert res["adopted"] and all(d == target for d in res["adopted"])         # every adopted row was decided adversarial
    assert decide([res["adv"]])[0] == target
    assert res["n_iters"] == 6 and tr.shape == (7, 8) and res["n_queries"] == len(res["decisions"]) == int(tr[-1, 6])
    assert res["dist2"] == tr[-1, 0] < tr[0, 0]                                # closer than the first boundary point
    stalls = int((tr[1:, 4] < 0).sum())
    assert 2 * stalls <= res["n_iters"]                                        # a cap, not a measurement
    # the log replays the attack: the same batches, the same bits
    again = R.drive(a, start, dict(R.DEFAULTS), "targeted", target, oracle.noise, 1234, 0, 6, decisions=res["decisions"])
    assert np.array_equal(again["trace"], tr) and np.array_equal(again["adv"], res["adv"]) and np.array_equal(again["x"], res["x"])
    assert len(again["batches"]) == len(res["batches"]) and all(np.array_equal(p, q) for p, q in zip(again["batches"], res["batches"]))


def test_drive_honours_max_queries_and_a_failing_start(oracle):
    a, start = synthetic_audio(0, 2048), synthetic_audio(1, 2048)
    never = lambda rows: [0] * len(rows)                                        # noqa: E731
    res = R.drive(a, start, dict(R.DEFAULTS), "targeted", 1, oracle.noise, 5, 0, 3, victim=never)
    assert (res["success"], res["n_iters"], res["n_queries"]) == (-1, 0, 15) and np.array_equal(res["adv"], R.cast_i16(a))
    always = lambda rows: [1] * len(rows)                                       # noqa: E731
    for cap in (1, 15, 16, 30, 47, 62, 63, 200):
        res = R.drive(a, start, dict(R.DEFAULTS, max_queries=cap), "targeted", 1, oracle.noise, 5, 0, 3, victim=always)
        assert res["success"] == 1 and res["n_queries"] <= max(cap, 15)         # round 0 of the start search is exempt
        assert res["trace"].shape[0] == res["n_iters"] + 1 == len(res["xs"])


# ------------------------------------------------------------------------------------------------ HopSkipJump
class _Engine(object):
    """what HopSkipJump asks of an engine, with canned answers"""

    def __init__(self):
        self.calls = []

    def attack_hsj(self, p, k, audio, init):
        self.calls.append(dict(stream=p.stream, seed=p.seed, task=p.task, attack_type=p.attack_type, threshold=p.threshold,
                               target=p.target, true=p.true_label, bits=p.bits_per_sample, max_iter=p.max_iter, grid=k.grid,
                               max_rounds=k.max_rounds, b0=k.num_evals_init, b1=k.num_evals_max, max_queries=k.max_queries,
                               sigma_min=k.sigma_min, probe_scale=k.probe_scale, init=np.array(init), n=audio.size))
        adv = (np.trunc(audio * 2048.0) + 2).astype(np.int16)
        trace = np.array([[4.0, 0, 0, -1, 500, 3, 45, 0.0], [1.0, 32, 10, 0, 900, 4, 150, 0.001]])
        return dict(adv=adv, adv_f64=audio.copy(), success=1, dist2=1.0, n_iters=1, n_queries=150, trace=trace,
                    decisions=np.zeros(150, np.int32))

    def attack_iter_seconds(self, n):
        return 0.25 * np.arange(1, n + 1)

    def estimate_threshold(self, p, model_threshold, audio, noise_all=None, max_total_iters=0):
        self.calls.append(("estimate", p.stream, p.seed, p.attack_type))
        return 1.5, 7, 2, 1.75, audio


class _Model(object):
    """decisions read off the first sample, as the driver site's stub reads them: d = round(32768 x[0]) - 1"""

    def __init__(self, task):
        self.task, self.threshold, self.engine, self.seen = task, 0.5, _Engine(), []

    def make_decisions(self, audios, **kw):
        v = float(np.asarray(audios).reshape(-1)[0])
        self.seen.append(v)
        return (1 if v > 0.5 else 0), np.zeros(3)


def test_hopskipjump_checks_its_arguments():
    m = _Model("CSI")
    h = H.HopSkipJump("CSI", "targeted", m, seed=3, verbose=False)
    assert (h.grid, h.max_rounds, h.num_evals_init, h.num_evals_max, h.max_queries, h.sigma_min, h.probe_scale) == (
        15, 8, 32, 256, 0, 2.0 ** -15, 0.05)
    assert h.dist is None and h.snr_db is None and h.linf_lsb is None and h.n_queries == 0
    with pytest.raises(ValueError, match="foreign"):
        H.HopSkipJump("OSI", "untargeted", DS.StubModel("OSI"))                # score / make_decisions, no engine
    with pytest.raises(ValueError):
        H.HopSkipJump("SV", "untargeted", m)                                   # the model's task is CSI
    nan, inf = float("nan"), float("inf")
    bad = [dict(grid=0), dict(grid=65), dict(max_rounds=0), dict(max_rounds=33), dict(num_evals_init=0),
           dict(num_evals_init=300), dict(num_evals_max=1025), dict(max_queries=-1), dict(sigma_min=0.0), dict(sigma_min=nan),
           dict(sigma_min=inf), dict(probe_scale=-0.1), dict(probe_scale=nan), dict(probe_scale=inf), dict(max_iter=-1)]
    for kw in bad:
        with pytest.raises(ValueError):
            H.HopSkipJump("CSI", "targeted", m, **kw)
    for ok in (dict(grid=1), dict(grid=64), dict(max_rounds=32), dict(num_evals_init=1, num_evals_max=1),
               dict(num_evals_init=1024, num_evals_max=1024), dict(probe_scale=0.0), dict(max_iter=0)):
        H.HopSkipJump("CSI", "targeted", m, verbose=False, **ok)
    with pytest.raises(ValueError):
        H.HopSkipJump("XYZ", "targeted", m)
    with pytest.raises(ValueError):
        H.HopSkipJump("CSI", "sideways", m)


def test_hopskipjump_marshals_crops_tiles_and_writes_its_checkpoint(tmp_path):
    m = _Model("CSI")
    h = H.HopSkipJump("CSI", "targeted", m, grid=4, max_rounds=9, num_evals_init=8, num_evals_max=64, max_queries=500,
                      sigma_min=0.001, probe_scale=0.1, max_iter=7, seed=11, verbose=False)
    audio = np.linspace(-0.5, 0.5, 40)
    cp = str(tmp_path / "a.cp")
    adv, flag = h.attack(audio, cp, threshold=0.25, target=2, bits_per_sample=12, init=np.arange(100) / 128.0)
    c = m.engine.calls[-1]
    assert adv.dtype == np.int16 and adv.shape == (40, 1) and flag == 1 and h.n_queries == 150
    assert (c["stream"], c["seed"], c["task"], c["attack_type"], c["threshold"], c["target"], c["bits"], c["max_iter"]) == (
        0, 11, 1, 1, 0.25, 2, 12, 7)
    assert (c["grid"], c["max_rounds"], c["b0"], c["b1"], c["max_queries"], c["sigma_min"], c["probe_scale"]) == (4, 9, 8, 64, 500, 0.001, 0.1)
    assert np.array_equal(c["init"], np.arange(40) / 128.0)                    # a longer init is cropped
    assert h.dist == 1.0 and h.linf_lsb == 2 and h.snr_db == pytest.approx(
        10 * math.log10(np.sum(np.trunc(audio * 2048.0) ** 2) / np.sum((adv[:, 0] - np.trunc(audio * 2048.0)) ** 2)))
    h.attack(audio[:, None], None, target=2, init=[0.25, -0.25, 0.5])          # a column, no checkpoint; a shorter init is tiled
    c = m.engine.calls[-1]
    assert c["stream"] == 1 and np.array_equal(c["init"], np.tile([0.25, -0.25, 0.5], 14)[:40])
    with open(cp, "rb") as r:
        rows = pickle.load(r)
    assert rows == [[4.0, 0, 0, -1, 500, 3, 45, 0.0, 0.25], [1.0, 32, 10, 0, 900, 4, 150, 0.001, 0.5]]
    assert np.array_equal(H.fit_init(np.arange(5.0), 5), np.arange(5.0))
    with pytest.raises(ValueError):
        H.fit_init([], 5)
    with pytest.raises(ValueError):
        h.attack(audio, None, target=2)                                        # targeted, no init
    with pytest.raises(ValueError):
        h.attack(audio, None, init=audio)                                      # targeted, no target
    with pytest.raises(ValueError):
        h.attack(audio, None, target=2, init=audio, bits_per_sample=17)
    with pytest.raises(ValueError):
        H.HopSkipJump("CSI", "untargeted", m, verbose=False).attack(audio, None, init=audio)   # untargeted CSI needs `true`


def test_an_untargeted_attack_without_init_starts_from_noise():
    m = _Model("CSI")
    h = H.HopSkipJump("CSI", "untargeted", m, seed=21, verbose=False)
    audio = np.linspace(-0.5, 0.5, 40)
    rows = np.random.RandomState(21).uniform(-1.0, 1.0, (H.NOISE_STARTS, 40))
    want = [j for j in range(H.NOISE_STARTS) if (1 if rows[j, 0] > 0.5 else 0) != 0]
    assert want and want[0] > 0                                                 # (seed 21: not the first row)
    adv, flag = h.attack(audio, None, true=0)
    assert flag == 1 and np.array_equal(m.engine.calls[-1]["init"], rows[want[0]])
    assert m.seen == rows[:want[0] + 1, 0].tolist()                             # row by row, the first adversarial one is taken
    # no row is decided otherwise than `true`: the cast of the audio, -1, and the engine is not asked
    m2 = _Model("CSI")
    m2.make_decisions = lambda audios, **kw: (0, np.zeros(3))
    adv, flag = H.HopSkipJump("CSI", "untargeted", m2, seed=21, verbose=False).attack(audio, None, true=0)
    assert flag == -1 and adv.shape == (40, 1) and np.array_equal(adv[:, 0], np.trunc(audio * 32768.0).astype(np.int16))
    assert m2.engine.calls == []


def test_hopskipjump_borrows_fakebobs_threshold_sweep(monkeypatch):
    monkeypatch.delenv("FB_EOT_SIZE", raising=False)
    m = _Model("OSI")
    h = H.HopSkipJump("OSI", "untargeted", m, seed=11, verbose=False)
    h._stream = 4
    assert h.estimate_threshold(np.zeros(40))[:2] == (1.5, 7)
    assert m.engine.calls == [("estimate", 4, 11, 0)]
    assert h.threshold == 1.75 and h._stream == 5


# ------------------------------------------------------------------------------------------------ attack_main
@pytest.fixture()
def site(tmp_path):
    DS.make_site(str(tmp_path))
    old = os.getcwd()
    os.chdir(str(tmp_path))
    yield str(tmp_path)
    os.chdir(old)


class _Bob(DS.StubBob):
    inits = None

    def attack(self, audio, checkpoint_path, init=None, **kw):
        _Bob.inits.append(None if init is None else np.array(init))
        return DS.StubBob.attack(self, audio, checkpoint_path, **kw)


def _main(extra, built=None, attack_type="untargeted"):
    seen = []

    def bob(task, at, model, **hp):
        seen.append(hp)
        return _Bob(task, at, model, **hp)

    def model(archi, t, ml, pre, th, gid):
        if built is not None:
            built.append(gid)
        return DS.StubModel(t, th)
    DS.StubBob.log = []
    _Bob.inits = []
    argv = ["-spk_id"] + DS.SPK_IDS + ["-task", "OSI", "-type", attack_type, "--streams", "1", "--seed", "5"] + extra
    with contextlib.redirect_stdout(io.StringIO()), contextlib.redirect_stderr(io.StringIO()):
        res = AM.main(argv, model_factory=model, bob_factory=bob)
    return res, seen


def test_attack_main_hands_hsj_its_options(site):
    from scipy.io.wavfile import write
    wav = os.path.join(site, "start.wav")
    write(wav, 16000, np.array([16384, -8192, 0, 32767], np.int16))
    (g, results, _thr), seen = _main(["--attack", "hsj", "--hsj-init", wav, "--hsj-grid", "7", "--hsj-evals", "16:128",
                                      "--hsj-max-queries", "5000", "--hsj-sigma-min", "0.001", "--hsj-probe-scale", "0.2",
                                      "-max_iter", "9", "--eot-size", "1"])
    assert seen == [dict(grid=7, num_evals_init=16, num_evals_max=128, max_queries=5000, sigma_min=0.001, probe_scale=0.2, max_iter=9)]
    assert g[1] == len(results) == len(_Bob.inits) > 0
    assert all(np.array_equal(v, np.array([0.5, -0.25, 0.0, 32767 / 32768.0])) for v in _Bob.inits)
    _res, seen = _main(["--attack", "hsj"])                                     # untargeted: a noise start, no --hsj-init
    assert seen[0]["grid"] == 15 and (seen[0]["num_evals_init"], seen[0]["num_evals_max"]) == (32, 256)
    assert (seen[0]["max_queries"], seen[0]["sigma_min"], seen[0]["probe_scale"]) == (0, 2.0 ** -15, 0.05)
    assert _Bob.inits and all(v is None for v in _Bob.inits)
    _res, seen = _main([])                                                      # the default: nothing changes
    assert "grid" not in seen[0] and "samples_per_draw" in seen[0]


@pytest.mark.parametrize("extra", [["--eot-size", "2"], ["--companions", "1"], ["--hsj-grid", "1.5"], ["--hsj-evals", "32"],
                                   ["--hsj-evals", "a:b"], ["--hsj-max-queries", "many"], ["--hsj-sigma-min", "small"]])
def test_attack_main_refuses_before_any_model_is_built(site, extra):
    built = []
    with pytest.raises(SystemExit):
        _main(["--attack", "hsj"] + extra, built)
    assert built == []


def test_attack_main_refuses_a_targeted_hsj_without_a_start(site):
    built = []
    with pytest.raises(SystemExit):
        _main(["--attack", "hsj"], built, attack_type="targeted")
    assert built == []
