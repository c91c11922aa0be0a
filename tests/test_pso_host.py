"""The particle-swarm attack without a GPU: the numpy restatement (tests/pso_ref.py) against the contract's own claims --
exact uniforms, the tie and stop rules of the state machine, the ball and the velocity clamp --, then ParticleSwarm's
argument checks and attack_main's new flags, with stub models as tests/test_driver_rules.py uses them."""
import contextlib
import io
import os
import pickle
from fractions import Fraction

import numpy as np
import pytest

from fakebob_amd import attack_main as AM
from fakebob_amd.pso import ParticleSwarm
from tests import pso_ref as R
from tests.golden import driver_site as DS

SEED, STREAM = 0xC0FFEE1234567, 5
KW = dict(eps=0.002, P=3, w_init=0.9, w_end=0.1, c1=1.4961, c2=1.4961, v_max=0.002, seed=SEED, stream=STREAM)


@pytest.fixture(scope="module")
def philox(oracle):
    return oracle.philox


@pytest.fixture(scope="module")
def audio():
    return np.random.RandomState(4).uniform(-0.5, 0.5, 7)


# ------------------------------------------------------------------------------------------------ uniforms
def test_uniforms_are_exact_and_inside_the_open_interval():
    for w in (0, 1, 2 ** 31, 2 ** 32 - 2, 2 ** 32 - 1, 0x9E3779B9):
        u = float(R.U(w))
        assert Fraction(u) == Fraction(2 * w + 1, 2 ** 33)                     # no rounding anywhere
        assert 0.0 < u < 1.0
        assert Fraction(2.0 * u - 1.0) == Fraction(2 * w + 1 - 2 ** 32, 2 ** 32)   # 2 u - 1 is exact as well
    assert float(R.U(0)) == 2.0 ** -33 and float(R.U(2 ** 32 - 1)) == 1.0 - 2.0 ** -33


def test_uniforms_follow_the_counter_layout(philox):
    n, P, t = 5, 3, 4
    u1, u2 = R.uniforms(philox, SEED, STREAM, t, P, n)
    key = [(SEED & 0xFFFFFFFF) ^ 0x5053574D, (SEED >> 32) ^ STREAM]
    for p in range(P):
        for i in range(n):
            w = philox([i >> 1, p, t, 0], key)
            assert u1[p, i] == (w[2 * (i & 1)] + 0.5) / 2 ** 32 and u2[p, i] == (w[2 * (i & 1) + 1] + 0.5) / 2 ** 32
    # both key words matter
    assert not np.array_equal(u1, R.uniforms(philox, SEED, STREAM + 1, t, P, n)[0])
    assert not np.array_equal(u1, R.uniforms(philox, SEED ^ 1, STREAM, t, P, n)[0])


# ------------------------------------------------------------------------------------------------ the state machine
def test_ties_go_to_the_lowest_particle_and_an_equal_loss_replaces_nothing(philox, audio):
    losses = [[0.5, 0.5, 0.7],
              [0.5, 0.3, 0.3],     # particle 0 repeats its loss: no improvement; 1 and 2 tie at the new minimum: 1 wins
              [0.4, 0.3, 0.3],     # 0 improves, 1 and 2 repeat theirs: gl, g stay
              [0.4, 0.35, 0.2]]
    r = R.replay(philox, audio, losses, max_iter=4, keep=(0, 1, 2, 3), **KW)
    assert r["n_iters"] == 4 and r["success"] == -1
    assert r["trace"][:, 0].tolist() == [0.5, 0.3, 0.3, 0.2]
    assert r["trace"][:, 1].tolist() == [0.0, 1.0, 1.0, 2.0]
    assert r["trace"][:, 2].tolist() == [3.0, 2.0, 1.0, 1.0]
    assert np.array_equal(r["adv_f64"], r["positions"][3][2])                  # the position that was scored
    assert np.array_equal(r["adv_i16"], R.cast_i16(r["adv_f64"]))


def test_stop_rules(philox, audio):
    # at k = 0: particle 0 is the audio itself
    r = R.replay(philox, audio, [[-0.1, 0.2, 0.3]], max_iter=5, **KW)
    assert (r["n_iters"], r["success"]) == (1, 1) and np.array_equal(r["adv_f64"], audio)
    # exactly at max_iter - 1 with a negative loss: success
    r = R.replay(philox, audio, [[0.3, 0.2, 0.3], [0.3, 0.1, 0.3], [0.3, 0.1, -1e-9]], max_iter=3, **KW)
    assert (r["n_iters"], r["success"], r["gl"]) == (3, 1, -1e-9)
    # never below zero (zero itself is not below)
    r = R.replay(philox, audio, [[0.3, 0.2, 0.3], [0.3, 0.0, 0.3], [0.3, 0.1, 0.0]], max_iter=3, **KW)
    assert (r["n_iters"], r["success"], r["gl"]) == (3, -1, 0.0) and r["trace"][-1, 1] == 1.0
    # in the middle
    r = R.replay(philox, audio, [[0.3, 0.2, 0.3], [-0.5, 0.0, 0.3], [9, 9, 9]], max_iter=3, **KW)
    assert (r["n_iters"], r["success"]) == (2, 1) and r["trace"][-1, 1] == 0.0


def test_the_global_best_never_rises(philox, audio):
    losses = np.random.RandomState(8).uniform(0.1, 1.0, (12, 3))
    r = R.replay(philox, audio, losses, max_iter=12, **KW)
    gl = r["trace"][:, 0]
    assert r["n_iters"] == 12 and np.all(np.diff(gl) <= 0) and gl[-1] == losses.min()
    assert np.array_equal(gl, np.minimum.accumulate(losses.min(axis=1)))


# ------------------------------------------------------------------------------------------------ the ball and the clamp
@pytest.mark.parametrize("v_max", [0.0005, 0.01])              # below and above the ball's diameter 2 eps
def test_positions_stay_in_the_ball_and_velocities_in_the_clamp(philox, v_max):
    eps, P = 0.002, 4
    a = np.array([1.0, -1.0, 1.0 - 0.001, -1.0 + 0.0015, 0.999, 0.0, -0.25, 0.3, 1.0 - 0.002])
    lo, hi = R.ball(a, eps)
    assert hi[0] == 1.0 and lo[1] == -1.0 and hi[2] == 1.0 and lo[3] == -1.0 and np.all(hi - lo <= 2 * eps + 1e-15)
    x, v, q = R.init(philox, a, eps, P, v_max, SEED, STREAM)
    assert np.array_equal(x[0], a) and not v[0].any() and np.array_equal(q, R.cast_i16(x))
    pb, gb = x.copy(), x[1].copy()
    rng = np.random.RandomState(2)
    for t in range(1, 9):
        assert np.all(x >= lo) and np.all(x <= hi) and np.all(np.abs(v) <= v_max)
        imp = rng.rand(P) < 0.5
        x, v, pb, gb, q = R.step(philox, a, eps, x, v, pb, gb, imp, int(rng.randint(-1, P)), 0.9, 1.5, 1.5, v_max, SEED, STREAM, t)
        assert np.all(pb >= lo) and np.all(pb <= hi) and np.all(gb >= lo) and np.all(gb <= hi)
    assert np.all(x >= lo) and np.all(x <= hi) and np.all(np.abs(v) <= v_max)
    assert np.abs(v).max() > 0.5 * min(v_max, 2 * eps)         # the swarm does move


# ------------------------------------------------------------------------------------------------ ParticleSwarm
class _Engine(object):
    """what ParticleSwarm asks of an engine, with canned answers"""

    def __init__(self, S, rows=3, P=4):
        self.S, self.rows, self.P, self.calls = S, rows, P, []

    def attack_pso(self, p, q, audio):
        self.calls.append(("pso", p.stream, p.seed, p.max_iter, p.epsilon, p.threshold, p.target, q.particles, q.v_max, q.w_init,
                           q.w_end, q.c1, q.c2, p.bits_per_sample))
        trace = np.arange(self.rows * (3 + self.S), dtype=np.float64).reshape(self.rows, 3 + self.S)
        return np.arange(audio.size).astype(np.int16), -1, audio.copy(), trace, np.zeros((self.rows, self.P))

    def attack_iter_seconds(self, n):
        return 0.25 * np.arange(1, n + 1)

    def estimate_threshold(self, p, model_threshold, audio, noise_all=None, max_total_iters=0):
        self.calls.append(("estimate", p.stream, p.seed, p.attack_type))
        return 1.5, 7, 2, 1.75, audio


class _Model(object):
    def __init__(self, task, S):
        self.task, self.threshold, self.engine = task, 0.5, _Engine(S)


def test_particle_swarm_checks_its_arguments():
    m = _Model("OSI", 3)
    ps = ParticleSwarm("OSI", "targeted", m, epsilon=0.004, seed=3, verbose=False)
    assert ps.v_max == 0.004 and ps.n_particles == 25 and ps.max_iter == 300           # v_max=None means epsilon
    assert ParticleSwarm("OSI", "targeted", m, v_max=0.001, verbose=False).v_max == 0.001
    with pytest.raises(ValueError, match="foreign"):
        ParticleSwarm("OSI", "targeted", DS.StubModel("OSI"))                           # score / make_decisions, no engine
    with pytest.raises(ValueError):
        ParticleSwarm("SV", "targeted", m)                                              # the model's task is OSI
    bad = [dict(n_particles=1), dict(n_particles=65), dict(max_iter=0), dict(epsilon=0.0), dict(epsilon=float("inf")),
           dict(v_max=0.0), dict(v_max=-1.0), dict(v_max=float("nan")), dict(w_init=-0.1), dict(w_end=float("nan")),
           dict(c1=-1.0), dict(c2=float("inf"))]
    for kw in bad:
        with pytest.raises(ValueError):
            ParticleSwarm("OSI", "targeted", m, **kw)
    with pytest.raises(ValueError):
        ParticleSwarm("XYZ", "targeted", m)
    for ok in (dict(n_particles=2), dict(n_particles=64), dict(w_init=0.0, w_end=0.0, c1=0.0, c2=0.0), dict(max_iter=1)):
        ParticleSwarm("OSI", "targeted", m, verbose=False, **ok)


@pytest.mark.parametrize("task,S", [("OSI", 3), ("SV", 1)])
def test_particle_swarm_attack_marshals_and_writes_its_checkpoint(tmp_path, task, S):
    m = _Model(task, S)
    ps = ParticleSwarm(task, "targeted", m, epsilon=0.003, max_iter=9, n_particles=4, w_init=0.8, w_end=0.2, c1=1.0, c2=2.0,
                       seed=11, verbose=False)
    audio = np.linspace(-0.5, 0.5, 40)
    cp = str(tmp_path / "a.cp")
    adv, flag = ps.attack(audio, cp, threshold=0.25, target=2 if task == "OSI" else None, bits_per_sample=12)
    assert adv.dtype == np.int16 and adv.shape == (40, 1) and flag == -1
    assert m.engine.calls == [("pso", 0, 11, 9, 0.003, 0.25, 2 if task == "OSI" else 0, 4, 0.003, 0.8, 0.2, 1.0, 2.0, 12)]
    adv2, _ = ps.attack(audio[:, None], None)                                            # a column, no checkpoint
    assert adv2.shape == (40, 1) and m.engine.calls[-1][1] == 1                          # the next stream, as FakeBob counts
    with open(cp, "rb") as r:
        rows = pickle.load(r)
    assert len(rows) == 3
    for k, row in enumerate(rows):
        assert len(row) == 3                                                             # no distance column
        assert isinstance(row[0], np.ndarray) and row[0].shape == (1,) and row[0][0] == k * (3 + S)
        if task == "SV":
            assert np.ndim(row[1]) == 0 and row[1] == k * (3 + S) + 3
        else:
            assert row[1].shape == (S,) and row[1][0] == k * (3 + S) + 3
        assert row[2] == 0.25 * (k + 1)
    with pytest.raises(ValueError):
        ps.attack(audio, None, bits_per_sample=17)


def test_particle_swarm_borrows_fakebobs_threshold_sweep(monkeypatch):
    monkeypatch.delenv("FB_EOT_SIZE", raising=False)
    m = _Model("OSI", 3)
    ps = ParticleSwarm("OSI", "targeted", m, seed=11, verbose=False)
    ps._stream = 4
    assert ps.estimate_threshold(np.zeros(40))[:2] == (1.5, 7)
    assert m.engine.calls == [("estimate", 4, 11, 0)]                                    # this attack's seed and stream, untargeted
    assert ps.threshold == 1.75 and ps._stream == 5
    assert "no threshold sweep of its own" in ParticleSwarm.estimate_threshold.__doc__
    csi = ParticleSwarm("CSI", "targeted", _Model("CSI", 3), verbose=False)
    with contextlib.redirect_stdout(io.StringIO()):
        assert csi.estimate_threshold(np.zeros(40)) is None


# ------------------------------------------------------------------------------------------------ attack_main
@pytest.fixture()
def site(tmp_path):
    DS.make_site(str(tmp_path))
    old = os.getcwd()
    os.chdir(str(tmp_path))
    yield str(tmp_path)
    os.chdir(old)


def _main(extra, built=None):
    seen = []

    def bob(task, at, model, **hp):
        seen.append(hp)
        return DS.StubBob(task, at, model, **hp)

    def model(archi, t, ml, pre, th, gid):
        if built is not None:
            built.append(gid)
        return DS.StubModel(t, th)
    DS.StubBob.log = []
    argv = ["-spk_id"] + DS.SPK_IDS + ["-task", "OSI", "-type", "targeted", "--streams", "1", "--seed", "5"] + extra
    with contextlib.redirect_stdout(io.StringIO()), contextlib.redirect_stderr(io.StringIO()):
        res = AM.main(argv, model_factory=model, bob_factory=bob)
    return res, seen


def test_attack_main_hands_the_swarm_its_options(site):
    (g, results, _thr), seen = _main(["--attack", "pso", "--particles", "7", "--pso-w", "0.8:0.2", "--pso-c", "1:2.5", "--pso-vmax",
                                      "0.001", "-epsilon", "0.004", "-max_iter", "40", "-adver", "0.5", "--eot-size", "1"])
    assert seen == [dict(adver_thresh=0.5, epsilon=0.004, max_iter=40, n_particles=7, w_init=0.8, w_end=0.2, c1=1.0, c2=2.5,
                         v_max=0.001)]
    assert g[1] == len(results) > 0
    _res, seen = _main(["--attack", "pso"])
    assert seen[0]["n_particles"] == 25 and seen[0]["v_max"] is None and (seen[0]["w_init"], seen[0]["w_end"]) == (0.9, 0.1)
    assert (seen[0]["c1"], seen[0]["c2"]) == (1.4961, 1.4961) and "samples_per_draw" not in seen[0]
    for extra in ([], ["--attack", "nes"]):                                  # the default: nothing changes
        _res, seen = _main(extra)
        assert sorted(seen[0]) == sorted(["adver_thresh", "epsilon", "max_iter", "max_lr", "min_lr", "samples_per_draw", "sigma",
                                          "momentum", "plateau_length", "plateau_drop"])


@pytest.mark.parametrize("extra", [["--eot-size", "2"], ["--companions", "1"], ["--pso-w", "0.9"], ["--pso-c", "a:b"],
                                   ["--particles", "x"]])
def test_attack_main_refuses_before_any_model_is_built(site, extra):
    built = []
    with pytest.raises(SystemExit):
        _main(["--attack", "pso"] + extra, built)
    assert built == []
    with pytest.raises(SystemExit):
        _main(["--attack", "swarm"], built)
    assert built == []
