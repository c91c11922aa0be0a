"""The particle-swarm attack on the device (fb_attack_pso; the "particle-swarm attack" section of include/fakebob_hip.h): the two
kernels against the numpy restatement (tests/pso_ref.py) bit for bit through the hooks, whole attacks replayed from the losses
they returned, attacks on randomised victims, the refusals, and ParticleSwarm on top.

Bit-exact checks use np.array_equal.  The one tolerance is the suite's bound between a row of an NES batch and a scoring call
of the same samples: SCORE_TOL of tests/test_gpu_input_transform.py for a score (SV's loss is one score), twice that for a loss
that is a difference of two scores (OSI, CSI), as tests/test_gpu_replicated_batches.py states it."""
import pickle

import numpy as np
import pytest

from fakebob_amd import _native, companions as CP
from fakebob_amd._native import FB_E_ARG, FB_E_STATE, NativeError
from fakebob_amd.attack import FakeBob
from fakebob_amd.engine import Engine, nes_params, pso_params
from fakebob_amd.models import synthetic_audio, synthetic_ivector_system
from fakebob_amd.pso import ParticleSwarm
from fakebob_amd.systems import gmm_CSI, gmm_OSI, iv_SV
from tests import pso_ref as R
from tests.test_gpu_input_transform import SCORE_TOL   # the bound between an NES batch's row and a scoring call

pytestmark = pytest.mark.gpu
SEED, STREAM = 0xC0FFEE1234567, 5                      # high bits set, stream != 0: both key words matter
EPS = 0.002
N = 4000                                               # the utterance length of tests/test_gpu_companions.py


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def philox(oracle):
    return oracle.philox


def _edge_audio(n, seed=3):
    """samples all over [-1, 1], with +-1.0 themselves and values within eps of them: the ball's clip is active"""
    a = np.random.RandomState(seed + n).uniform(-1.0, 1.0, n)
    edge = [1.0, -1.0, 1.0 - 0.5 * EPS, -1.0 + 0.25 * EPS, 1.0 - EPS, -1.0 + EPS, 0.0]
    for i, v in enumerate(edge[:n]):
        a[(i * 37) % n] = v
    return a


def _state(a, P, seed=1):
    """a swarm in mid-flight: positions, bests inside the ball, velocities inside the clamp"""
    rng = np.random.RandomState(seed)
    lo, hi = R.ball(a, EPS)
    inside = lambda: lo + rng.uniform(0, 1, (P, a.size)) * (hi - lo)   # noqa: E731
    return inside(), inside(), inside()[0]


def _same(got, want, names):
    for g, w, name in zip(got, want, names):
        assert g.dtype == w.dtype and g.shape == w.shape, name
        assert np.array_equal(g, w), (name, int(np.flatnonzero((g != w).ravel())[0]))


def _check_hooks(eng, philox, n, P, bits, v_max, improved, g_new, w=0.7, c1=1.4961, c2=1.25):
    a = _edge_audio(n)
    x, v, q = eng.debug_pso_init(a, EPS, P, v_max, SEED, STREAM, bits)
    _same((x, v, q), R.init(philox, a, EPS, P, v_max, SEED, STREAM, bits), ("x", "v", "q"))
    if bits == 16:
        assert np.array_equal(q, CP.cast_i16(x.reshape(-1), 16).reshape(P, n))
    x1, pb, gb = _state(a, P)
    got = eng.debug_pso_step(a, EPS, x1, v, pb, gb, improved, g_new, w, c1, c2, v_max, SEED, STREAM, 3, bits)
    want = R.step(philox, a, EPS, x1, v, pb, gb, improved, g_new, w, c1, c2, v_max, SEED, STREAM, 3, bits)
    _same(got, want, ("x'", "v'", "pb'", "gb'", "q'"))
    lo, hi = R.ball(a, EPS)
    assert np.all(got[0] >= lo) and np.all(got[0] <= hi) and np.all(np.abs(got[1]) <= v_max)
    return got


def _mixed(P):
    return (np.arange(P) % 3 != 1).astype(np.int32)


# ------------------------------------------------------------------------------------- 1. the kernels, bit for bit
@pytest.mark.parametrize("n", [1, 2, 5, 255, 256, 257, 1023, 4099])    # odd sizes, a lone last element, around a workgroup's 128
def test_hooks_at_every_length(eng, philox, n):
    _check_hooks(eng, philox, n, 3, 16, EPS, _mixed(3), 2)


@pytest.mark.parametrize("P", [2, 3, 25, 64])
@pytest.mark.parametrize("bits", [16, 8])
def test_hooks_at_every_swarm_size(eng, philox, P, bits):
    _check_hooks(eng, philox, 257 if P > 3 else 1023, P, bits, EPS, _mixed(P), P - 1)


@pytest.mark.parametrize("v_max", [0.0005, 0.01])                       # below and above the ball's diameter 2 eps
@pytest.mark.parametrize("improved", ["none", "all", "mixed"])
@pytest.mark.parametrize("g_new", [-1, 0, "last"])
def test_hooks_with_every_decision(eng, philox, v_max, improved, g_new):
    P, n = 5, 256
    imp = {"none": np.zeros(P, np.int32), "all": np.ones(P, np.int32), "mixed": _mixed(P)}[improved]
    g = P - 1 if g_new == "last" else g_new
    a = _edge_audio(n)
    x1, pb, gb = _state(a, P)
    got = _check_hooks(eng, philox, n, P, 16, v_max, imp, g)
    assert np.array_equal(got[3], gb if g < 0 else x1[g])                # gb: the old one, or x of g_new as it WAS
    for p in range(P):
        assert np.array_equal(got[2][p], x1[p] if imp[p] else pb[p])


def test_the_swarm_depends_on_both_key_words(eng):
    a = _edge_audio(64)
    base = eng.debug_pso_init(a, EPS, 3, EPS, SEED, STREAM)
    assert np.array_equal(base[0][0], a) and not base[1][0].any()        # particle 0: the audio at rest
    for seed, stream in ((SEED ^ (1 << 40), STREAM), (SEED ^ 1, STREAM), (SEED, STREAM + 1)):
        other = eng.debug_pso_init(a, EPS, 3, EPS, seed, stream)
        assert not np.array_equal(base[0][1:], other[0][1:]) and not np.array_equal(base[1][1:], other[1][1:])


# ------------------------------------------------------------------------------------- 2. whole attacks
PSO = dict(particles=8, w_init=0.9, w_end=0.1, c1=1.4961, c2=1.4961, v_max=EPS)
MAX_ITER = 12


def _models(small_system, d):
    ubm, spk = small_system
    return ubm, [["spk%d" % i, "utt%d" % i, g, -80.0 + 5.0 * i, 3.0 + 0.5 * i] for i, g in enumerate(spk)], str(d)


def _system(case, small_system, d, **kw):
    if case == "gmm OSI targeted":
        ubm, ml, d = _models(small_system, d)
        return gmm_OSI(d + "/osi", ml, ubm, pre_model_dir=d, threshold=0.0, **kw)
    if case == "gmm CSI untargeted":
        _ubm, ml, d = _models(small_system, d)
        return gmm_CSI(d + "/csi", ml, pre_model_dir=d, **kw)
    sy = synthetic_ivector_system(C=96, D=72, R=48, L=24, n_speakers=1, seed=11)
    return iv_SV(str(d) + "/sv", ["spk0", "utt0", sy.enrolled[0].copy(), -40.0, 10.0], pre_model_dir=str(d), threshold=0.0,
                 system=sy, **kw)


class _Scorer(object):
    """model.score for FakeBob.loss_fn: Engine.score_i16 + system_scores of int16 rows"""

    def __init__(self, eng, task):
        self.eng, self.task = eng, task

    def score(self, rows, **_kw):
        raw, tv = self.eng.score_raw(rows)
        assert np.all(tv > 0)
        sc = self.eng.system_scores(raw)
        return sc[:, 0] if self.task == "SV" else sc


# the settings were fixed on the CPU, with the restatement as the attack and the CPU oracle as the scorer: there the swarm's
# best loss falls by 0.08 (OSI), 0.2 (CSI) and 0.25 (i-vector SV) over 12 iterations, four orders above SCORE_TOL, and the OSI
# attack -- best loss 0.063 at iteration 0 with adver_thresh 0.045 -- crosses zero at iteration 10 (0.007 before, -0.004 there)
CASES = {
    "gmm OSI targeted": ("OSI", "targeted", dict(target=1, threshold=0.0, adver_thresh=0.045)),
    "gmm CSI untargeted": ("CSI", "untargeted", dict(adver_thresh=1e3)),   # (no stop: all twelve iterations)
    "ivector SV": ("SV", "targeted", dict(threshold=1e3)),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_a_whole_attack_is_its_replay(small_system, philox, tmp_path, case):
    """The returned losses drive the restatement; everything else the attack returned must come out of it bit for bit.  The
    best loss of the last iteration is strictly below that of iteration 0 (settings chosen on the CPU, see CASES)."""
    task, at, kw = CASES[case]
    model = _system(case, small_system, tmp_path)
    e = model.engine
    try:
        audio = synthetic_audio(9, N)
        if task == "CSI":
            kw = dict(kw, true=int(model.make_decisions(audio)[0]))
        p = nes_params(task, at, epsilon=EPS, max_iter=MAX_ITER, seed=5, stream=1, **kw)
        q = pso_params(**PSO)
        before = e.stats()
        adv, flag, adv_f, trace, losses = e.attack_pso(p, q, audio)
        after = e.stats()
        n = trace.shape[0]
        S = e.n_speakers
        assert losses.shape == (n, 8) and trace.shape == (n, 3 + S) and np.all(np.isfinite(trace)) and np.all(np.isfinite(losses))
        assert after["scored_utts"] - before["scored_utts"] == 8 * n and after["nes_iters"] == before["nes_iters"]
        secs = e.attack_iter_seconds(n)
        assert secs.shape == (n,) and np.all(secs > 0)
        with pytest.raises(NativeError):
            e.attack_iter_seconds(n + 1)
        keep = (0, n // 2, n - 1)
        r = R.replay(philox, audio, losses, eps=EPS, max_iter=MAX_ITER, P=8, w_init=PSO["w_init"], w_end=PSO["w_end"], c1=PSO["c1"],
                     c2=PSO["c2"], v_max=PSO["v_max"], seed=5, stream=1, keep=keep)
        assert (r["n_iters"], r["success"]) == (n, flag)
        assert np.array_equal(trace[:, :3], r["trace"])
        assert np.array_equal(adv_f, r["adv_f64"]) and np.array_equal(adv, r["adv_i16"])
        assert np.array_equal(adv, CP.cast_i16(adv_f, 16))
        # inside the ball, with no slack at all: the contract's ball is lo = fl(a - eps), hi = fl(a + eps), one rounding each
        # (FAKEBOB.py:163-164), and a sample on its edge IS that rounded value.  Its float64 distance from a can therefore
        # exceed eps by the rounding of the edge itself, at most half an ulp of a value below 1 (2^-53; 1.8e-18 was seen):
        # "max |adv_f64 - audio| <= eps" holds to the precision of the format and not beyond
        lo, hi = R.ball(audio, EPS)
        assert np.all(adv_f >= lo) and np.all(adv_f <= hi)
        print("  max |adv_f64 - audio| - eps = %.3g" % (np.abs(adv_f - audio).max() - EPS))
        assert np.abs(adv_f - audio).max() <= EPS + 2.0 ** -53
        gl = trace[:, 0]
        print("%s: %d iterations, flag %d, best loss %.6f -> %.6f" % (case, n, flag, gl[0], gl[-1]))
        assert np.all(np.diff(gl) <= 0) and gl[-1] < gl[0]
        assert flag == (1 if gl[-1] < 0 else -1) and (flag == 1 or n == MAX_ITER)
        # the positions of three iterations, scored by ordinary scoring calls
        fb = FakeBob(task, at, _Scorer(e, task), adver_thresh=kw.get("adver_thresh", 0.0), verbose=False)
        fb.threshold, fb.target, fb.true = kw.get("threshold", 0.0), kw.get("target"), kw.get("true")
        tol = SCORE_TOL if task == "SV" else 2 * SCORE_TOL
        for k in keep:
            rows = [CP.cast_i16(x, 16) for x in r["positions"][k]]
            want_l, want_sc = fb.loss_fn(rows)
            err = np.abs(want_l.reshape(-1) - losses[k]).max()
            print("  iteration %d: max |loss - scoring call| %.3g (bound %.3g)" % (k, err, tol))
            assert err <= tol
            g = int(trace[k, 1])
            if k == 0 or trace[k, 0] < trace[k - 1, 0]:                                        # gs was taken in this iteration
                assert np.abs(np.asarray(want_sc).reshape(8, -1)[g] - trace[k, 3:]).max() <= SCORE_TOL
        if case == "gmm OSI targeted":
            assert flag == 1 and 1 < n < MAX_ITER
        if flag == 1:
            model.threshold = kw.get("threshold", 0.0)
            dec, _sc = model.make_decisions(adv)
            assert int(dec) == (kw["target"] if task == "OSI" else 1)
    finally:
        e.close()


# ------------------------------------------------------------------------------------- 3. defended victims
def _defended(small_system, d, stream, **defence):
    model = _system("gmm OSI targeted", small_system, d, **defence)
    try:
        p = nes_params("OSI", "targeted", epsilon=EPS, max_iter=4, target=1, threshold=1e3, seed=5, stream=stream)
        return model.engine.attack_pso(p, pso_params(**dict(PSO, particles=4)), synthetic_audio(9, N))
    finally:
        model.engine.close()


@pytest.mark.parametrize("defence", [dict(input_transform="noise:30"), dict(feature_compression="0.5:4")], ids=["noise", "feco"])
def test_an_attack_on_a_randomised_victim_depends_on_seed_and_stream_only(small_system, tmp_path, defence):
    a = _defended(small_system, tmp_path, 2, **defence)
    b = _defended(small_system, tmp_path, 2, **defence)                # a fresh engine
    assert a[1] == b[1] and all(np.array_equal(x, y) for x, y in zip((a[0],) + a[2:], (b[0],) + b[2:]))
    c = _defended(small_system, tmp_path, 3, **defence)
    assert not np.array_equal(a[4], c[4])                              # another stream: other losses
    plain = _defended(small_system, tmp_path, 2)
    assert not np.array_equal(a[4], plain[4])                          # and the defence does act on the swarm's rows


# ------------------------------------------------------------------------------------- 4. refusals
def _code(fn):
    with pytest.raises(NativeError) as ex:
        fn()
    return ex.value.code


def test_refusals_leave_the_engine_usable(small_system, tmp_path):
    audio = synthetic_audio(9, N)
    bare = Engine(0)
    try:
        assert _code(lambda: bare.attack_pso(nes_params("OSI", "targeted", target=1, max_iter=2), pso_params(particles=4), audio)) == FB_E_STATE
    finally:
        bare.close()
    model = _system("gmm OSI targeted", small_system, tmp_path)
    e = model.engine
    try:
        nes = nes_params("OSI", "targeted", samples_per_draw=6, max_iter=3, target=1, threshold=1e3, seed=5, stream=1)
        want = e.attack(nes, audio)

        def unchanged():
            got = e.attack(nes, audio)
            return got[1] == want[1] and all(np.array_equal(x, y) for x, y in zip((got[0],) + got[2:], (want[0],) + want[2:]))
        good = dict(epsilon=EPS, max_iter=2, target=1, threshold=1e3, seed=5, stream=1)
        run = lambda pk, qk: e.attack_pso(nes_params("OSI", "targeted", **dict(good, **pk)), pso_params(**dict(dict(PSO, particles=4), **qk)), audio)   # noqa: E731
        nan, inf = float("nan"), float("inf")
        bad = [({}, dict(particles=1)), ({}, dict(particles=65)), ({}, dict(particles=0)), ({}, dict(w_init=-0.1)), ({}, dict(w_init=nan)),
               ({}, dict(w_end=-1.0)), ({}, dict(w_end=inf)), ({}, dict(c1=-1e-9)), ({}, dict(c1=nan)), ({}, dict(c2=-2.0)), ({}, dict(c2=inf)),
               ({}, dict(v_max=0.0)), ({}, dict(v_max=-EPS)), ({}, dict(v_max=inf)), ({}, dict(v_max=nan)),
               (dict(max_iter=0), {}), (dict(epsilon=0.0), {}), (dict(epsilon=-EPS), {}), (dict(epsilon=inf), {}), (dict(epsilon=nan), {}),
               (dict(target=3), {}), (dict(target=-1), {}), (dict(bits_per_sample=1), {}), (dict(bits_per_sample=17), {})]
        for pk, qk in bad:
            assert _code(lambda: run(pk, qk)) == FB_E_ARG, (pk, qk)
            assert unchanged(), (pk, qk)
        assert _code(lambda: e.attack_pso(nes_params("CSI", "untargeted", **dict(good, true=0)), pso_params(**PSO), audio)) == FB_E_ARG   # the task
        # the NES-only fields are neither read nor validated
        junk = dict(samples_per_draw=-7, sigma=-1.0, max_lr=nan, min_lr=nan, momentum=nan, plateau_length=-3, plateau_drop=0.0)
        ok = run({}, {})
        got = run(junk, {})
        assert got[1] == ok[1] and all(np.array_equal(x, y) for x, y in zip((got[0],) + got[2:], (ok[0],) + ok[2:]))
        e.set_eot(2)
        assert _code(lambda: run({}, {})) == FB_E_STATE
        e.set_eot(1)
        assert unchanged()
        e.set_companions([CP.cast_i16(synthetic_audio(3, N), 16)])
        assert _code(lambda: run({}, {})) == FB_E_STATE
        e.set_companions(None)
        assert unchanged()
        silent = np.zeros(N)
        assert _code(lambda: e.attack_pso(nes_params("OSI", "targeted", **good), pso_params(**PSO), silent)) == _native.FB_E_NO_VOICED
        assert unchanged()
        # the hooks refuse what the attack refuses
        a = np.zeros(8)
        for fn in (lambda: e.debug_pso_init(a, EPS, 1, EPS, 1, 1), lambda: e.debug_pso_init(a, EPS, 65, EPS, 1, 1),
                   lambda: e.debug_pso_init(a, 0.0, 3, EPS, 1, 1), lambda: e.debug_pso_init(a, EPS, 3, nan, 1, 1),
                   lambda: e.debug_pso_init(a, EPS, 3, EPS, 1, 1, 17),
                   lambda: e.debug_pso_step(a, EPS, np.zeros((3, 8)), np.zeros((3, 8)), np.zeros((3, 8)), a, [0, 0, 0], 3, 0.5, 1, 1, EPS, 1, 1, 1)):
            assert _code(fn) == FB_E_ARG
        assert unchanged()
    finally:
        e.close()


# ------------------------------------------------------------------------------------- 5. ParticleSwarm
def test_particle_swarm_attack_and_an_interleaved_fakebob(small_system, tmp_path):
    model = _system("gmm OSI targeted", small_system, tmp_path)
    try:
        audio = synthetic_audio(9, N)
        fb = FakeBob("OSI", "targeted", model, samples_per_draw=6, max_iter=4, seed=5, verbose=False)
        alone = fb.attack(audio, None, threshold=1e3, target=1)
        ps = ParticleSwarm("OSI", "targeted", model, adver_thresh=0.045, epsilon=EPS, max_iter=MAX_ITER, n_particles=8, seed=5, verbose=False)
        ps._stream = 1
        cp = str(tmp_path / "pso.cp")
        adv, flag = ps.attack(audio, cp, threshold=0.0, target=1)
        assert adv.dtype == np.int16 and adv.shape == (N, 1) and flag == 1 and ps._stream == 2
        p = nes_params("OSI", "targeted", adver_thresh=0.045, epsilon=EPS, max_iter=MAX_ITER, target=1, threshold=0.0, seed=5, stream=1)
        direct = model.engine.attack_pso(p, pso_params(**PSO), audio)                       # v_max=None meant epsilon
        assert np.array_equal(adv[:, 0], direct[0]) and flag == direct[1]
        with open(cp, "rb") as r:
            rows = pickle.load(r)
        assert len(rows) == direct[3].shape[0]
        for k, row in enumerate(rows):
            assert len(row) == 3 and row[0].shape == (1,) and row[0][0] == direct[3][k, 0]
            assert np.array_equal(row[1], direct[3][k, 3:]) and row[2] > 0
        fb._stream = 0
        again = fb.attack(audio, None, threshold=1e3, target=1)                              # FakeBob after PSO on the same engine
        assert again[1] == alone[1] and np.array_equal(again[0], alone[0])
        assert model.make_decisions(adv)[0] == 1
    finally:
        model.engine.close()
