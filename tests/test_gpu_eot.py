"""Expectation over transformation (fb_set_eot; include/fakebob_hip.h): the replication and the averaged loss on a
deterministic victim, where they must change nothing; reproducibility of attacks on a randomised victim; the refusals; and
fb_get_grad's averaged scores and loss against the numpy mean of per-replica scoring calls."""
import ctypes

import numpy as np
import pytest

from fakebob_amd import _native, input_transform as T
from fakebob_amd._native import FB_E_ARG, FB_E_STATE, NativeError
from fakebob_amd.engine import Engine, nes_params
from fakebob_amd.models import synthetic_audio, synthetic_gmm_system, synthetic_ivector_system
from tests.input_transform_noise_ref import NOISE, eot_mean, ref_noisy
from tests.test_gpu_input_transform import SCORE_TOL   # the bound between an NES batch's column 0 and a scoring call

pytestmark = pytest.mark.gpu
N = 16000
SPD = 6


def _audio(utt=9):
    return synthetic_audio(utt, N)


def _cast(x):
    return (np.asarray(x, np.float64) * 32768.0).astype(np.int64).astype(np.int16)


def _gmm(system, task):
    ubm, spk = system
    e = Engine(0)
    if task == "CSI":
        e.load_gmm(spk)
        e.set_system("CSI", np.array([-80.0, -75.0, -90.0]), np.array([3.0, 2.0, 4.0]))
    elif task == "SV":
        e.load_gmm([ubm, spk[0]])
        e.set_system("SV")
    else:
        e.load_gmm([ubm] + spk)
        e.set_system("OSI")
    return e


def _iv_sv():
    sy = synthetic_ivector_system(C=96, D=72, R=48, L=24, n_speakers=1, seed=11)
    sy = sy.with_enrolled(sy.enrolled, [-40.0], [10.0])
    e = Engine(0)
    e.load_ivector(sy, "SV")
    return e


def _run(e, p, audio):
    adv, flag, adv_f, trace = e.attack(p, audio)
    rows = trace.shape[0]
    assert e.attack_iter_seconds(rows).shape == (rows,)
    with pytest.raises(NativeError):
        e.attack_iter_seconds(rows + 1)
    return adv, flag, adv_f, trace


def _same(a, b):
    return a[1] == b[1] and np.array_equal(a[0], b[0]) and np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])


CASES = {
    "gmm OSI targeted": ("OSI", "targeted", dict(target=1, threshold=1e3)),
    "gmm OSI untargeted": ("OSI", "untargeted", dict(threshold=1e3)),
    "gmm CSI": ("CSI", "targeted", dict(target=2, adver_thresh=1e3)),   # (no early stop: six iterations)
    "gmm SV": ("SV", "targeted", dict(threshold=1e3)),
    "ivector SV": ("SV", "targeted", dict(threshold=1e3)),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_eot_on_a_deterministic_victim_changes_nothing(small_system, monkeypatch, name):
    """ms:3, dither 0: every replica is the same utterance, the mean of 2 or 4 equal values is exact, and the attack is the
    r = 1 attack on the unfused chain bit for bit."""
    monkeypatch.delenv("FB_NO_FUSE", raising=False)
    task, kind, kw = CASES[name]
    e = _iv_sv() if name.startswith("ivector") else _gmm(small_system, task)
    try:
        e.set_input_transform("ms:3")
        p = nes_params(task, kind, samples_per_draw=SPD, max_iter=6, epsilon=0.002, seed=5, stream=1, **kw)
        audio = _audio()
        e.set_fused_chain(False)
        base = _run(e, p, audio)
        assert base[3].shape[0] == 6 and np.all(np.isfinite(base[3]))
        e.set_fused_chain(None)
        for r in (2, 4):
            e.set_eot(r)
            assert _same(base, _run(e, p, audio)), r
        e.set_eot(1)                                   # back on the fused chain: the same trajectory again
        e.set_fused_chain(True)
        assert _same(base, _run(e, p, audio))
    finally:
        e.close()


def _attack_once(system, chain, dither, r, stream=2, batch=None, warm=False, monkeypatch=None):
    if batch is not None:
        monkeypatch.setenv("FB_ATTACK_BATCH", str(batch))
    e = _gmm(system, "OSI")
    try:
        if dither:
            e.set_frontend(dither=dither)
        e.set_input_transform(chain)
        e.set_eot(r)
        kw = dict(samples_per_draw=SPD, max_iter=5, target=1, epsilon=0.002, threshold=1e3, seed=5)
        if warm:
            e.attack(nes_params("OSI", "targeted", stream=9, **kw), _audio(3))
        return e.attack(nes_params("OSI", "targeted", stream=stream, **kw), _audio())
    finally:
        e.close()
        if batch is not None:
            monkeypatch.delenv("FB_ATTACK_BATCH")


@pytest.mark.parametrize("victim", ["at:20", "dither 1"])
def test_an_eot_attack_depends_on_seed_and_stream_only(small_system, monkeypatch, victim):
    monkeypatch.delenv("FB_ATTACK_BATCH", raising=False)
    chain, dither = ("at:20", 0.0) if victim == "at:20" else (None, 1.0)
    a = _attack_once(small_system, chain, dither, 3)
    assert a[3].shape[0] == 5 and np.all(np.isfinite(a[3]))
    assert _same(a, _attack_once(small_system, chain, dither, 3))                                  # a fresh engine
    assert _same(a, _attack_once(small_system, chain, dither, 3, batch=1, monkeypatch=monkeypatch))
    assert _same(a, _attack_once(small_system, chain, dither, 3, batch=4, monkeypatch=monkeypatch))
    assert _same(a, _attack_once(small_system, chain, dither, 3, warm=True))                       # after another attack
    assert not np.array_equal(a[3], _attack_once(small_system, chain, dither, 3, stream=3)[3])     # another stream differs
    assert not np.array_equal(a[3], _attack_once(small_system, chain, dither, 1)[3])               # and r matters here


def test_refusals(small_system):
    e = _gmm(small_system, "OSI")
    try:
        e.set_input_transform("at:20")
        e.set_eot(3)
        p = nes_params("OSI", "targeted", samples_per_draw=SPD, max_iter=3, target=1, threshold=1e3, seed=5, stream=1)
        want = e.attack(p, _audio())
        for bad in (0, 33, -1):
            with pytest.raises(NativeError) as ex:       # the library's own refusal, past the wrapper's
                _native.check(e._L.fb_set_eot(e._h, ctypes.c_int(bad)))
            assert ex.value.code == FB_E_ARG
            with pytest.raises(ValueError):
                e.set_eot(bad)
        assert _same(want, e.attack(p, _audio()))                    # the previous size was kept
        with pytest.raises(NativeError) as ex:
            e.estimate_threshold(nes_params("OSI", "untargeted", samples_per_draw=SPD, seed=1), 1e3, _audio(), max_total_iters=3)
        assert ex.value.code == FB_E_STATE
    finally:
        e.close()


def test_foreign_models_are_unaffected():
    audio = _audio()
    p = nes_params("OSI", "targeted", samples_per_draw=SPD, max_iter=4, target=1, threshold=1e3, seed=5, stream=1)
    calls = []

    def score(a):       # (N, B) -> (B, 3)
        calls.append(a.shape[1])
        m = np.stack([a[:200].sum(axis=0), a[200:400].sum(axis=0), a[400:600].sum(axis=0)], axis=1)
        return m
    x = Engine(0)
    try:
        base = x.attack_ext(p, 3, score, audio)
        g_base = x.get_grad_ext(p, 3, score, audio)
        x.set_eot(4)
        calls.clear()
        assert _same(base, x.attack_ext(p, 3, score, audio))
        assert set(calls) == {SPD + 1}                               # the batch is not replicated
        g = x.get_grad_ext(p, 3, score, audio)
        assert all(np.array_equal(u, v) for u, v in zip(g, g_base))
    finally:
        x.close()


def test_device_models_are_unaffected():
    torch = _native.torch_first()
    audio = _audio()
    p = nes_params("SV", "targeted", samples_per_draw=SPD, max_iter=4, threshold=1e3, seed=5, stream=1)
    B = SPD + 1
    e = Engine(0)
    try:
        dev = torch.device("cuda", 0)
        x = torch.zeros((B, N), dtype=torch.float64, device=dev)
        sc = torch.zeros((B, 1), dtype=torch.float64, device=dev)

        def model(xb):      # [B, N] on the device -> [B, 1]
            return xb[:, :500].sum(dim=1, keepdim=True)
        base = e.attack_dev(p, 1, model, x, sc, audio)
        e.set_eot(4)
        assert _same(base, e.attack_dev(p, 1, model, x, sc, audio))
    finally:
        e.close()


@pytest.mark.parametrize("task", ["SV", "OSI"])
def test_get_grad_averages_over_the_replicas(small_system, task):
    """r = 3, at:20: score0 and adver_loss against the numpy mean (the contract's order) of per-replica system scores and
    losses from scoring the restatement's replicas of the cast clean audio on a chain-less engine.  An NES batch's row and a
    scoring call of the same utterance agree to SCORE_TOL (tests/test_gpu_properties.py); the mean of r such rows keeps that
    bound, and the loss is a difference of two of them: 2 * SCORE_TOL."""
    r, it, seed, stream = 3, 4, 11, 6
    chain = T.parse("at:20")
    audio = _audio()
    d, c = _gmm(small_system, task), _gmm(small_system, task)
    try:
        d.set_input_transform(chain)
        d.set_eot(r)
        thr, adv_thr = 0.1, 0.05
        kw = dict(target=1) if task == "OSI" else {}
        p = nes_params(task, "targeted", samples_per_draw=SPD, threshold=thr, adver_thresh=adv_thr, seed=seed, stream=stream, **kw)
        fl, _g, al, sc0 = d.get_grad(p, audio, it=it)
        w = _cast(audio)
        reps = []
        for j in range(r):
            normals = {s: d.debug_tf_noise(seed, stream, it, 0, j, s, 0, w.size) for s, st in enumerate(chain) if st.kind == NOISE}
            reps.append(ref_noisy(w, chain, normals))
        dbg = d.debug_input_transform_eot([w], r, seed, stream, it)[0]
        assert all(np.array_equal(a, b) for a, b in zip(dbg, reps))
        raw, _ = c.score_raw(reps)
        sc = raw[:, 1:] - raw[:, 0:1]                                # OSI / SV: model 0 is the UBM
        if task == "SV":
            losses = (thr + adv_thr) - sc[:, 0]
        else:
            others = np.delete(sc, 1, axis=1).max(axis=1)
            losses = (np.maximum(others, thr) + adv_thr) - sc[:, 1]
        want_sc = eot_mean(sc.T)
        want_al = float(eot_mean(losses))
    finally:
        d.close()
        c.close()
    S = want_sc.size
    print("score0 %.3g adver_loss %.3g" % (np.abs(sc0[:S] - want_sc).max(), abs(al - want_al)))
    assert np.abs(sc0[:S] - want_sc).max() <= 2 * SCORE_TOL
    assert abs(al - want_al) <= 2 * SCORE_TOL
    assert np.isfinite(fl)
    assert np.ptp(losses) > 10 * SCORE_TOL                          # the replicas do differ: the mean is not a formality
