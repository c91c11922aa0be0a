"""Companion utterances (fb_set_companions; include/fakebob_hip.h): the composing launch against the numpy restatement to
the bit, the two identities (no companions: the parent's attack; one companion equal to a_0: the single-utterance attack),
the averaged loss and scores of fb_get_grad against per-row scoring calls, reproducibility under a randomised victim, the
effect of a universal perturbation judged per utterance, the refusals and the paths companions must leave alone."""
import ctypes

import numpy as np
import pytest

from fakebob_amd import _native, companions as CP, input_transform as T
from fakebob_amd._native import FB_E_ARG, FB_E_STATE, NativeError
from fakebob_amd.engine import Engine, nes_params
from fakebob_amd.models import synthetic_audio
from tests import companions_ref as R
from tests.test_gpu_eot import _gmm, _iv_sv, _same
from tests.test_gpu_input_transform import SCORE_TOL   # the bound between an NES batch's row and a scoring call

pytestmark = pytest.mark.gpu
_native.torch_first()   # torch ahead of the library (one HIP runtime for both): the device-model case, also when this file runs alone
N = 4000
SPD = 4          # B = 5 rows per NES batch


def _audio(utt=9, n=N):
    return synthetic_audio(utt, n)


def _companions(n=N, count=2):
    return [CP.cast_i16(_audio(20 + u, n)) for u in range(count)]


# ------------------------------------------------------------------------------------------------ bits of the kernel
def _hand_made(n, K1):
    """a0, B = 5 NES rows around it and K1 companions, with samples forced to the rails -- at both utterance ends and inside --
    so that the clip acts on either side: a companion at 32767 under a positive difference, at -32768 under a negative one"""
    rng = np.random.default_rng(n)
    a0 = CP.cast_i16(_audio(9, n))
    comp = np.stack(_companions(n, K1))
    q = np.clip(a0.astype(np.int32) + rng.integers(-70, 71, size=(5, n)), -32768, 32767).astype(np.int16)
    q[0] = a0                                           # row 0 of an NES batch: the unperturbed audio
    for p in (0, 1, 17, n // 2, n - 2, n - 1):
        comp[0, p], comp[-1, p] = 32767, -32768
        a0[p] = 0
        q[1:, p] = (40, -40, 65, -65)                   # the difference: positive for rows 1 and 3, negative for 2 and 4
    q[3, 5], a0[5] = 32767, -32768                      # the largest difference, +65535 ...
    q[4, 6], a0[6] = -32768, 32767                      # ... and -65535
    return q, a0, comp


CHAINS = {"empty": (None, 1), "ms:7,qt:512": ("ms:7,qt:512", 1), "fir31": ("lpf:3000:31", 1), "noise:20 r=2": ("noise:20", 2),
          "at:20 r=2": ("at:20", 2)}


# (8200 samples: three tiles, a halo across a tile seam -- with one chain that has a radius and one randomised chain)
BIT_CASES = [(name, n) for name in CHAINS for n in (4000, 4001)] + [("ms:7,qt:512", 8200), ("at:20 r=2", 8200)]


@pytest.mark.parametrize("name,n", BIT_CASES)
def test_the_composing_launch_to_the_bit(name, n):
    spec, r = CHAINS[name]
    seed, stream, epoch = 11, 6, 3
    q, a0, comp = _hand_made(n, 2)
    chain = T.parse(spec)
    e = Engine(0)
    try:
        e.set_input_transform(chain)
        e.set_eot(5)                                   # (the hook takes r from its argument, not from the engine)
        e.set_companions(comp)
        got = e.debug_compose(q, a0, r, seed, stream, epoch)
        want = R.compose(q, a0, comp, chain, r, lambda b, rho, s: e.debug_tf_noise(seed, stream, epoch, b, rho, s, 0, n))
        e.set_companions(None)                         # K = 1: the chain over q, replicated
        alone = e.debug_compose(q, a0, r, seed, stream, epoch)
    finally:
        e.close()
    assert got.shape == (5, 3, r, n)
    assert np.array_equal(got, want)
    assert np.array_equal(alone[:, 0], want[:, 0])
    rails = R.compose_row(q[3], a0, comp)
    assert rails[1, 0] == 32767 and rails[2, 0] == -32768 + 65 and rails[1, 5] == 32767     # the clip did act
    if r > 1:                                          # the replica index u * r + j and the per-row power both show
        flat = got.reshape(5, 3 * r, n)
        assert all(not np.array_equal(flat[1, i], flat[1, j]) for i in range(3 * r) for j in range(i))


# ------------------------------------------------------------------------------------------------ the identities
def _run(e, p, audio):
    return e.attack(p, audio)


@pytest.mark.parametrize("kind", ["gmm", "ivector"])
def test_without_companions_nothing_changes(small_system, monkeypatch, kind):
    """never set, or set and cleared again: the attack of an engine that never saw the call, on the default (fused) chain"""
    monkeypatch.delenv("FB_NO_FUSE", raising=False)
    task, kw = ("OSI", dict(target=1)) if kind == "gmm" else ("SV", {})
    p = nes_params(task, "targeted", samples_per_draw=SPD, max_iter=6, epsilon=0.002, threshold=1e3, seed=5, stream=1, **kw)
    audio = _audio()
    mk = (lambda: _gmm(small_system, "OSI")) if kind == "gmm" else _iv_sv
    a, b = mk(), mk()
    try:
        base = _run(a, p, audio)
        assert base[3].shape[0] == 6 and np.all(np.isfinite(base[3]))
        b.set_companions(_companions())
        with_c = _run(b, p, audio)
        assert with_c[3].shape[0] == 6 and not np.array_equal(with_c[3], base[3])      # (they do act while set)
        b.set_companions(None)
        assert _same(base, _run(b, p, audio))
        b.set_companions(_companions(count=1))
        _native.check(b._L.fb_set_companions(b._h, None, ctypes.c_int(0), ctypes.c_int64(0)))
        assert _same(base, _run(b, p, audio))
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("kind", ["gmm", "ivector"])
def test_a_companion_equal_to_a0_is_the_single_utterance_attack(small_system, monkeypatch, kind):
    """K = 2, the companion = a_0, a deterministic victim (ms:3): every composed row is q_b, (l + l) / 2 == l exactly, and
    the attack is the fb_set_eot(1) attack on the unfused chain bit for bit.  (K = 2 only: three equal terms do not sum
    exactly.)"""
    monkeypatch.delenv("FB_NO_FUSE", raising=False)
    task, kw = ("OSI", dict(target=1)) if kind == "gmm" else ("SV", {})
    p = nes_params(task, "targeted", samples_per_draw=SPD, max_iter=6, epsilon=0.002, threshold=1e3, seed=5, stream=1, **kw)
    audio = _audio()
    e = _gmm(small_system, "OSI") if kind == "gmm" else _iv_sv()
    try:
        e.set_input_transform("ms:3")
        e.set_eot(1)
        e.set_fused_chain(False)
        base = _run(e, p, audio)
        assert base[3].shape[0] == 6 and np.all(np.isfinite(base[3]))
        e.set_fused_chain(None)
        e.set_companions([CP.cast_i16(audio)])
        q = np.stack([CP.cast_i16(audio), CP.cast_i16(audio) + np.int16(3)])
        rows = e.debug_compose(q, CP.cast_i16(audio), 1, 5, 1, 0)
        assert np.array_equal(rows[:, 1], rows[:, 0])                  # every composed row equals q_b (through the chain)
        assert _same(base, _run(e, p, audio))
    finally:
        e.close()


# ------------------------------------------------------------------------------------------------ averaging
@pytest.mark.parametrize("kind", ["gmm OSI", "ivector SV"])
def test_get_grad_averages_over_the_utterances(small_system, kind):
    """Two different companions, no chain.  Row 0 of the NES batch is a_0, so its K composed rows are a_0 and the companions
    themselves: scoring those three with ordinary scoring calls gives the per-row values, and loss[0] / score0 must be their
    mean in the contract's order.  An NES batch's row and a scoring call of the same utterance agree to SCORE_TOL
    (tests/test_gpu_properties.py) and the mean of K such rows keeps that bound; the OSI loss is a difference of two scores:
    2 * SCORE_TOL, as in tests/test_gpu_eot.py."""
    thr, adv_thr = 0.1, 0.05
    audio = _audio()
    comp = _companions()
    gmm = kind.startswith("gmm")
    mk = (lambda: _gmm(small_system, "OSI")) if gmm else _iv_sv
    d, c = mk(), mk()
    try:
        d.set_companions(comp)
        kw = dict(target=1) if gmm else {}
        p = nes_params("OSI" if gmm else "SV", "targeted", samples_per_draw=SPD, threshold=thr, adver_thresh=adv_thr, seed=11, stream=6, **kw)
        fl, _g, al, sc0 = d.get_grad(p, audio, it=4)
        rows = [CP.cast_i16(audio)] + comp
        assert np.array_equal(d.debug_compose(rows[0], rows[0], 1, 11, 6, 4)[0, :, 0], np.stack(rows))
        raw, tv = c.score_raw(rows)
        assert np.all(tv > 0)
        sc = c.system_scores(raw)                                        # [K][S]
        if gmm:
            losses = (np.maximum(np.delete(sc, 1, axis=1).max(axis=1), thr) + adv_thr) - sc[:, 1]
        else:
            losses = (thr + adv_thr) - sc[:, 0]
        want_sc = R.mean_over_replicas(sc.T)
        want_al = float(R.mean_over_replicas(losses))
        stats = d.stats()
    finally:
        d.close()
        c.close()
    S = want_sc.size
    print("score0 %.3g adver_loss %.3g" % (np.abs(sc0[:S] - want_sc).max(), abs(al - want_al)))
    assert np.abs(sc0[:S] - want_sc).max() <= SCORE_TOL
    assert abs(al - want_al) <= (2 if gmm else 1) * SCORE_TOL
    assert np.isfinite(fl)
    assert np.ptp(losses) > 10 * SCORE_TOL                               # the utterances do differ: the mean is not a formality
    assert stats["scored_utts"] == (SPD + 1) * 3                         # fb_stats counts what the front end scored


# ------------------------------------------------------------------------------------------------ reproducibility
def _attack_once(system, stream=2, warm=False, eot=2, comp=True):
    e = _gmm(system, "OSI")
    try:
        e.set_input_transform("at:20")
        e.set_eot(eot)
        if comp:
            e.set_companions(_companions())
        if warm:                                                         # an unrelated scoring call: the serial advances
            e.score_raw([CP.cast_i16(_audio(3))])
        p = nes_params("OSI", "targeted", samples_per_draw=SPD, max_iter=5, target=1, epsilon=0.002, threshold=1e3, seed=5, stream=stream)
        return e.attack(p, _audio())
    finally:
        e.close()


def test_an_attack_with_companions_depends_on_seed_and_stream_only(small_system):
    a = _attack_once(small_system)
    assert a[3].shape[0] == 5 and np.all(np.isfinite(a[3]))
    assert _same(a, _attack_once(small_system))                                          # a fresh engine
    assert _same(a, _attack_once(small_system, warm=True))                               # after an unrelated scoring call
    assert not np.array_equal(a[3], _attack_once(small_system, stream=3)[3])             # another stream differs
    assert not np.array_equal(a[3], _attack_once(small_system, eot=1)[3])                # and the draws matter
    assert not np.array_equal(a[3], _attack_once(small_system, comp=False)[3])           # as do the companions


# ------------------------------------------------------------------------------------------------ effect
def test_a_universal_perturbation_moves_every_utterance(small_system, tmp_path):
    """A targeted attack with two companions, judged through per_utterance against the companions left unperturbed: the mean
    loss ends lower than it started and the returned perturbation raises the target's score on each of the three utterances.
    (threshold 1e3: no early stop, loss = 1e3 - the target's mean score.)"""
    from fakebob_amd.attack import FakeBob
    from fakebob_amd.systems import gmm_OSI
    ubm, spk = small_system
    ml = [["spk%d" % i, "utt%d" % i, g, -60.0 - i, 2.0 + i] for i, g in enumerate(spk)]
    model = gmm_OSI(str(tmp_path / "osi"), ml, ubm, pre_model_dir=str(tmp_path), threshold=0.0)
    try:
        audio, comp = _audio(), _companions()
        clean = np.atleast_2d(model.score([CP.cast_i16(audio)] + comp))                  # [3][S]
        target = int(np.argmin(clean.mean(axis=0)))
        fb = FakeBob("OSI", "targeted", model, samples_per_draw=SPD, max_iter=60, epsilon=0.004, seed=5, verbose=False)
        cp = str(tmp_path / "t.cp")
        with pytest.raises(ValueError, match="lengths"):
            fb.attack(audio, None, threshold=1e3, target=target, companions=[comp[0], comp[1][:-1]])
        res = fb.attack(audio, cp, threshold=1e3, target=target, companions=comp)
        adv, flag = res
        assert model.engine.companions is None                                           # for that call only
        import pickle
        with open(cp, "rb") as r:
            trace = pickle.load(r)
        assert len(trace) == 60 and trace[-1][1][0] < trace[0][1][0]                     # the mean loss went down
        assert np.array_equal(res.perturbation_i16, adv[:, 0].astype(np.int32) - CP.cast_i16(audio))
        assert np.abs(res.perturbation_i16).max() <= 0.004 * 32768 + 1
        per = res.per_utterance
        assert [d["utterance"] for d in per] == [0, 1, 2] and np.array_equal(per[0]["audio_i16"], adv[:, 0])
        moved = res.apply_perturbation(comp)
        for u in (1, 2):
            assert np.array_equal(per[u]["audio_i16"], moved[u - 1])
            assert np.array_equal(per[u]["audio_i16"], R.compose_row(adv[:, 0], CP.cast_i16(audio), np.stack(comp))[u])
        gain = [float(np.ravel(per[u]["score"])[target] - clean[u, target]) for u in range(3)]
        print("target %d: score gain per utterance %s, mean loss %.4f -> %.4f" % (target, gain, trace[0][1][0], trace[-1][1][0]))
        assert all(g > 0 for g in gain)
        assert all(d["success"] == (int(d["decision"]) == target) for d in per)
    finally:
        model.engine.close()


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals(small_system):
    e = _gmm(small_system, "OSI")
    try:
        comp = np.stack(_companions())
        e.set_companions(comp)
        p = nes_params("OSI", "targeted", samples_per_draw=SPD, max_iter=3, target=1, threshold=1e3, seed=5, stream=1)
        want = e.attack(p, _audio())

        def raw_set(ptr, K1, n):
            return e._L.fb_set_companions(e._h, ptr, ctypes.c_int(K1), ctypes.c_int64(n))
        for fn in (lambda: e.attack(p, _audio(n=N + 1)), lambda: e.get_grad(p, _audio(n=N - 1))):     # wrong N
            with pytest.raises(NativeError) as ex:
                fn()
            assert ex.value.code == FB_E_ARG
        big = np.zeros((32, 8), np.int16)
        for args in ((_native.ptr(big), 32, 8), (_native.ptr(big), -1, 8), (None, 2, N), (_native.ptr(big), 2, 0)):
            with pytest.raises(NativeError) as ex:
                _native.check(raw_set(*args))
            assert ex.value.code == FB_E_ARG
        with pytest.raises(ValueError):
            e.set_companions([np.zeros(8, np.int16)] * 32)
        with pytest.raises(NativeError) as ex:                           # K * eot = 33 from fb_set_eot's side
            _native.check(e._L.fb_set_eot(e._h, ctypes.c_int(11)))
        assert ex.value.code == FB_E_ARG
        assert _same(want, e.attack(p, _audio()))                        # companions and eot as they were
        e.set_eot(10)                                                    # 3 * 10 = 30: allowed
        e.set_eot(1)
        e.set_companions(None)
        e.set_eot(11)                                                    # ... and from fb_set_companions' side
        with pytest.raises(NativeError) as ex:
            _native.check(raw_set(_native.ptr(comp), 2, N))
        assert ex.value.code == FB_E_ARG
        with pytest.raises(ValueError):
            e.set_companions(comp)
        assert e.companions is None
        e.set_eot(1)
        assert not _same(want, e.attack(p, _audio()))                    # still none set
        e.set_companions(comp)
        assert _same(want, e.attack(p, _audio()))
        with pytest.raises(NativeError) as ex:
            e.estimate_threshold(nes_params("OSI", "untargeted", samples_per_draw=SPD, seed=1), 1e3, _audio(), max_total_iters=3)
        assert ex.value.code == FB_E_STATE
    finally:
        e.close()


# ------------------------------------------------------------------------------------------------ non-effects
def test_scoring_and_foreign_models_are_unaffected(small_system):
    audio = _audio()
    p = nes_params("OSI", "targeted", samples_per_draw=SPD, max_iter=4, target=1, threshold=1e3, seed=5, stream=1)
    calls = []

    def score(a):       # (N, B) -> (B, 3)
        calls.append(a.shape[1])
        return np.stack([a[:200].sum(axis=0), a[200:400].sum(axis=0), a[400:600].sum(axis=0)], axis=1)
    x = _gmm(small_system, "OSI")
    try:
        base = x.attack_ext(p, 3, score, audio)
        g_base = x.get_grad_ext(p, 3, score, audio)
        raw_base = x.score_raw([CP.cast_i16(audio), CP.cast_i16(_audio(3, 2500))])
        x.set_companions(_companions())
        calls.clear()
        assert _same(base, x.attack_ext(p, 3, score, audio))
        assert set(calls) == {SPD + 1}                                   # the batch is not replicated
        g = x.get_grad_ext(p, 3, score, audio)
        assert all(np.array_equal(u, v) for u, v in zip(g, g_base))
        raw = x.score_raw([CP.cast_i16(audio), CP.cast_i16(_audio(3, 2500))])            # (another length is no refusal here)
        assert np.array_equal(raw[0], raw_base[0]) and np.array_equal(raw[1], raw_base[1])
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
        e.set_companions(_companions())
        assert _same(base, e.attack_dev(p, 1, model, x, sc, audio))
    finally:
        e.close()


def test_the_host_cast_is_the_devices(engine):
    x = np.concatenate([_audio(), [1.0, -1.0, 0.99999, 1.5, -1.5, 0.0]])
    for bits in (16, 8):
        assert np.array_equal(CP.cast_i16(x, bits), engine.debug_quantize(x, bits))
