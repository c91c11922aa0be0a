"""The play offset on the device (fb_set_play_offset; its contract is in include/fakebob_hip.h): k_play_compose and the
launches behind it against the numpy restatement (tests/play_offset_ref.py) to the bit, the identities (never set, set and
cleared: the parent's attack; a batch of a_0 rows: the host utterances), the averaged loss and scores against ordinary scoring
calls on numpy-composed rows, reproducibility under a randomised victim, the refusals, and the Python surface.
tests/test_play_offset_host.py shows on the restatement alone that the fixed cases draw distinct offsets and wraps inside a
workgroup's tile."""
import ctypes

import numpy as np
import pytest

from fakebob_amd import _native, air_channel as A, companions as CP, input_transform as T, play_offset as PO
from fakebob_amd._native import FB_E_ARG, FB_E_STATE, NativeError
from fakebob_amd.engine import Engine, cw2_params, hsj_params, kv_params, nes_params, pso_params, psy_params
from fakebob_amd.models import synthetic_audio
from tests import air_channel_ref as AR
from tests import codec_ref
from tests import companions_ref as CR
from tests import play_offset_ref as R
from tests.input_transform_noise_ref import NOISE, ref_noisy
from tests.play_offset_cases import ADPCM, AIR, BIT_CASES, POINT, ROWS
from tests.test_gpu_eot import _gmm, _iv_sv, _same
from tests.test_gpu_input_transform import SCORE_TOL   # the bound between an NES batch's row and a scoring call

pytestmark = pytest.mark.gpu
N = 4000
SPD = 4          # B = 5 rows per NES batch
ROOM64 = A.AirChannel(64, 8, 3000.0, 0.9, 0.99)


@pytest.fixture(scope="module")
def philox(oracle):
    return oracle.philox


def _audio(utt=9, n=N):
    return synthetic_audio(utt, n)


def _companions(n=N, count=2):
    return [CP.cast_i16(_audio(20 + u, n)) for u in range(count)]


# ------------------------------------------------------------------------------------------------ bits of the launch
def _hand_made(n, K1):
    """a0, ROWS NES rows around it and K1 companions, with samples forced to the rails -- at both utterance ends and inside --
    so that the clip acts on either side under every offset: a host at 32767 / -32768 meets differences of both signs, and the
    difference itself reaches +-65535"""
    rng = np.random.default_rng(7 * n + K1)
    a0 = CP.cast_i16(_audio(9, n))
    comp = np.stack(_companions(n, K1)) if K1 else np.zeros((0, n), np.int16)
    q = np.clip(a0.astype(np.int32) + rng.integers(-70, 71, size=(ROWS, n)), -32768, 32767).astype(np.int16)
    q[0] = a0                                           # row 0 of an NES batch: the unperturbed audio
    spots = (0, 1, 17, n // 2, n - 2, n - 1)
    for k, p in enumerate(spots):
        a0[p] = 32767 if k % 2 == 0 else -32768         # utterance 0's own host at a rail
        q[1:, p] = a0[p]
        if K1:
            comp[0, p], comp[-1, p] = 32767, -32768
    q[3, 5], a0[5] = 32767, -32768                      # the largest difference, +65535 ...
    q[4, 6], a0[6] = -32768, 32767                      # ... and -65535
    q[0] = a0
    return q, a0, comp


@pytest.mark.parametrize("stage,n,S,K,eot", BIT_CASES)
def test_the_composing_launch_to_the_bit(philox, stage, n, S, K, eot):
    seed, stream, epoch = POINT
    q, a0, comp = _hand_made(n, K - 1)
    front, _, codec = stage.partition("|") if "|" in stage else ((stage, "", "") if stage != ADPCM else ("empty", "", ADPCM))
    chain = T.parse(None if front in ("empty", AIR) else front)
    r = K * eot
    e = Engine(0)
    try:
        e.set_input_transform(chain)
        e.set_air_channel(ROOM64 if front == AIR else None)
        e.set_codec(codec or None)                      # (under an offset the hook returns the rows the front end reads)
        e.set_eot(3)                                   # (the hook takes the draws from its argument, not from the engine)
        e.set_companions(comp if K > 1 else None)
        e.set_play_offset(S)
        got = e.debug_compose(q, a0, eot, seed, stream, epoch)
        launches = e.debug_play_route()
        tau = e.debug_play_offsets(seed, stream, epoch, ROWS, r)
        want_tau = R.offsets(philox, seed, stream, epoch, ROWS, r, S)
        assert tau.dtype == np.uint32 and np.array_equal(tau, want_tau)
        rows = np.stack([R.compose_rows(q[b], a0, comp, eot, want_tau[b]) for b in range(ROWS)])     # [B][r][n]
        want = np.empty_like(rows)
        for b in range(ROWS):
            for rho in range(r):
                w = rows[b, rho]
                if front == AIR:
                    taps, z, wd = e.debug_air_taps(seed, stream, epoch, b, rho)
                    assert np.array_equal(taps, AR.taps(ROOM64.taps, ROOM64.predelay, ROOM64.amp, ROOM64.rho_lo, ROOM64.rho_hi, z, wd))
                    w = AR.convolve(w, taps)
                normals = {s: e.debug_tf_noise(seed, stream, epoch, b, rho, s, 0, n) for s, st in enumerate(chain) if st[0] == NOISE}
                w = ref_noisy(w, chain, normals)                  # (an SNR stage's E: the power of the composed, OFFSET row)
                want[b, rho] = codec_ref.adpcm(w) if codec else w
        e.set_play_offset(0)                           # cleared: the companions composition again (and the hook ignores the codec again)
        e.set_input_transform(None)
        e.set_air_channel(None)
        cleared = e.debug_compose(q, a0, 1, seed, stream, epoch)
    finally:
        e.close()
    assert got.shape == (ROWS, K, eot, n) and launches == 1
    assert np.array_equal(got.reshape(ROWS, r, n), want), (stage, n, S, K, eot)
    assert np.array_equal(cleared[:, :, 0], np.stack([CR.compose_row(q[b], a0, comp) for b in range(ROWS)]))
    if codec:
        assert not np.array_equal(want, rows)          # the codec did act
    if stage == "empty":
        assert np.array_equal(got[0], np.broadcast_to(np.concatenate([a0[None], comp])[:, None], (K, eot, n)))  # row 0: the hosts
        flat = rows.reshape(ROWS * r, n)
        assert (flat == 32767).any() and (flat == -32768).any()                    # the clip did act
        if S == n - 1 and r > 1:                       # ... and the offsets did: replicas of one utterance differ
            assert any(not np.array_equal(rows[1, 0], rows[1, j]) for j in range(1, eot)) or eot == 1
    if stage == "at:20" and r > 1:
        assert all(not np.array_equal(got.reshape(ROWS, r, n)[1, i], got.reshape(ROWS, r, n)[1, j]) for i in range(r) for j in range(i))


def test_a_batch_of_a0_rows_composes_to_the_host_utterances():
    a0 = CP.cast_i16(_audio())
    comp = np.stack(_companions())
    e = Engine(0)
    try:
        e.set_companions(comp)
        e.set_play_offset(N - 1)
        got = e.debug_compose(np.stack([a0] * 3), a0, 4, 5, 1, 0)
        tau = e.debug_play_offsets(5, 1, 0, 3, 12)
    finally:
        e.close()
    assert len(set(tau.ravel().tolist())) > 30          # (the offsets are all over the loop, and still ...)
    assert np.array_equal(got, np.broadcast_to(np.concatenate([a0[None], comp])[None, :, None], (3, 3, 4, N)))


# ------------------------------------------------------------------------------------------------ the identities
@pytest.mark.parametrize("kind", ["gmm", "ivector"])
def test_without_an_offset_nothing_changes(small_system, monkeypatch, kind):
    """never set, or set and cleared again: the attack of an engine that never saw the call, on the default (fused) chain, with
    the launches of the parent (the route counters)"""
    monkeypatch.delenv("FB_NO_FUSE", raising=False)
    task, kw = ("OSI", dict(target=1)) if kind == "gmm" else ("SV", {})
    p = nes_params(task, "targeted", samples_per_draw=SPD, max_iter=6, epsilon=0.002, threshold=1e3, seed=5, stream=1, **kw)
    audio = _audio()
    mk = (lambda: _gmm(small_system, "OSI")) if kind == "gmm" else _iv_sv
    a, b = mk(), mk()
    try:
        base = a.attack(p, audio)
        base_route = a.debug_nes_route()
        assert base[3].shape[0] == 6 and np.all(np.isfinite(base[3]))
        b.set_play_offset(500)
        with_s = b.attack(p, audio)
        assert with_s[3].shape[0] == 6 and not np.array_equal(with_s[3], base[3])       # (it does act while set)
        assert b.debug_play_route() == 6 and b.debug_nes_route() != base_route          # one launch per batch, the eot route
        b.set_play_offset(0)
        assert _same(base, b.attack(p, audio)) and b.debug_nes_route() == base_route and b.debug_play_route() == 0
        b.set_play_offset(7)
        _native.check(b._L.fb_set_play_offset(b._h, ctypes.c_int64(0)))
        assert _same(base, b.attack(p, audio)) and b.debug_nes_route() == base_route and b.debug_play_route() == 0
        b.set_play_offset(None)
        assert _same(base, b.attack(p, audio))
    finally:
        a.close()
        b.close()


# ------------------------------------------------------------------------------------------------ averaging
def _losses(sc, gmm, thr, adv_thr):
    if gmm:
        return (np.maximum(np.delete(sc, 1, axis=1).max(axis=1), thr) + adv_thr) - sc[:, 1]
    return (thr + adv_thr) - sc[:, 0]


@pytest.mark.parametrize("kind", ["gmm OSI", "gmm OSI adpcm", "ivector SV"])
def test_the_loss_is_the_mean_over_offsets_and_utterances(small_system, philox, kind):
    """A perturbed audio against its original through fb_get_grad_wb_from with the switches on (fb_get_grad's a_0 is the audio
    it is handed, so its row 0 carries no perturbation): K = 3 utterances, S = 500, no random stage.  adver_loss and score0 must
    be the contract-order mean of ordinary scoring calls on the numpy-composed rows -- tests/test_gpu_companions.py's bound:
    SCORE_TOL, and 2 * SCORE_TOL for the OSI loss, a difference of two scores.  The ADPCM case codes the composed rows on the
    host (tests/codec_ref.py) and scores them on an engine without a codec.  Then an NES call for fb_stats."""
    thr, adv_thr, S, it, seed, stream = 0.1, 0.05, 500, 4, 11, 6
    gmm, adpcm = kind.startswith("gmm"), kind.endswith("adpcm")
    original = _audio()
    audio = original + np.where(np.random.RandomState(3).randint(0, 2, N) == 1, 40.0, -40.0) / 32768.0
    comp = _companions()
    mk = (lambda: _gmm(small_system, "OSI")) if gmm else _iv_sv
    d, c = mk(), mk()
    try:
        d.set_companions(comp)
        d.set_play_offset(S)
        d.set_wb_universal(True)
        d.set_wb_ivector(not gmm)
        if adpcm:
            d.set_codec("adpcm")
            d.set_wb_bpda(True)
        kw = dict(target=1) if gmm else {}
        p = nes_params("OSI" if gmm else "SV", "targeted", samples_per_draw=0, threshold=thr, adver_thresh=adv_thr, seed=seed, stream=stream, **kw)
        before = d.stats()["scored_utts"]
        _g, al, sc0 = d.get_grad_wb_from(p, audio, original, it)
        assert d.stats()["scored_utts"] - before == 3
        tau = d.debug_play_offsets(seed, stream, it, 1, 3)[0]
        want_tau = R.offsets(philox, seed, stream, it, 1, 3, S)[0]
        assert np.array_equal(tau, want_tau) and len(set(tau.tolist())) >= 2
        rows = R.compose_rows(CP.cast_i16(audio), CP.cast_i16(original), np.stack(comp), 1, want_tau)
        scored = [codec_ref.adpcm(w) for w in rows] if adpcm else list(rows)
        # (under an offset the hook returns the rows the front end reads: coded where a codec is set)
        assert np.array_equal(d.debug_compose(CP.cast_i16(audio), CP.cast_i16(original), 1, seed, stream, it)[0, :, 0], np.stack(scored))
        assert not np.array_equal(rows, CR.compose_row(CP.cast_i16(audio), CP.cast_i16(original), np.stack(comp)))   # the offsets act
        raw, tv = c.score_raw(scored)
        assert np.all(tv > 0)
        sc = c.system_scores(raw)                                        # [K][S]
        losses = _losses(sc, gmm, thr, adv_thr)
        want_sc, want_al = CR.mean_over_replicas(sc.T), float(CR.mean_over_replicas(losses))
        # fb_get_grad under the same setting: (spd + 1) * K * eot rows scored
        d.set_eot(2)
        pn = nes_params("OSI" if gmm else "SV", "targeted", samples_per_draw=SPD, threshold=thr, adver_thresh=adv_thr, seed=seed, stream=stream, **kw)
        before = d.stats()["scored_utts"]
        fl, _gg, al_nes, _s = d.get_grad(pn, audio, it=it)
        assert d.stats()["scored_utts"] - before == (SPD + 1) * 3 * 2 and np.isfinite(fl) and np.isfinite(al_nes)
    finally:
        d.close()
        c.close()
    n_sc = want_sc.size
    print("%s: score0 %.3g adver_loss %.3g (bound %.3g)" % (kind, np.abs(sc0[:n_sc] - want_sc).max(), abs(al - want_al), SCORE_TOL))
    assert np.abs(sc0[:n_sc] - want_sc).max() <= SCORE_TOL
    assert abs(al - want_al) <= (2 if gmm else 1) * SCORE_TOL
    assert np.ptp(losses) > 10 * SCORE_TOL                               # the rows do differ: the mean is not a formality


# ------------------------------------------------------------------------------------------------ reproducibility
def _attack_once(system, stream=2, warm=False, S=500):
    e = _gmm(system, "OSI")
    try:
        e.set_input_transform("at:20")
        e.set_eot(2)
        e.set_companions(_companions())
        e.set_play_offset(S)
        if warm:                                                         # an unrelated scoring call: the serial advances
            e.score_raw([CP.cast_i16(_audio(3))])
        p = nes_params("OSI", "targeted", samples_per_draw=SPD, max_iter=5, target=1, epsilon=0.002, threshold=1e3, seed=5, stream=stream)
        return e.attack(p, _audio()), (e.debug_play_offsets(5, stream, 0, SPD + 1, 6) if S else None)
    finally:
        e.close()


def test_an_attack_under_an_offset_depends_on_seed_and_stream_only(small_system):
    a, tau = _attack_once(small_system)
    assert a[3].shape[0] == 5 and np.all(np.isfinite(a[3]))
    assert _same(a, _attack_once(small_system)[0])                                       # a fresh engine
    assert _same(a, _attack_once(small_system, warm=True)[0])                            # after an unrelated scoring call
    b, tau_b = _attack_once(small_system, stream=3)
    assert not np.array_equal(tau, tau_b) and not np.array_equal(a[3], b[3])             # another stream: other offsets
    assert not np.array_equal(a[3], _attack_once(small_system, S=0)[0][3])               # and the offsets matter


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals(small_system):
    audio = _audio()
    e = _gmm(small_system, "OSI")
    try:
        e.set_play_offset(300)
        p = nes_params("OSI", "targeted", samples_per_draw=SPD, max_iter=3, target=1, threshold=1e3, seed=5, stream=1)
        want = e.attack(p, audio)

        def refused(fn, code, *words):
            with pytest.raises(NativeError) as ex:
                fn()
            assert ex.value.code == code, str(ex.value)
            for w in words:
                assert w in str(ex.value), str(ex.value)
        for S in (-1, 2 ** 31 - 1, 2 ** 40):                                             # the setter's range: the previous S stays
            refused(lambda: _native.check(e._L.fb_set_play_offset(e._h, ctypes.c_int64(S))), FB_E_ARG)
        with pytest.raises(ValueError):
            e.set_play_offset(2 ** 31 - 1)
        assert e.play_offset == 300 and _same(want, e.attack(p, audio))
        named = ("fb_set_play_offset", "not in this version")
        refused(lambda: e.estimate_threshold(nes_params("OSI", "untargeted", samples_per_draw=SPD, seed=1), 1e3, audio, max_total_iters=3),
                FB_E_STATE, *named)
        pw = nes_params("OSI", "targeted", target=1, threshold=0.0, max_iter=2)
        theta = np.full((29, 257), 1e6)                                                  # (N = 4000, window 512, hop 128: 29 frames)
        for quorum in (None, "majority"):
            e.set_query_eot(quorum)
            refused(lambda: e.attack_pso(p, pso_params(particles=4), audio), FB_E_STATE, *named)
            refused(lambda: e.attack_kenansville(p, kv_params(), audio), FB_E_STATE, *named)
            refused(lambda: e.attack_hsj(p, hsj_params(), audio, audio), FB_E_STATE, *named)
        e.set_query_eot(None)
        refused(lambda: e.attack_cw2(pw, cw2_params(search_steps=1), audio), FB_E_STATE, *named)
        refused(lambda: e.attack_psy(pw, cw2_params(search_steps=1), psy_params(theta, 1.0, 512), audio), FB_E_STATE, *named)
        refused(lambda: e.get_grad_wb(pw, audio), FB_E_STATE, *named)                    # fb_set_wb_universal is off
        refused(lambda: e.get_grad_wb_from(pw, audio, audio, 0), FB_E_STATE, *named)
        refused(lambda: e.attack_wb(pw, audio), FB_E_STATE, *named)
        assert _same(want, e.attack(p, audio))                                           # the engine and S as they were
        short = _audio(n=300)                                                            # N <= S
        refused(lambda: e.attack(p, short), FB_E_ARG, "fb_set_play_offset")
        refused(lambda: e.get_grad(p, _audio(n=200)), FB_E_ARG, "fb_set_play_offset")
        refused(lambda: e.bench_nes(p, short, 1, 1), FB_E_ARG, "fb_set_play_offset")      # the timing loop is an NES call too
        refused(lambda: e.bench_nes(p, _audio(n=299), 0, 2), FB_E_ARG, "fb_set_play_offset")
        assert e.bench_nes(p, _audio(n=301 + 400), 1, 2)[0] > 0.0                         # (one sample more than S: it runs)
        e.set_wb_universal(True)
        refused(lambda: e.get_grad_wb(pw, short), FB_E_ARG, "fb_set_play_offset")
        e.get_grad_wb(pw, _audio(n=301 + 400))                                            # one more sample than S, and a frame: fine
        e.set_wb_universal(False)
        e.set_companions(np.stack(_companions()))                                        # K * eot > 32 from either side
        refused(lambda: _native.check(e._L.fb_set_eot(e._h, ctypes.c_int(11))), FB_E_ARG)
        e.set_companions(None)
        assert e.play_offset == 300 and _same(want, e.attack(p, audio))
        raw0 = e.score_raw([CP.cast_i16(audio)])                                         # scoring ignores the offset
        e.set_play_offset(0)
        raw1 = e.score_raw([CP.cast_i16(audio)])
        assert np.array_equal(raw0[0], raw1[0])
        refused(lambda: e.debug_play_offsets(1, 0, 0, 1, 1), FB_E_STATE)                 # nothing to draw without one
    finally:
        e.close()


@pytest.mark.parametrize("air", [False, True])
def test_the_defence_hook_ignores_the_offset(small_system, air):
    """fb_debug_defence_vjp has no contract point of the play offset: with one set -- below the length or beyond it, on an engine
    that never composed a row and on one that did -- its rows and its transposes are those of an engine without one, through an
    SNR noise stage (the power index), a median and, in the second case, the channel's transpose"""
    n, seed, stream, it = N, 11, 6, 3
    wav = CP.cast_i16(_audio())
    cot = np.random.default_rng(4).standard_normal((2, n))
    e = _gmm(small_system, "OSI")
    try:
        e.set_input_transform("at:20,ms:3")
        e.set_air_channel(ROOM64 if air else None)
        e.set_eot(2)
        e.set_wb_bpda(True)
        e.set_wb_air(air)
        want = e.debug_defence_vjp(wav, cot, seed, stream, it)
        want_route = e.debug_wb_route()
        for S in (500, n + 5):                         # (the first on an engine whose wav_play was never written)
            e.set_play_offset(S)
            got = e.debug_defence_vjp(wav, cot, seed, stream, it)
            assert np.array_equal(got[1], want[1]) and np.array_equal(got[0].view(np.uint64), want[0].view(np.uint64)), S
            assert e.debug_wb_route() == want_route and e.debug_play_route() == 0 and e.debug_wb_play_route() == 0
        e.set_play_offset(500)                         # ... and after a call that did compose
        e.set_wb_universal(True)
        p = nes_params("OSI", "targeted", samples_per_draw=0, target=1, threshold=0.0, seed=seed, stream=stream)
        e.get_grad_wb_from(p, _audio(), _audio(), it)
        got = e.debug_defence_vjp(wav, cot, seed, stream, it)
        assert np.array_equal(got[1], want[1]) and np.array_equal(got[0].view(np.uint64), want[0].view(np.uint64))
    finally:
        e.close()
    assert np.isfinite(want[0]).all() and want[0].any()


def test_foreign_models_ignore_the_offset(small_system):
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
        x.set_play_offset(N + 5)                                         # (longer than the audio: no refusal here either)
        calls.clear()
        assert _same(base, x.attack_ext(p, 3, score, audio))
        assert set(calls) == {SPD + 1}                                   # the batch is not replicated
        g = x.get_grad_ext(p, 3, score, audio)
        assert all(np.array_equal(u, v) for u, v in zip(g, g_base)) and x.debug_play_route() == 0
    finally:
        x.close()


# ------------------------------------------------------------------------------------------------ the Python surface
def test_fakebob_reports_every_offset_of_the_grid(small_system, tmp_path):
    from fakebob_amd.attack import FakeBob
    from fakebob_amd.systems import gmm_OSI
    ubm, spk = small_system
    ml = [["spk%d" % i, "utt%d" % i, g, -60.0 - i, 2.0 + i] for i, g in enumerate(spk)]
    model = gmm_OSI(str(tmp_path / "osi"), ml, ubm, pre_model_dir=str(tmp_path), threshold=0.0)
    try:
        audio, comp = _audio(), _companions()
        fb = FakeBob("OSI", "targeted", model, samples_per_draw=SPD, max_iter=4, epsilon=0.004, seed=5, verbose=False, play_offset=200)
        res = fb.attack(audio, None, threshold=1e3, target=1, companions=comp)
        assert model.engine.play_offset == 0 and model.engine.companions is None        # for that call only
        adv, flag = res
        per = res.per_offset
        assert [d["utterance"] for d in per] == [0, 1, 2]
        grid = PO.offset_grid(200)
        assert len(grid) == 16 and grid[0] == 0 and grid[-1] == 200
        hosts = [CP.cast_i16(audio)] + comp
        for d, host in zip(per, hosts):
            assert d["offsets"] == grid and len(d["decisions"]) == 16 and len(d["successes"]) == 16
            assert d["n_success"] == sum(d["successes"])
            for t, dec in zip(grid[:3], d["decisions"][:3]):
                w = PO.compose(host, res.perturbation_i16, t)
                assert int(model.make_decisions(w)[0]) == int(dec)
        for t in (0, 1, 77, 200, N - 1):
            moved = res.apply_perturbation(comp, offset=t)
            assert all(np.array_equal(m, PO.compose(h, res.perturbation_i16, t)) for m, h in zip(moved, comp))
        assert np.array_equal(res.apply_perturbation([audio])[0], adv[:, 0])             # offset 0, utterance 0: adv itself
        plain = FakeBob("OSI", "targeted", model, samples_per_draw=SPD, max_iter=2, seed=5, verbose=False).attack(audio, None, threshold=1e3, target=1)
        assert not hasattr(plain, "per_offset")
        with pytest.raises(ValueError):
            FakeBob("OSI", "targeted", model, play_offset=N, verbose=False).attack(audio, None, threshold=1e3, target=1)
    finally:
        model.engine.close()
