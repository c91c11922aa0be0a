"""The over-the-air channel on the device (fb_set_air_channel; its contract is in include/fakebob_hip.h): k_air_taps and
k_air_conv against the numpy restatement (tests/air_channel_ref.py) to the bit, the whole path in front of the chain and
behind the composition, the identity channel under every attack, scoring, attacks through a real channel, the refusals.
Every comparison of samples or taps is np.array_equal."""
import ctypes

import numpy as np
import pytest

from fakebob_amd import _native, air_channel as A, companions as CP, input_transform as T
from fakebob_amd._native import FB_E_ARG, NativeError
from fakebob_amd.engine import Engine, nes_params, pso_params
from fakebob_amd.models import synthetic_audio, synthetic_ivector_system
from tests import air_channel_ref as R
from tests.companions_ref import compose_row
from tests.feco_ref import feco_keys
from tests.input_transform_noise_ref import NOISE, eot_mean, ref_noisy
from tests.test_gpu_input_transform import SCORE_TOL   # the bound between an NES batch's column 0 and a scoring call

pytestmark = pytest.mark.gpu
SEED, STREAM, EPOCH = 0x1234567887654321, 7, 3
N = 16000
SPD = 6
ROOM = A.AirChannel(1000, 32, 3000.0, 0.995, 0.999)        # a real channel: a tail of 1000 taps, about 10 dB under the direct path
IDENT = A.AirChannel(1000, 32, 0.0, 0.995, 0.999)          # amp = 0: the identity, bit for bit


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


def _rand(n, seed, amp=3000):
    return np.random.default_rng(seed).integers(-amp, amp + 1, n).astype(np.int16)


def _audio(utt=9, n=N):
    return synthetic_audio(utt, n)


def _cast(x):
    return (np.asarray(x, np.float64) * 32768.0).astype(np.int64).astype(np.int16)


def _ref_taps(e, ch, seed, stream, epoch, utt, replica):
    """the restatement's taps of one row, fed the normals and the word the device drew; the device's own taps must be these"""
    got, z, w = e.debug_air_taps(seed, stream, epoch, utt, replica)
    want = R.taps(ch.taps, ch.predelay, ch.amp, ch.rho_lo, ch.rho_hi, z, w)
    assert np.array_equal(got, want)
    return want


# ------------------------------------------------------------------------------------------------------- k_air_taps
@pytest.mark.parametrize("L", [2, 3, 64, 65, 1000, 4096])
def test_taps_equal_the_restatement(eng, oracle, L):
    try:
        for d in sorted({1, min(32, L - 1), L - 1}):
            for rho_lo, rho_hi in ((1.0, 1.0), (0.99, 0.9995)):
                ch = A.AirChannel(L, d, 5000.0, rho_lo, rho_hi)
                eng.set_air_channel(ch)
                for utt, rep in ((0, 0), (3, 5)):
                    got, z, w = eng.debug_air_taps(SEED, STREAM, EPOCH, utt, rep)
                    assert got.dtype == np.int16 and got.shape == (L,) and z.dtype == np.float32 and z.shape == (L,)
                    want = R.taps(L, d, 5000.0, rho_lo, rho_hi, z, w)
                    assert np.array_equal(got, want), (L, d, rho_lo, int(np.flatnonzero(got != want)[0]))
                    assert got[0] == 16384 and not got[1:d].any()
                    assert w == oracle.philox(R.air_counter(R.DECAY_C0, rep, utt, EPOCH), R.air_key(SEED, STREAM))[0]
                    # the normals' layout: the oracle's float32 Box-Muller over Philox counters (n >> 2, j, iter, stream) pairs
                    # words 0, 1 and 2, 3 -- with the channel's key as its seed, j = replica, iter = utterance row and
                    # stream = epoch that is the counter (k >> 2, replica, utterance row, epoch) of the contract
                    k0, k1 = R.air_key(SEED, STREAM)
                    zo = oracle.noise(k0 | (k1 << 32), utt, EPOCH, 4 * ((L + 3) // 4), rep + 1)[rep][:L]
                    assert np.array_equal(z.view(np.uint32), zo.view(np.uint32)), (L, utt, rep)
                if L >= 64 and d < L // 2:
                    assert np.abs(got[d:]).max() > 1000              # there is a tail
    finally:
        eng.set_air_channel(None)


def test_the_clip_of_the_taps(eng):
    """amp at its limit and no decay: |amp * z| passes 32767 for |z| > 2, about one tap in twenty"""
    ch = A.AirChannel(4096, 1, 16384.0, 1.0, 1.0)
    eng.set_air_channel(ch)
    try:
        t = _ref_taps(eng, ch, SEED, STREAM, EPOCH, 0, 0)
    finally:
        eng.set_air_channel(None)
    assert (t == 32767).sum() > 40 and (t == -32767).sum() > 40 and t.min() == -32767


def test_normals_moments_and_layout(eng):
    eng.set_air_channel(A.AirChannel(4096, 1, 1.0, 0.5, 1.0))
    try:
        zs, ws = [], []
        for utt in range(64):
            _t, z, w = eng.debug_air_taps(SEED, STREAM, EPOCH, utt, 0)
            zs.append(z)
            ws.append(w)
        short = eng.debug_air_taps(SEED, STREAM, EPOCH, 5, 0)
        eng.set_air_channel(A.AirChannel(10, 1, 1.0, 0.5, 1.0))   # a shorter response draws the head of the same stream
        _t, z10, w10 = eng.debug_air_taps(SEED, STREAM, EPOCH, 5, 0)
    finally:
        eng.set_air_channel(None)
    assert np.array_equal(z10.view(np.uint32), short[1][:10].view(np.uint32)) and w10 == short[2]
    z = np.concatenate(zs).astype(np.float64)
    n = z.size
    assert np.all(np.isfinite(z))
    assert abs(z.mean()) <= 5.0 / np.sqrt(n)                   # sd of the mean: 1 / sqrt(n)
    assert abs(z.var() - 1.0) <= 5.0 * np.sqrt(2.0 / n)        # sd of the variance of normals: sqrt(2 / n)
    U = (np.array(ws, np.float64) + 0.5) * 2.0 ** -32
    assert len(set(ws)) == 64 and 0.3 < U.mean() < 0.7         # 64 uniforms: the mean's sd is 0.036


def test_every_word_of_the_key_and_counter_matters(eng):
    eng.set_air_channel(A.AirChannel(2048, 1, 100.0, 0.5, 1.0))
    try:
        base = dict(seed=SEED, stream=STREAM, epoch=EPOCH, utt=1, replica=0)
        _t, z, w = eng.debug_air_taps(**base)
        others = {"seed": SEED ^ 1, "seed hi": SEED ^ (1 << 40), "stream": STREAM + 1, "epoch": EPOCH + 1, "utt": 2, "replica": 1}
        for name, v in others.items():
            kw = dict(base)
            kw["seed" if name == "seed hi" else name] = v
            _t2, z2, w2 = eng.debug_air_taps(**kw)
            assert not np.any(np.all(z.reshape(-1, 4) == z2.reshape(-1, 4), axis=1)), name   # a row = one Philox call
            assert w2 != w, name
        again = eng.debug_air_taps(**base)
        assert np.array_equal(again[1].view(np.uint32), z.view(np.uint32)) and again[2] == w
    finally:
        eng.set_air_channel(None)


def test_no_row_shared_with_the_other_streams(eng, oracle):
    n, seed = 2048, 99
    eng.set_air_channel(A.AirChannel(n, 1, 100.0, 0.5, 1.0))
    try:
        _t, z, w = eng.debug_air_taps(seed, 0, 0, 0, 0)
    finally:
        eng.set_air_channel(None)
    z = z.reshape(-1, 4)
    noise = eng.debug_tf_noise(seed, 0, 0, 0, 0, 0, 0, n).reshape(-1, 4)
    nes = eng.debug_noise(seed, 0, 0, n, 1).reshape(-1, 4)
    dith = eng.debug_dither_noise(seed, 0, 0, 0, 0, 1, L=n).reshape(-1, 4)
    for name, other in (("noise", noise), ("NES", nes), ("dither", dith)):
        assert not np.any(np.all(z == other, axis=1)), name
    # FeCo and PSO use raw words: the channel's words at their counters, under their keys, are other words
    air_words = [oracle.philox(R.air_counter(c0, 0, 0, 0), R.air_key(seed, 0)) for c0 in list(range(16)) + [R.DECAY_C0]]
    assert air_words[-1][0] == w
    flat = {x for q in air_words for x in q}
    assert not flat & {int(k) for k in feco_keys(oracle.philox, seed, 0, 0, 0, 0, 64)}
    pso_key = [(seed & 0xFFFFFFFF) ^ 0x5053574D, (seed >> 32) & 0xFFFFFFFF]
    assert not flat & {x for c0 in range(16) for x in oracle.philox([c0, 0, 0, 0], pso_key)}
    assert not flat & {int(k) for k in eng.debug_feco_keys(seed, 0, 0, 0, 0, 64)}


# ------------------------------------------------------------------------------------------------------- k_air_conv
CONV_N = [1, 15, 16, 17, 255, 256, 257, 4099, 8191, 8193, 20000]


def _some_taps(L, seed):
    g = np.random.default_rng(seed)
    t = g.integers(-32767, 32768, L).astype(np.int16)
    t[0] = 16384
    t[1:1 + L // 3] //= 64                                     # (a quiet stretch: sums that do not clip)
    return t


@pytest.mark.parametrize("L", [2, 17, 64, 511, 4096])
def test_convolution_equals_the_restatement(eng, L):
    """one batch of unequal lengths, n < L included; each row has a response of its own"""
    wavs = [_rand(n, 10 + i, amp=32767 if i % 2 else 3000) for i, n in enumerate(CONV_N)]
    taps = np.stack([_some_taps(L, 100 + i) for i in range(len(wavs))])
    got = eng.debug_air_convolve(wavs, taps)
    for i, (w, g) in enumerate(zip(wavs, got)):
        want = R.convolve(w, taps[i])
        assert g.dtype == np.int16 and g.shape == w.shape
        assert np.array_equal(g, want), (L, w.size, int(np.flatnonzero(g != want)[0]))
    one = eng.debug_air_convolve([wavs[-1]], taps[-1])[0]     # a row does not depend on its batch
    assert np.array_equal(one, got[-1])
    assert any(not np.array_equal(g, w) for g, w in zip(got, wavs))


@pytest.mark.parametrize("L", [511, 4096])
def test_full_scale_input_against_full_scale_taps(eng, L):
    """the 2^42 bound and both clips: x = -32768 everywhere and alternating, taps of +-32767 with the same and alternating signs"""
    n = 8193
    flat = np.full(n, -32768, np.int16)
    alt = np.where(np.arange(n) % 2 == 0, 32767, -32768).astype(np.int16)
    same = np.full(L, 32767, np.int16)
    neg = np.full(L, -32767, np.int16)
    zig = np.where(np.arange(L) % 2 == 0, 32767, -32767).astype(np.int16)
    cases = [(flat, same), (flat, neg), (flat, zig), (alt, same), (alt, zig), (alt, neg)]
    got = eng.debug_air_convolve([x for x, _ in cases], np.stack([t for _, t in cases]))
    for (x, t), g in zip(cases, got):
        assert np.array_equal(g, R.convolve(x, t))
    assert np.abs(R.conv_sums(flat, same)).max() == L * 32767 * 32768
    assert np.all(got[0] == -32768) and np.all(got[1] == 32767)                # both clips, every sample
    assert got[4].max() == 32767 and got[4].min() == -32768                    # alternating against alternating: the largest swings


def test_identity_taps_and_a_silent_row(eng):
    L = 2048
    ident = np.zeros(L, np.int16)
    ident[0] = 16384
    w = _rand(9000, 3, amp=32767)
    w[:4] = (-32768, 32767, -32768, 32767)
    silent = np.zeros(5000, np.int16)
    got = eng.debug_air_convolve([w, silent], np.stack([ident, _some_taps(L, 1)]))
    assert np.array_equal(got[0], w) and np.array_equal(got[1], silent)


# ------------------------------------------------------------------------------------------------------- whole path
def _chain_after(e, o, chain, utt, rho, seed, stream, epoch):
    normals = {s: e.debug_tf_noise(seed, stream, epoch, utt, rho, s, 0, o.size) for s, st in enumerate(chain) if st.kind == NOISE}
    return ref_noisy(o, chain, normals)


@pytest.mark.parametrize("r", [1, 3])
@pytest.mark.parametrize("spec", [None, "ms:3", "at:20"])
def test_the_channel_in_front_of_the_chain(eng, spec, r):
    chain = T.parse(spec)
    wavs = [_rand(n, 30 + i) for i, n in enumerate((5, 4095, 4097, 9001))]
    wavs.append(np.zeros(700, np.int16))                      # a silent row stays silent through the channel and an SNR stage
    eng.set_air_channel(ROOM)
    eng.set_input_transform(chain)
    try:
        got = eng.debug_input_transform_eot(wavs, r, SEED, STREAM, EPOCH)
        plain = eng.debug_input_transform(wavs)                # no point of the contract: the channel is ignored
        for b, w in enumerate(wavs):
            for j in range(r):
                o = R.convolve(w, _ref_taps(eng, ROOM, SEED, STREAM, EPOCH, b, j))
                want = _chain_after(eng, o, chain, b, j, SEED, STREAM, EPOCH)   # (an SNR stage's E: the power of o)
                assert np.array_equal(got[b][j], want), (spec, r, b, j)
        eng.set_air_channel(None)
        if spec != "at:20":
            assert all(np.array_equal(p, q) for p, q in zip(plain, eng.debug_input_transform(wavs)))
    finally:
        eng.set_air_channel(None)
        eng.set_input_transform(None)
    assert not np.array_equal(got[3][0], wavs[3])
    assert not got[4][0].any()
    if r == 3:
        assert not any(np.array_equal(got[3][a], got[3][c]) for a, c in ((0, 1), (0, 2), (1, 2)))   # a room per draw


@pytest.mark.parametrize("spec", [None, "at:20"])
def test_the_channel_behind_the_composition(spec):
    """K = 2, r = 2: composition, then air, then the chain; replica rho = u * r + j draws the room and the noise"""
    n, r = 4100, 2
    chain = T.parse(spec)
    g = np.random.default_rng(1)
    a0 = CP.cast_i16(_audio(9, n))
    comp = np.stack([CP.cast_i16(_audio(21, n))])
    q = np.clip(a0.astype(np.int32) + g.integers(-70, 71, size=(3, n)), -32768, 32767).astype(np.int16)
    comp[0, :3] = (32767, -32768, 32767)
    q[1, :3], a0[:3] = (40, -40, 32767), (0, 0, -32768)         # the composition's clip acts on both sides
    e = Engine(0)
    try:
        e.set_air_channel(ROOM)
        e.set_input_transform(chain)
        e.set_companions(comp)
        got = e.debug_compose(q, a0, r, SEED, STREAM, EPOCH)
        assert got.shape == (3, 2, r, n)
        for b in range(3):
            w = compose_row(q[b], a0, comp)
            for u in range(2):
                for j in range(r):
                    rho = u * r + j
                    o = R.convolve(w[u], _ref_taps(e, ROOM, SEED, STREAM, EPOCH, b, rho))
                    assert np.array_equal(got[b, u, j], _chain_after(e, o, chain, b, rho, SEED, STREAM, EPOCH)), (b, u, j)
    finally:
        e.close()
    assert compose_row(q[1], a0, comp)[1, 0] == 32767


# ------------------------------------------------------------------------------------------------- identity channel
def _gmm(system, task="OSI"):
    ubm, spk = system
    e = Engine(0)
    if task == "SV":
        e.load_gmm([ubm, spk[0]])
    else:
        e.load_gmm([ubm] + spk)
    e.set_system(task)
    return e


def _same(a, b):
    return a[1] == b[1] and all(np.array_equal(u, v) for u, v in zip(a, b) if isinstance(u, np.ndarray))


@pytest.mark.parametrize("case", ["eot 3", "companions", "pso"])
def test_the_identity_channel_changes_no_attack(small_system, case):
    """at:20 is randomised per (utterance row, replica): the same trace, flag and audio with amp = 0 says that the chain's two
    indices survived its "input already replicated" mode"""
    e = _gmm(small_system)
    try:
        e.set_input_transform("at:20")
        audio = _audio()
        if case == "pso":
            run = lambda: e.attack_pso(nes_params("OSI", "targeted", epsilon=0.002, max_iter=4, target=1, threshold=1e3, seed=5, stream=1),   # noqa: E731
                                       pso_params(particles=4), audio)
        else:
            e.set_eot(3 if case == "eot 3" else 2)
            if case == "companions":
                e.set_companions([CP.cast_i16(_audio(20)), CP.cast_i16(_audio(21))])
            p = nes_params("OSI", "targeted", samples_per_draw=SPD, max_iter=5, target=1, epsilon=0.002, threshold=1e3, seed=5, stream=2)
            run = lambda: e.attack(p, audio)   # noqa: E731
        base = run()
        assert np.all(np.isfinite(base[3])) and base[3].shape[0] >= 4
        e.set_air_channel(IDENT)
        assert _same(base, run())
        e.set_air_channel(ROOM)
        assert not np.array_equal(base[3], run()[3])           # (and a real room is not the identity)
        e.set_air_channel(None)
        assert _same(base, run())
    finally:
        e.close()


# ---------------------------------------------------------------------------------------------------------- scoring
def _wav(utt, n=16000):
    return (synthetic_audio(utt, n) * 32768.0).astype(np.int16)


def _check_scoring(d, c):
    wavs = [_wav(0), _wav(1, 12000), _wav(2, 9001)]
    d.set_air_channel(ROOM)
    d.set_dither_seed(77)
    raw0, tv0 = d.score_raw(wavs)                                   # serial 0
    raw1, _ = d.score_raw(wavs)                                     # serial 1
    for serial, raw in ((0, raw0), (1, raw1)):
        ref_w = [R.convolve(w, _ref_taps(d, ROOM, 77, 0xFFFFFFFF, serial, b, 0)) for b, w in enumerate(wavs)]
        raw_c, tv_c = c.score_raw(ref_w)
        assert np.array_equal(raw, raw_c), serial
    assert np.array_equal(tv0, tv_c)
    assert not np.array_equal(raw0, raw1)                           # the serial advances: a fresh room per query
    d.set_dither_seed(77)
    assert np.array_equal(d.score_raw(wavs)[0], raw0)               # the same seed reproduces them
    assert np.array_equal(d.score_raw(wavs)[0], raw1)


@pytest.mark.parametrize("mfcc_f32", [0, 1], ids=["float64 MFCC", "float32 MFCC"])
def test_scoring_through_a_channel_gmm(small_system, mfcc_f32):
    ubm, spk = small_system
    d, c = Engine(0), Engine(0)
    try:
        for e in (d, c):
            e.set_frontend(mfcc_f32=mfcc_f32)
            e.load_gmm([ubm] + spk)
            e.set_system("OSI")
        _check_scoring(d, c)
    finally:
        d.close()
        c.close()


def test_scoring_through_a_channel_ivector():
    sy = synthetic_ivector_system(C=96, D=72, R=48, L=24, n_speakers=3, seed=11)
    d, c = Engine(0), Engine(0)
    try:
        d.load_ivector(sy, "OSI")
        c.load_ivector(sy, "OSI")
        _check_scoring(d, c)
    finally:
        d.close()
        c.close()


# ---------------------------------------------------------------------------------------------------------- attacks
def _attack_once(system, r=3, stream=2, batch=None, warm=False, channel=ROOM, monkeypatch=None):
    if batch is not None:
        monkeypatch.setenv("FB_ATTACK_BATCH", str(batch))
    e = _gmm(system)
    try:
        e.set_air_channel(channel)
        e.set_eot(r)
        kw = dict(samples_per_draw=SPD, max_iter=5, target=1, epsilon=0.002, threshold=1e3, seed=5)
        if warm:
            e.attack(nes_params("OSI", "targeted", stream=9, **kw), _audio(3))
        return e.attack(nes_params("OSI", "targeted", stream=stream, **kw), _audio())
    finally:
        e.close()
        if batch is not None:
            monkeypatch.delenv("FB_ATTACK_BATCH")


def test_an_attack_through_a_channel_depends_on_seed_and_stream_only(small_system, monkeypatch):
    monkeypatch.delenv("FB_ATTACK_BATCH", raising=False)
    a = _attack_once(small_system)
    assert a[3].shape[0] == 5 and np.all(np.isfinite(a[3]))
    assert _same(a, _attack_once(small_system))                                                # a fresh engine
    assert _same(a, _attack_once(small_system, batch=1, monkeypatch=monkeypatch))
    assert _same(a, _attack_once(small_system, batch=4, monkeypatch=monkeypatch))
    assert _same(a, _attack_once(small_system, warm=True))                                     # after another attack
    assert not np.array_equal(a[3], _attack_once(small_system, stream=3)[3])                   # another stream differs
    assert not np.array_equal(a[3], _attack_once(small_system, r=1)[3])                        # and r matters here


def test_clearing_the_channel_restores_the_undefended_trace(small_system):
    e = _gmm(small_system)
    try:
        p = nes_params("OSI", "targeted", samples_per_draw=SPD, max_iter=5, target=1, epsilon=0.002, threshold=1e3, seed=5, stream=2)
        base = e.attack(p, _audio())
        e.set_air_channel(ROOM)
        through = e.attack(p, _audio())
        assert not np.array_equal(base[3], through[3])
        e.set_air_channel("none")
        assert e.air_channel is None and _same(base, e.attack(p, _audio()))
        e.set_air_channel(ROOM)
        _native.check(e._L.fb_set_air_channel(e._h, None))                                      # NULL clears as well
        assert _same(base, e.attack(p, _audio()))
    finally:
        e.close()


@pytest.mark.parametrize("task,spec", [("SV", None), ("OSI", "at:20")])
def test_get_grad_averages_over_the_rooms(small_system, task, spec):
    """r = 3: score0 and adver_loss against the numpy mean (the contract's order) of per-replica system scores and losses from
    scoring the restated rows -- channel, then chain -- of the cast clean audio on an engine without either.  An NES batch's
    row and a scoring call of the same utterance agree to SCORE_TOL; the mean of r such rows keeps that bound, and the loss is
    a difference of two of them: 2 * SCORE_TOL."""
    r, it, seed, stream = 3, 4, 11, 6
    chain = T.parse(spec)
    audio = _audio()
    d, c = _gmm(small_system, task), _gmm(small_system, task)
    try:
        d.set_air_channel(ROOM)
        d.set_input_transform(chain)
        d.set_eot(r)
        thr, adv_thr = 0.1, 0.05
        kw = dict(target=1) if task == "OSI" else {}
        p = nes_params(task, "targeted", samples_per_draw=SPD, threshold=thr, adver_thresh=adv_thr, seed=seed, stream=stream, **kw)
        fl, _g, al, sc0 = d.get_grad(p, audio, it=it)
        w = _cast(audio)
        reps = []
        for j in range(r):
            o = R.convolve(w, _ref_taps(d, ROOM, seed, stream, it, 0, j))
            reps.append(_chain_after(d, o, chain, 0, j, seed, stream, it))
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
    assert np.ptp(losses) > 10 * SCORE_TOL                          # the rooms do differ: the mean is not a formality


# -------------------------------------------------------------------------------------------------------- refusals
def test_refusals_keep_the_previous_setting(eng):
    w = _rand(5000, 4)
    kept = A.AirChannel(64, 9, 2000.0, 0.97, 0.99)
    eng.set_air_channel(kept)
    try:
        want = eng.debug_input_transform_eot([w], 2, SEED, STREAM, EPOCH)[0]
        nan, inf = float("nan"), float("inf")
        bad = {
            "taps 1": (1, 1, 0.0, 0.5, 0.5), "taps -3": (-3, 1, 0.0, 0.5, 0.5), "taps 4097": (4097, 1, 0.0, 0.5, 0.5),
            "delay 0": (8, 0, 0.0, 0.5, 0.5), "delay L": (8, 8, 0.0, 0.5, 0.5), "delay -1": (8, -1, 0.0, 0.5, 0.5),
            "amp < 0": (8, 1, -1.0, 0.5, 0.5), "amp > 16384": (8, 1, 16384.5, 0.5, 0.5), "amp nan": (8, 1, nan, 0.5, 0.5),
            "amp inf": (8, 1, inf, 0.5, 0.5), "rho_lo 0": (8, 1, 1.0, 0.0, 0.5), "rho_lo < 0": (8, 1, 1.0, -0.5, 0.5),
            "lo > hi": (8, 1, 1.0, 0.6, 0.5), "hi > 1": (8, 1, 1.0, 0.5, 1.0000001), "lo nan": (8, 1, 1.0, nan, 0.5),
            "hi nan": (8, 1, 1.0, 0.5, nan), "hi inf": (8, 1, 1.0, 0.5, inf),
        }
        for name, vals in sorted(bad.items()):
            with pytest.raises(NativeError) as ex:
                eng.set_air_channel(vals, validate=False)          # past the wrapper: the library's own refusal
            assert ex.value.code == FB_E_ARG, name
            assert eng.air_channel == kept, name
            got = eng.debug_input_transform_eot([w], 2, SEED, STREAM, EPOCH)[0]
            assert all(np.array_equal(g, x) for g, x in zip(got, want)), name
        with pytest.raises(ValueError):
            eng.set_air_channel("t60:300,taps:5000")               # the wrapper's
        assert eng.air_channel == kept
        for ok in ((2, 1, 0.0, 1.0, 1.0), (4096, 4095, 16384.0, 1e-300, 1.0)):   # the limits themselves are inside
            eng.set_air_channel(ok, validate=False)
        p = _native.AirParams(0, -7, nan, nan, nan)                # taps == 0 clears, whatever else the struct holds
        _native.check(eng._L.fb_set_air_channel(eng._h, ctypes.byref(p)))
        with pytest.raises(NativeError) as ex:
            _native.check(eng._L.fb_debug_air_taps(eng._h, ctypes.c_uint64(1), ctypes.c_uint32(0), ctypes.c_uint32(0), ctypes.c_uint32(0),
                                                   ctypes.c_int(0), _native.ptr(np.zeros(8, np.int16)), None, None))
        assert ex.value.code == _native.FB_E_STATE                 # no channel: nothing to draw
        got = eng.debug_input_transform_eot([w], 2, SEED, STREAM, EPOCH)[0]
        assert all(np.array_equal(g, w) for g in got)              # cleared: a replicating copy again
        for L in (1, 4097):
            with pytest.raises(NativeError) as ex:
                eng.debug_air_convolve([w], np.zeros((1, L), np.int16))
            assert ex.value.code == FB_E_ARG
    finally:
        eng.set_air_channel(None)
