"""Input-transform chains on the device (fb_set_input_transform; the stage contract of include/fakebob_hip.h): the
kernel against the numpy restatement bit for bit, then what the contract promises about where the chain applies --
scoring, the NES loops -- and where it does not, and the refusals.

Bit-exact checks use np.array_equal.  The two tolerance checks carry the bound of tests/test_gpu_properties.py between an
NES batch's column 0 and a scoring call (2e-6), once per side."""
import numpy as np
import pytest

from fakebob_amd import input_transform as T
from fakebob_amd._native import FB_E_ARG, NativeError
from fakebob_amd.engine import Engine, nes_params
from fakebob_amd.models import synthetic_audio, synthetic_gmm_system, synthetic_ivector_system
from tests.input_transform_ref import ref

pytestmark = pytest.mark.gpu
TILE = 4096
SCORE_TOL = 2e-6


def _wav(utt, n=48000):
    return (synthetic_audio(utt, n) * 32768.0).astype(np.int16)


def _cast(x):
    """the wrappers' int16 cast of float audio (gmm_ubm_OSI.py:83-85)"""
    return (np.asarray(x, np.float64) * 32768.0).astype(np.int64).astype(np.int16)


def _noisy(n, seed):
    """full-range samples with runs at both ends of the scale (both clips fire behind a gain) and a quiet stretch"""
    rng = np.random.default_rng(seed)
    x = rng.integers(-32768, 32768, n).astype(np.int16)
    for a, v in ((n // 5, 32767), (n // 2, -32768), (3 * n // 4, 32767)):
        x[a:a + 37] = v
    q = x[n // 3:n // 3 + 50]
    q[:] = rng.integers(-3, 4, q.size)
    return x


def _delta(L, at=None, gain=1.0):
    h = np.zeros(L)
    h[(L - 1) // 2 if at is None else at] = gain
    return h


def _taps(L, seed, gain):
    """random taps of both signs whose sum is `gain`: inexact products and a sum whose order matters"""
    h = np.random.default_rng(seed).normal(size=L)
    return h * (gain / h.sum())


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


SINGLE = {
    "ms:3": [T.median(3)], "ms:7": [T.median(7)], "ms:31": [T.median(31)],
    "fir:1": [T.fir([-1.5])], "fir:3": [T.fir([0.25, 0.5, 0.25])], "fir:101": [T.fir(_taps(101, 1, 0.9))],
    "fir:511": [T.fir(_taps(511, 2, 1.0))], "fir:101:gain3": [T.fir(_taps(101, 3, 3.0))],
    "qt:1": [T.quant(1)], "qt:128": [T.quant(128)], "qt:1024": [T.quant(1024)],
    "dec:2": [T.decimate(2)], "dec:5": [T.decimate(5)],
}
CHAINS = {
    "2: ms:3,qt:128": T.parse("ms:3,qt:128"),
    "2: gain then median": [T.fir(_delta(1, gain=4.0)), T.median(5)],
    "3: squeeze 2": T.squeeze(2),
    "3: squeeze 5, 31 taps": T.squeeze(5, 31),
    "4: as:9,dec:3,lpf,qt": T.parse("as:9,dec:3,lpf:3000:51,qt:16"),
    "5: halo 1024": [T.fir(_taps(511, 4, 1.0)), T.fir(_taps(511, 5, -1.0)), T.fir(_delta(511, at=3)), T.fir(_delta(511, at=507)),
                     T.median(9)],
    "6": T.parse("qt:7,ms:15,dec:5,as:5,ms:3,qt:1000"),
    "8": [T.quant(64), T.median(5), T.fir(np.full(9, 1.0 / 9)), T.decimate(3), T.fir(_taps(101, 6, 3.0)), T.median(31),
          T.quant(1), T.fir([-1.5])],
    "8: squeeze twice": T.squeeze(2, 31) + [T.median(3)] + T.squeeze(3, 63) + [T.quant(4)],
}
# shorter than any halo, around one tile, several tiles with a remainder (the decimation phase 4096 mod 5, mod 3 crosses the
# tile boundaries), three seconds
LENGTHS = [1, 5, 100, TILE - 1, TILE, TILE + 1, 3 * TILE + 17, 48000]


# ------------------------------------------------------------------------------------- 1. the kernel, bit for bit
@pytest.mark.parametrize("name", sorted(SINGLE) + sorted(CHAINS))
def test_kernel_equals_the_restatement(eng, name):
    chain = SINGLE.get(name) or CHAINS[name]
    eng.set_input_transform(chain)
    try:
        wavs = [_noisy(n, 100 + i) for i, n in enumerate(LENGTHS)]
        got = eng.debug_input_transform(wavs)                       # one batch of unequal lengths
        for w, g in zip(wavs, got):
            want = ref(w, chain)
            assert g.dtype == np.int16 and g.shape == want.shape
            assert np.array_equal(g, want), (name, w.size, int(np.flatnonzero(g != want)[0]))
        one = eng.debug_input_transform([wavs[4]])                  # ... and alone
        assert np.array_equal(one[0], got[4])
        if name in ("fir:101:gain3", "8"):
            y = ref(wavs[-1], chain)
            assert y.max() == 32767 and y.min() == -32768           # both clips fired
    finally:
        eng.set_input_transform(None)


@pytest.mark.parametrize("name", ["ms:31", "fir:511", "qt:128", "dec:5", "8", "5: halo 1024"])
def test_kernel_on_a_30_s_utterance(eng, name):
    chain = SINGLE.get(name) or CHAINS[name]
    w = _noisy(480000, 7)
    eng.set_input_transform(chain)
    try:
        got = eng.debug_input_transform([w])[0]
    finally:
        eng.set_input_transform(None)
    assert np.array_equal(got, ref(w, chain))


def test_no_chain_is_a_copy(eng):
    eng.set_input_transform(None)
    wavs = [_noisy(n, i) for i, n in enumerate((3, TILE + 5, 9000))]
    for w, g in zip(wavs, eng.debug_input_transform(wavs)):
        assert np.array_equal(w, g)


# ---------------------------------------------------------------------------------------------- 2. scoring identity
def _gmm_engine(system, chain=None, **fe):
    ubm, spk = system
    e = Engine(0)
    e.set_frontend(**fe)
    e.load_gmm([ubm] + spk)
    e.set_system("OSI")
    e.set_input_transform(chain)
    return e


@pytest.mark.parametrize("mfcc_f32", [0, 1], ids=["float64 MFCC", "float32 MFCC"])
def test_scoring_through_the_chain_is_scoring_the_transformed_audio_gmm(small_system, mfcc_f32):
    chain = T.parse("ms:7,qt:16")
    wavs = [_wav(0), _wav(1, 30000), _wav(2, 20001)]
    d = _gmm_engine(small_system, chain, mfcc_f32=mfcc_f32)
    c = _gmm_engine(small_system, None, mfcc_f32=mfcc_f32)
    try:
        raw_d, tv_d = d.score_raw(wavs)
        raw_c, tv_c = c.score_raw([ref(w, chain) for w in wavs])    # same batch shape: same bits
        raw_f, tv_f = d.score_raw([w.astype(np.float64) / 32768.0 for w in wavs])   # fb_score_f64 goes through it too
        raw_0, _ = c.score_raw(wavs)
        route = d.debug_frontend_route()["mfcc"]
        m_d, m_c = d.debug_mfcc(wavs[1]), c.debug_mfcc(ref(wavs[1], chain))          # the hooks as well
    finally:
        d.close()
        c.close()
    assert route == ("k_mfcc_f32<12>" if mfcc_f32 else "k_mfcc_r16<12,true>")
    assert np.array_equal(tv_d, tv_c) and np.array_equal(raw_d, raw_c)
    assert np.array_equal(tv_f, tv_c) and np.array_equal(raw_f, raw_c)
    assert np.array_equal(m_d.view(np.uint32), m_c.view(np.uint32))
    assert np.abs(raw_d - raw_0).max() > 1e-3


def test_scoring_through_the_chain_is_scoring_the_transformed_audio_ivector():
    sy = synthetic_ivector_system(C=96, D=72, R=48, L=24, n_speakers=3, seed=11)
    chain = T.parse("ms:7,qt:16")
    wavs = [_wav(0), _wav(1, 30000), _wav(2, 20001)]
    d, c = Engine(0), Engine(0)
    try:
        d.load_ivector(sy, "OSI")
        c.load_ivector(sy, "OSI")
        d.set_input_transform(chain)
        raw_d, tv_d = d.score_raw(wavs)
        raw_c, tv_c = c.score_raw([ref(w, chain) for w in wavs])
        raw_0, _ = c.score_raw(wavs)
    finally:
        d.close()
        c.close()
    assert np.array_equal(tv_d, tv_c) and np.array_equal(raw_d, raw_c)
    assert not np.array_equal(raw_d, raw_0)


def test_enrolment_statistics_go_through_the_chain(small_system):
    ubm, _ = small_system
    chain = T.parse("ms:7")
    w = _wav(3)
    d, c = Engine(0), Engine(0)
    try:
        d.load_gmm([ubm])
        c.load_gmm([ubm])
        d.set_input_transform(chain)
        occ_d, F_d, tv_d = d.gmm_acc_stats(w)
        occ_c, F_c, tv_c = c.gmm_acc_stats(ref(w, chain))
    finally:
        d.close()
        c.close()
    assert tv_d == tv_c and np.array_equal(occ_d, occ_c) and np.array_equal(F_d, F_c)


# ------------------------------------------------------------------------------------------------ 3. / 4. attacks
def _attack(system, chain, fused, max_iter=12, iv=False):
    audio = synthetic_audio(9, 48000)
    e = Engine(0)
    try:
        if iv:
            e.load_ivector(system, "OSI")
        else:
            e.load_gmm([system[0]] + system[1])
            e.set_system("OSI")
        e.set_fused_chain(fused)
        e.set_input_transform(chain)
        p = nes_params("OSI", "targeted", samples_per_draw=50, max_iter=max_iter, target=1, epsilon=0.002, threshold=1e3,
                       seed=5, stream=1)
        return e.attack(p, audio)
    finally:
        e.close()


def _same(a, b):
    return a[1] == b[1] and np.array_equal(a[0], b[0]) and np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])


IDENTITY = [T.fir([1.0]), T.quant(1)]


@pytest.mark.parametrize("launches", ["fused", "unfused", "FB_NO_FUSE"])
def test_identity_chain_leaves_the_attack_alone(full_system, monkeypatch, launches):
    monkeypatch.delenv("FB_NO_FUSE", raising=False)
    if launches == "FB_NO_FUSE":
        monkeypatch.setenv("FB_NO_FUSE", "1")
    fused = {"fused": True, "unfused": False, "FB_NO_FUSE": None}[launches]
    plain = _attack(full_system, None, fused)
    assert plain[3].shape[0] == 12 and np.all(np.isfinite(plain[3]))
    assert _same(plain, _attack(full_system, IDENTITY, fused))


def test_identity_chain_leaves_the_attack_alone_ivector():
    sy = synthetic_ivector_system(C=96, D=72, R=48, L=24, n_speakers=3, seed=11)
    plain = _attack(sy, None, None, iv=True)
    assert plain[3].shape[0] == 12
    assert _same(plain, _attack(sy, IDENTITY, None, iv=True))


def test_a_real_chain_gives_one_trajectory_on_every_launch_chain(full_system, monkeypatch):
    monkeypatch.delenv("FB_NO_FUSE", raising=False)
    a = _attack(full_system, "ms:7", True)
    assert _same(a, _attack(full_system, "ms:7", True))             # again, on another engine
    assert _same(a, _attack(full_system, "ms:7", False))            # the unfused launch chain
    assert _same(a, _attack(full_system, "ms:7", None))
    assert not np.array_equal(a[3], _attack(full_system, None, True)[3])   # and it is not the undefended trajectory


# -------------------------------------------------------------------------------------------------- 5. refusals
def test_refusals_keep_the_previous_chain(eng, small_system):
    kept = T.parse("ms:5,qt:32")
    w = _noisy(10000, 3)
    d = _gmm_engine(small_system, kept)
    try:
        want_scores = d.score_raw([_wav(0)])[0]
        t511 = _delta(511)
        bad = {
            "9 stages": [T.quant(2)] * 9,
            "radii 1025": [T.Stage(T.FIR, 511, t511)] * 4 + [T.median(11)],
            "qt 0": [T.Stage(T.QUANT, 0, None)], "qt 16385": [T.Stage(T.QUANT, 16385, None)],
            "ms even": [T.Stage(T.MEDIAN, 4, None)], "ms 1": [T.Stage(T.MEDIAN, 1, None)], "ms 33": [T.Stage(T.MEDIAN, 33, None)],
            "fir 513": [T.Stage(T.FIR, 513, _delta(513))], "fir even": [T.Stage(T.FIR, 4, np.ones(4))],
            "fir 0": [T.Stage(T.FIR, 0, np.ones(1))], "fir null": [T.Stage(T.FIR, 3, None)],
            "tap nan": [T.Stage(T.FIR, 3, np.array([0.0, np.nan, 0.0]))], "tap inf": [T.Stage(T.FIR, 1, np.array([np.inf]))],
            "tap big": [T.Stage(T.FIR, 1, np.array([-(2.0 ** 20) - 1.0]))],
            "dec 1": [T.Stage(T.DECIMATE, 1, None)], "dec 65": [T.Stage(T.DECIMATE, 65, None)],
            "kind 4": [T.Stage(4, 3, None)], "kind -1": [T.Stage(-1, 3, None)],
            "second stage bad": [T.quant(2), T.Stage(T.MEDIAN, 6, None)],
        }
        for name, stages in sorted(bad.items()):
            with pytest.raises(NativeError) as ex:
                d.set_input_transform(stages, validate=False)
            assert ex.value.code == FB_E_ARG, name
            assert np.array_equal(d.debug_input_transform([w])[0], ref(w, kept)), name
        assert np.array_equal(d.score_raw([_wav(0)])[0], want_scores)   # a scoring call behind the refusals: the kept chain's
        d.set_input_transform([T.Stage(T.FIR, 1, np.array([2.0 ** 20]))], validate=False)   # the limits themselves are inside
        d.set_input_transform([T.Stage(T.FIR, 511, t511)] * 4 + [T.median(9)], validate=False)
        assert np.array_equal(d.debug_input_transform([w])[0], ref(w, [T.median(9)]))
        d.set_input_transform(None)
        assert np.array_equal(d.debug_input_transform([w])[0], w)
    finally:
        d.close()


# ------------------------------------------------------------------------------------------------ 6. - 8. tolerance
def test_nes_through_the_chain_against_the_callback_path(full_system):
    """fb_get_grad on a defended engine == fb_get_grad_ext whose callback casts, applies the restatement and scores on a
    chain-less engine.  Each side is within SCORE_TOL of a scoring call (test_gpu_properties.py): scores and losses within
    2 * SCORE_TOL; g_i = mean_j(loss_j z_ij) / sigma with losses that differ by at most twice that, so
    |dg_i| <= 2 * SCORE_TOL * mean_j|z_ij| / sigma."""
    chain = T.parse("ms:7")
    audio = synthetic_audio(7, 48000)
    half, sigma = 10, 0.001
    noise = np.random.default_rng(1).normal(size=(audio.size, half))
    p = nes_params("OSI", "targeted", samples_per_draw=2 * half, target=2, threshold=0.1, sigma=sigma, seed=42, stream=3)
    d = _gmm_engine(full_system, chain)
    c = _gmm_engine(full_system, None)
    x = Engine(0)
    try:
        fl_d, g_d, al_d, sc_d = d.get_grad(p, audio, noise_pos=noise)

        def score(a):    # a: (N, B) float64
            raw, _ = c.score_raw([ref(_cast(a[:, b]), chain) for b in range(a.shape[1])])
            return raw[:, 1:] - raw[:, 0:1]
        fl_x, g_x, al_x, sc_x = x.get_grad_ext(p, 5, score, audio, noise_pos=noise)
    finally:
        d.close()
        c.close()
        x.close()
    print("scores %.3g final_loss %.3g adver_loss %.3g" % (np.abs(sc_d - sc_x).max(), abs(fl_d - fl_x), abs(al_d - al_x)))
    bound = 2 * SCORE_TOL * np.abs(noise).mean(axis=1) / sigma
    print("gradient: max |dg| / bound %.3g" % (np.abs(g_d - g_x) / bound).max())
    assert np.abs(sc_d - sc_x).max() <= 2 * SCORE_TOL
    assert abs(fl_d - fl_x) <= 2 * SCORE_TOL and abs(al_d - al_x) <= 2 * SCORE_TOL
    assert np.all(np.abs(g_d - g_x) <= bound)
    assert np.abs(g_d).max() > 0


def test_attack_on_a_defended_system_is_consistent(full_system):
    """ms:7 in front of the victim: trace row 0 holds the scores of ref(cast(audio)) on an undefended engine, the returned
    audio is the raw adversarial audio (the attacker submits it; the filter sits inside the victim), and on success the
    defended system's decision on it is the target."""
    chain = T.parse("ms:7")
    audio = synthetic_audio(9, 48000)
    d = _gmm_engine(full_system, chain)
    c = _gmm_engine(full_system, None)
    try:
        raw, _ = d.score_raw([_cast(audio)])
        sc = raw[0, 1:] - raw[0, 0]                                  # the defended system's own clean scores
        target = int(np.argsort(sc)[-2])
        thr = float(sc.max()) - 0.02
        p = nes_params("OSI", "targeted", samples_per_draw=50, max_iter=300, target=target, epsilon=0.002, threshold=thr,
                       seed=1, stream=0)
        adv, flag, adv_f, trace = d.attack(p, audio)
        raw_c, _ = c.score_raw([ref(_cast(audio), chain)])
        sc_c = raw_c[0, 1:] - raw_c[0, 0]
        raw_a, _ = d.score_raw([adv])
        sc_a = raw_a[0, 1:] - raw_a[0, 0]
    finally:
        d.close()
        c.close()
    print("flag %d after %d iterations; |trace row 0 - chain-less score| max %.3g" % (flag, trace.shape[0], np.abs(trace[0, 3:] - sc_c).max()))
    assert np.abs(trace[0, 3:] - sc_c).max() <= SCORE_TOL
    assert np.abs(adv_f - audio).max() <= 0.002 + 1e-15                       # the returned audio is not filtered:
    assert np.array_equal(adv, np.trunc(adv_f * 32768.0).astype(np.int64).astype(np.int16))
    assert np.all(trace[:, 0] <= 0.002 + 1e-12) and trace[-1, 0] > 0           # nor is the distance column
    assert flag == 1, "the attack on the ms:7 system did not succeed within 300 iterations"
    decision = int(np.argmax(sc_a)) if sc_a.max() >= thr else -1               # gmm_OSI.make_decisions
    assert decision == target


def test_the_chain_is_what_the_mfcc_reads(full_system):
    """ms:7 moves the clean scores of the synthetic system by more than 1e-3: a transformed buffer the MFCC did not read
    would leave them where they were."""
    w = _wav(9)
    d = _gmm_engine(full_system, None)
    try:
        plain, _ = d.score_raw([w])
        d.set_input_transform("ms:7")
        defended, _ = d.score_raw([w])
        d.set_input_transform(None)
        again, _ = d.score_raw([w])
    finally:
        d.close()
    print("ms:7 moves the raw scores by %.3g .. %.3g" % (np.abs(defended - plain).min(), np.abs(defended - plain).max()))
    assert np.abs((defended[0, 1:] - defended[0, 0]) - (plain[0, 1:] - plain[0, 0])).max() > 1e-3
    assert np.array_equal(again, plain)
