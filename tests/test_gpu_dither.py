"""Kaldi's dither on the device (fb_frontend_cfg.dither, the "Dither RNG contract" of include/fakebob_hip.h): the three
dithered MFCC kernels against the float64 numpy restatement fed the device's own normals, the normals themselves, digital
silence, the stages behind the MFCC matrix against the oracle's, and what the contract promises about attacks and scoring
calls.

Measured on an MI355X, |device - restatement| max over the four inputs and three dithers: 2.2e-5 .. 1.3e-4 on the float32
route (allowed 6e-4 .. 6.7e-4), 0.9e-6 .. 1.9e-6 on the two float64 routes (allowed 1.2e-4 .. 1.4e-4)."""
import math

import numpy as np
import pytest

from fakebob_amd._native import FB_E_ARG, NativeError
from fakebob_amd.engine import Engine, nes_params
from fakebob_amd.models import stack_models, synthetic_audio, synthetic_gmm_system, synthetic_ivector_system
from tests.test_dither_host import dither_wavs, np_mfcc_dither

pytestmark = pytest.mark.gpu
FLT_EPS = float(np.finfo(np.float32).eps)
SCORING_STREAM = 0xFFFFFFFF

# route -> (front-end overrides, the restatement's arguments, kernel without dither, kernel with it)
ROUTES = {
    "r16": (dict(mfcc_f32=0), dict(), "k_mfcc_r16<12,true>", "k_mfcc_r16<12,true,dither>"),
    "f32": (dict(mfcc_f32=1), dict(), "k_mfcc_f32<12>", "k_mfcc_f32<12,dither>"),
    "generic": (dict(mfcc_f32=0, frame_length=401), dict(L=401), "k_mfcc", "k_mfcc<dither>"),
}


def _wav(utt, n):
    return (synthetic_audio(utt, n) * 32768.0).astype(np.int16)


def _tol(route, want):
    """tests/test_oracle_frontend.py's tolerances for this restatement: the float64 routes, the float32 route"""
    m = np.abs(want).max()
    return 1e-5 * max(10.0, m) + 2e-4 if route == "f32" else 3e-6 * max(1.0, m)


@pytest.fixture()
def eng():
    e = Engine(0)
    yield e
    e.close()


# ------------------------------------------------------------------------------------------------------- 1. arithmetic
@pytest.mark.parametrize("route", sorted(ROUTES))
def test_dithered_mfcc_against_the_restatement(eng, route):
    """fb_debug_mfcc_dither == the numpy restatement fed the hook's own z, dither 0.5 / 1 / 3, on every route (asserted),
    and at dither 0 the hook equals fb_debug_mfcc bit for bit."""
    over, kw, plain, dithered = ROUTES[route]
    L = kw.get("L", 400)
    key = dict(seed=2 ** 40 + 5, stream=3, epoch=7, utt=2)
    for i, w in enumerate(dither_wavs()):
        eng.set_frontend(dither=0.0, **over)
        m0 = eng.debug_mfcc(w)
        assert eng.debug_frontend_route()["mfcc"] == plain
        h0 = eng.debug_mfcc_dither(w, **key)
        assert eng.debug_frontend_route()["mfcc"] == plain
        assert np.array_equal(m0.view(np.uint32), h0.view(np.uint32))
        z = eng.debug_dither_noise(key["seed"], key["stream"], key["epoch"], key["utt"], 0, m0.shape[0], L)
        for dither in (0.5, 1.0, 3.0):
            eng.set_frontend(dither=dither, **over)
            got = eng.debug_mfcc_dither(w, **key).astype(np.float64)
            assert eng.debug_frontend_route()["mfcc"] == dithered
            want = np_mfcc_dither(w, z, dither, **kw)
            err = np.abs(got - want).max()
            print("%s wav %d dither %g: |device - restatement| max %.3g (allowed %.3g)" % (route, i, dither, err, _tol(route, want)))
            assert got.shape == want.shape
            assert err <= _tol(route, want), (route, i, dither, err)
            assert np.abs(got - m0).max() > 0.0


# ------------------------------------------------------------------------------------------------------------ 2. noise
def test_dither_normals(eng):
    T, L = 300, 400
    key = (11, 4, 9, 6)   # seed, stream, epoch, utt
    z = eng.debug_dither_noise(*key, 0, T, L).astype(np.float64)
    n = z.size
    assert abs(z.mean()) <= 5.0 / math.sqrt(n)
    assert abs(z.var() - 1.0) <= 5.0 * math.sqrt(2.0 / n)
    # the two draws one waveform sample gets in neighbouring frames are independent
    a, b = z[:-1, 160:], z[1:, :L - 160]
    assert abs(np.corrcoef(a.ravel(), b.ravel())[0, 1]) <= 5.0 / math.sqrt(a.size)
    # a window into the same stream is the same stream
    assert np.array_equal(eng.debug_dither_noise(*key, 17, 5, L), z[17:22].astype(np.float32))
    for other in ((12, 4, 9, 6), (11 + 2 ** 32, 4, 9, 6), (11, 5, 9, 6), (11, 4, 10, 6), (11, 4, 9, 7)):
        zo = eng.debug_dither_noise(*other, 0, T, L)
        assert not (zo == z.astype(np.float32)).all(axis=1).any(), other
    # disjoint from the NES stream of the same seed: no row of either appears in the other
    nes = eng.debug_noise(11, 9, 4, L, T)
    zf = z.astype(np.float32)
    assert not (nes == zf).all(axis=1).any()
    nes_rows = {r.tobytes() for r in nes}
    assert not any(r.tobytes() in nes_rows for r in zf)


# -------------------------------------------------------------------------------------------------- 3. digital silence
@pytest.mark.parametrize("route", sorted(ROUTES))
def test_digital_silence(eng, route):
    over = ROUTES[route][0]
    w = np.zeros(16000, np.int16)
    eng.set_frontend(dither=0.0, **over)
    c0 = eng.debug_mfcc(w)[:, 0]
    assert np.all(c0 == np.float32(math.log(FLT_EPS)))
    eng.set_frontend(dither=1.0, **over)
    c0 = eng.debug_mfcc(w)[:, 0].astype(np.float64)
    assert c0.size == 100
    assert np.all((c0 >= math.log(230.0)) & (c0 <= math.log(570.0))), (c0.min(), c0.max())   # chi^2_399 +- 6 sigma


# ------------------------------------------------------------------------------------------------------- 4. downstream
def _oracle_feats(oracle, cfg, mf, compress):
    m = oracle.compress_roundtrip(mf) if compress else mf
    v = oracle.vad(cfg, m).astype(bool)
    return oracle.cmvn_sliding(cfg, oracle.deltas(cfg, m))[v]


@pytest.mark.parametrize("compress", [0, 1], ids=["plain", "compress_feats"])
def test_stages_behind_the_dithered_mfcc(eng, oracle, small_system, compress):
    """With dither 1 the device's features are the oracle's VAD / deltas / CMVN of the device's dithered MFCC matrix
    (tests/test_gpu_parity.py's 1e-5), and its scores the oracle's diagonal-GMM average of those features (1e-4)."""
    ubm, spk = small_system
    models = [ubm] + spk
    gc, miv, iv = stack_models(models)
    eng.set_frontend(dither=1.0, compress_feats=compress)
    eng.load_gmm(models)
    cfg = oracle.default_cfg()
    seed = 77
    for serial, w in enumerate([_wav(0, 48000), _wav(3, 100000)]):      # the second: longer than the CMVN window
        key = dict(seed=seed, stream=SCORING_STREAM, epoch=serial, utt=0)
        mf = eng.debug_mfcc_dither(w, **key)
        if compress:                                                    # (the hook returns the matrix the later stages read)
            eng.set_frontend(compress_feats=0)
            mf = eng.debug_mfcc_dither(w, **key)
            eng.set_frontend(compress_feats=1)
        fg, T = eng.debug_feats_dither(w, **key)
        assert eng.debug_frontend_route()["mfcc"] == "k_mfcc_r16<12,true,dither>"
        fo = _oracle_feats(oracle, cfg, mf, compress)
        assert T == mf.shape[0] and fg.shape == fo.shape
        assert np.abs(fg.astype(np.float64) - fo).max() <= 1e-5
        if serial == 0:
            eng.set_dither_seed(seed)
        raw, tv = eng.score_raw([w])                                    # scoring call `serial` after set_dither_seed
        assert tv[0] == fo.shape[0]
        want = [oracle.diag_gmm_loglikes(gc[m], miv[m], iv[m], fo)[1] / fo.shape[0] for m in range(len(models))]
        assert np.abs(raw[0] - np.array(want)).max() <= 1e-4


def test_ivector_chain_behind_the_dithered_mfcc(eng, oracle):
    """... and for an i-vector system: the i-vector of a dithered scoring call is the oracle's extraction from the device's
    dithered features (tests/test_gpu_ivector.py's 1e-6 of the largest entry)."""
    sy = synthetic_ivector_system(C=96, D=72, R=48, L=24, n_speakers=3, seed=11)
    sy = sy.with_enrolled(sy.enrolled, z_mean=[-30.0, -50.0, -20.0], z_std=[5.0, 8.0, 4.0])
    eng.set_frontend(dither=1.0)
    eng.load_ivector(sy, "OSI")
    ctx = oracle.IvSystemCtx(oracle.default_cfg(), sy)
    w = _wav(1, 24000)
    fg, _ = eng.debug_feats_dither(w, seed=5, stream=SCORING_STREAM, epoch=0, utt=0)
    eng.set_dither_seed(5)
    llr, tv = eng.score_raw([w])
    assert tv[0] == fg.shape[0]
    iv_o = ctx.extract(*ctx.stats(fg))
    iv_g = eng.debug_ivectors(1, sy.R)[0]
    assert np.abs(iv_g - iv_o).max() <= 1e-6 * max(1.0, np.abs(iv_o).max())
    eng.set_frontend(dither=0.0)
    llr0, _ = eng.score_raw([w])
    assert np.abs(llr - llr0).max() > 0.0


# ---------------------------------------------------------------------------------------------------------- 5. contract
def _attack(monkeypatch, fused=None, batch=None, stream=2, mfcc_f32=1):
    if batch is None:
        monkeypatch.delenv("FB_ATTACK_BATCH", raising=False)
    else:
        monkeypatch.setenv("FB_ATTACK_BATCH", batch)
    ubm, spk = synthetic_gmm_system(n_speakers=3, C=128, D=72)
    audio = synthetic_audio(6, 16000)
    e = Engine(0)
    try:
        e.set_frontend(dither=1.0, mfcc_f32=mfcc_f32)
        e.load_gmm([ubm] + spk)
        e.set_system("OSI")
        e.set_fused_chain(fused)
        e.set_dither_seed(123)
        raw, _ = e.score_raw([(audio * 32768.0).astype(np.int16)])
        sc = raw[0, 1:] - raw[0, 0]
        p = nes_params("OSI", "targeted", samples_per_draw=10, max_iter=60, target=int(np.argmax(sc)),
                       threshold=float(sc.max()) + 0.01, epsilon=0.004, max_lr=0.002, seed=11, stream=stream)
        out = e.attack(p, audio)
        assert e.debug_frontend_route()["mfcc"].endswith("dither>")
        return out
    finally:
        e.close()


def _same(a, b):
    return a[1] == b[1] and all(np.array_equal(x, y) for x, y in zip((a[0], a[2], a[3]), (b[0], b[2], b[3])))


@pytest.mark.parametrize("mfcc_f32", [0, 1], ids=["r16", "f32"])
def test_dithered_attack_depends_on_seed_and_stream_only(monkeypatch, mfcc_f32):
    ref = _attack(monkeypatch, mfcc_f32=mfcc_f32)
    assert ref[1] == 1 and 0 < ref[3].shape[0] < 60                                  # early stop reached
    assert _same(ref, _attack(monkeypatch, mfcc_f32=mfcc_f32))                       # (a) again, on another engine
    assert _same(_attack(monkeypatch, fused=True, mfcc_f32=mfcc_f32),
                 _attack(monkeypatch, fused=False, mfcc_f32=mfcc_f32))               # (b) fused and 6-launch chains
    assert _same(ref, _attack(monkeypatch, fused=True, mfcc_f32=mfcc_f32))
    assert _same(ref, _attack(monkeypatch, batch="1", mfcc_f32=mfcc_f32))            # (c) queue depth
    other = _attack(monkeypatch, stream=3, mfcc_f32=mfcc_f32)                        # (d) another stream
    assert other[3].shape != ref[3].shape or not np.array_equal(other[3], ref[3])


def test_scoring_calls_are_keyed_by_the_dither_seed_and_their_serial(eng, small_system):
    ubm, spk = small_system
    eng.set_frontend(dither=1.0)
    eng.load_gmm([ubm] + spk)
    wavs = [_wav(0, 16000), _wav(1, 24000)]
    runs = []
    for _ in range(2):
        eng.set_dither_seed(9)
        runs.append([eng.score_raw(wavs)[0] for _ in range(3)])
    for a, b in zip(*runs):
        assert np.array_equal(a, b)                                                  # (e) the same sequence, the same bits
    assert not np.array_equal(runs[0][0], runs[0][1])                                # ... and every call draws afresh
    eng.set_dither_seed(10)
    assert not np.array_equal(eng.score_raw(wavs)[0], runs[0][0])


@pytest.mark.parametrize("mfcc_f32", [0, 1], ids=["r16", "f32"])
def test_noise_of_an_utterance_does_not_depend_on_its_batch(eng, small_system, mfcc_f32):
    """(f) Three equal-length utterances (k_mfcc_f32 computes their frame records) against the same batch with the third
    one lengthened (it loads them): rows 0 and 1 agree as closely as they do at dither 0 -- measured here; 10 x that or 1e-5
    is allowed -- and another seed moves them by at least 100 x the allowance.  Dither 8 makes the effect unmistakable."""
    ubm, spk = small_system
    eng.load_gmm([ubm] + spk)
    equal = [_wav(0, 16000), _wav(1, 16000), _wav(2, 16000)]
    ragged = equal[:2] + [_wav(2, 24000)]

    def rows01(dither, seed):
        eng.set_frontend(dither=dither, mfcc_f32=mfcc_f32)
        out = []
        for batch in (equal, ragged):
            eng.set_dither_seed(seed)
            out.append(eng.score_raw(batch)[0][:2])
        return out

    a0, b0 = rows01(0.0, 1)
    allowed = max(10.0 * np.abs(a0 - b0).max(), 1e-5)
    a8, b8 = rows01(8.0, 1)
    assert eng.debug_frontend_route()["mfcc"].endswith("dither>")
    print("rows 0, 1 between the batches: dither 0 %.3g, dither 8 %.3g (allowed %.3g)" % (np.abs(a0 - b0).max(), np.abs(a8 - b8).max(), allowed))
    assert np.abs(a8 - b8).max() <= allowed
    c8, _ = rows01(8.0, 2)
    assert np.abs(c8 - a8).max(axis=1).min() >= 100.0 * allowed                       # each of the two rows moved


# -------------------------------------------------------------------------------------------------------- 6. validation
def test_set_frontend_refuses_a_bad_dither(eng):
    eng.set_frontend(dither=0.5)
    w = _wav(0, 8000)
    key = dict(seed=1, stream=0, epoch=0, utt=0)
    before = eng.debug_mfcc_dither(w, **key)
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(NativeError) as ex:
            eng.set_frontend(dither=bad)
        assert ex.value.code == FB_E_ARG
        assert eng.cfg.dither == 0.5
        assert np.array_equal(eng.debug_mfcc_dither(w, **key), before)
