"""The device front end at Kaldi's other options (tests/test_oracle_frontend_options.py pins the oracle there): MFCC and
compacted features against the oracle, a ragged score_raw batch with one utterance longer than the CMVN window, one
get_grad, and the three post-MFCC chains giving the same bits.  Every option set is read from Kaldi conf text, and
every case asserts which kernels ran (Engine.debug_frontend_route)."""
import numpy as np
import pytest

from fakebob_amd._native import FB_E_ARG, NativeError
from fakebob_amd.engine import Engine, nes_params
from fakebob_amd.models import stack_models, synthetic_audio, synthetic_gmm_system
from tests.test_oracle_frontend_options import OPTION_SETS, overrides

pytestmark = pytest.mark.gpu
SCORE_TOL = 1e-4
# |device - oracle| of MFCC and features, absolute, as tests/test_gpu_configs.py holds them.  (Measured on an MI355X at
# every option set below: 0 -- the float64-between-storage-points kernels and the float32 twin round as the oracle does.)
FEAT_TOL = 2e-5

CMN_SETS = [("cmn_%d" % w, dict(cmn_window=w)) for w in (1, 2, 3, 101, 600)]
SETS = [(c[0], overrides(c)) for c in OPTION_SETS] + CMN_SETS


def _wav(utt, n):
    return (synthetic_audio(utt, n) * 32768.0).astype(np.int16)


def _wavs():
    # 150 / 50 / 350 frames: the last one is longer than the recipe's CMVN window (k_vad, k_deltas, k_cmvn_sliding)
    return [_wav(0, 24000), _wav(1, 8000), _wav(2, 56000)]


def _mfcc_kernel(over):
    if over.get("frame_length", 400) % 2:
        return "k_mfcc"
    return "k_mfcc_r16<12,%s>" % ("true" if over.get("raw_energy", 1) else "false")


def _feats_route(over, T):
    if T > over.get("cmn_window", 300):
        return "separate+sliding"
    return "split"


@pytest.mark.parametrize("name,over", SETS, ids=[s[0] for s in SETS])
def test_frontend_options_against_the_oracle(oracle, monkeypatch, name, over):
    for k in ("FB_NO_FUSE", "FB_VAD_WHOLE", "FB_FUSE_PARTS"):
        monkeypatch.delenv(k, raising=False)
    cfg = oracle.default_cfg(**over)
    e = Engine(0)
    try:
        e.set_frontend(**over)
        D = e.feat_dim
        wavs = _wavs()
        for w in wavs:
            mg, mo = e.debug_mfcc(w), oracle.mfcc(cfg, w)
            assert mg.shape == mo.shape
            assert np.abs(mg.astype(np.float64) - mo).max() <= FEAT_TOL, name
            fg, Tg = e.debug_feats(w)
            fo, To = oracle.frontend(cfg, w)
            assert Tg == To and fg.shape == fo.shape, (name, fg.shape, fo.shape)      # identical VAD decisions
            assert np.abs(fg.astype(np.float64) - fo).max() <= FEAT_TOL, name
            r = e.debug_frontend_route()
            assert r["mfcc"] == _mfcc_kernel(over) and r["t_max"] == To and r["B"] == 1
            assert r["chain"] == _feats_route(over, To) and r["compress"] is None, (name, r)
        # the split, the whole and the unfused chain: identical bits, on an utterance inside the window (none fits the
        # windows of 1 .. 3 frames: every chain there is the separate one)
        fits = [x for x in wavs[:2] if oracle.num_frames(cfg, x.size) <= over.get("cmn_window", 300)]
        got = {}
        for chain, env in (("split", {}), ("whole", {"FB_VAD_WHOLE": "1"}), ("vad+delta_cmvn", {"FB_NO_FUSE": "1"})):
            if not fits:
                break
            for k in ("FB_NO_FUSE", "FB_VAD_WHOLE"):
                monkeypatch.delenv(k, raising=False)
            for k, v in env.items():
                monkeypatch.setenv(k, v)
            got[chain] = e.debug_feats(fits[0])[0]
            assert e.debug_frontend_route()["chain"] == chain, (name, chain)
        for k in ("FB_NO_FUSE", "FB_VAD_WHOLE"):
            monkeypatch.delenv(k, raising=False)
        assert len(got) == (3 if fits else 0)
        for chain, f in got.items():
            assert np.array_equal(f.view(np.uint32), got["split"].view(np.uint32)), (name, chain)
        if D > 80:                                     # accepted by fb_set_frontend, refused by fb_load_gmm
            ubm, spk = synthetic_gmm_system(n_speakers=2, C=32, D=D)
            with pytest.raises(NativeError):
                e.load_gmm([ubm] + spk)
            return
        ubm, spk = synthetic_gmm_system(n_speakers=2, C=256, D=D)
        models = [ubm] + spk
        e.load_gmm(models)
        gc, miv, iv = stack_models(models)
        batch = wavs + [_wav(5, 112000)]               # 700 frames: longer than every window of these sets (600 included)
        raw_g, tv_g = e.score_raw(batch)
        raw_o, tv_o = oracle.gmm_score_batch(cfg, batch, gc, miv, iv, nthreads=8)
        assert np.array_equal(tv_g, tv_o)
        assert np.abs(raw_g - raw_o).max() <= SCORE_TOL, name
        r = e.debug_frontend_route()
        assert r["B"] == 4 and r["t_max"] == 700 - (2 if over.get("snip_edges") else 0)
        assert r["chain"] == "separate+sliding" and r["mfcc"] == _mfcc_kernel(over)
        e.set_system("OSI")
        ctx = oracle.GmmSystemCtx(cfg, "OSI", gc, miv, iv, nthreads=8)
        audio = synthetic_audio(4, 16000)
        kw = dict(target=1, threshold=0.05)
        pg = nes_params("OSI", "targeted", samples_per_draw=6, seed=5, stream=2, **kw)
        po = oracle.nes_params("OSI", "targeted", ctx.S, samples_per_draw=6, **kw)
        flg, gg, alg, scg = e.get_grad(pg, audio, it=1)
        flo, go, alo, sco = oracle.get_grad(po, ctx.fn, ctx.ctx, audio, seed=5, it=1, stream=2)
        assert abs(alg - alo) <= SCORE_TOL and abs(flg - flo) <= SCORE_TOL
        assert np.abs(scg[:ctx.S] - sco).max() <= SCORE_TOL
        assert np.abs(gg - go).max() <= SCORE_TOL * 6.0 / pg.sigma
        r = e.debug_frontend_route()
        assert r["B"] == 7 and r["chain"] == _feats_route(over, r["t_max"]), (name, r)
    finally:
        e.close()


F32_SETS = [s for s in SETS if s[1].get("raw_energy", 1) and s[1].get("frame_length", 400) % 2 == 0]


@pytest.mark.parametrize("name,over", F32_SETS, ids=[s[0] for s in F32_SETS])
def test_frontend_options_float32_mfcc_bit_for_bit(oracle, name, over):
    """k_mfcc_f32 at the same options: the MFCC matrix bit for bit equal to the oracle's float32 twin, and the features
    within 2e-5."""
    cfg = oracle.default_cfg(mfcc_f32=1, **over)
    e = Engine(0)
    try:
        e.set_frontend(mfcc_f32=1, **over)
        for w in _wavs():
            mg, mo = e.debug_mfcc(w), oracle.mfcc(cfg, w)
            assert mg.shape == mo.shape and np.array_equal(mg.view(np.uint32), mo.view(np.uint32)), name
            assert e.debug_frontend_route()["mfcc"] == "k_mfcc_f32<12>"
            fg, Tg = e.debug_feats(w)
            fo, To = oracle.frontend(cfg, w)
            assert Tg == To and fg.shape == fo.shape
            assert np.abs(fg.astype(np.float64) - fo).max() <= FEAT_TOL, name
    finally:
        e.close()


def test_not_raw_energy_short_window_and_f32_short_window_routes(oracle):
    """The instantiations for frames of fewer than 384 samples: k_mfcc_r16<0, *> and k_mfcc_f32<0>."""
    w = _wav(0, 24000)
    for over, kernel in ((dict(frame_length=320, raw_energy=0, snip_edges=1), "k_mfcc_r16<0,false>"),
                         (dict(frame_length=320, remove_dc=0, energy_floor=5e8), "k_mfcc_r16<0,true>"),
                         (dict(frame_length=320, mfcc_f32=1, snip_edges=1, preemph=0.5), "k_mfcc_f32<0>")):
        cfg = oracle.default_cfg(**over)
        e = Engine(0)
        try:
            e.set_frontend(**over)
            mg, mo = e.debug_mfcc(w), oracle.mfcc(cfg, w)
            assert e.debug_frontend_route()["mfcc"] == kernel
            if over.get("mfcc_f32"):
                assert np.array_equal(mg.view(np.uint32), mo.view(np.uint32))
            else:
                assert np.abs(mg.astype(np.float64) - mo).max() <= FEAT_TOL
        finally:
            e.close()


def test_meaningless_options_are_refused_and_the_previous_configuration_stays(oracle, small_system):
    """cmn_window < 1 (the sliding mean divided by an empty window: NaN features, scored), vad_frames_context < 0, and a
    mel bin that covers no FFT bin are refused; the engine keeps computing with its previous configuration."""
    ubm, spk = small_system
    e = Engine(0)
    try:
        e.set_frontend(cmn_window=101)
        e.load_gmm([ubm] + spk)
        wavs = _wavs()
        before = e.score_raw(wavs)
        feats = e.debug_feats(wavs[2])[0]
        for over, why in ((dict(cmn_window=0), "cmn_window 0 < 1"), (dict(cmn_window=-1), "cmn_window -1 < 1"),
                          (dict(vad_frames_context=-1), "vad_frames_context -1 < 0"),
                          (dict(num_mel_bins=128), "covers no FFT bin"),
                          (dict(num_mel_bins=40, high_freq=200.0), "covers no FFT bin")):
            with pytest.raises(NativeError, match=why) as ei:         # each refused by its own check
                e.set_frontend(**over)
            assert ei.value.code == FB_E_ARG
            with pytest.raises(ValueError):
                oracle.default_cfg(**over)
            assert e.cfg.cmn_window == 101 and e.cfg.vad_frames_context == 2 and e.cfg.num_mel_bins == 30
        after = e.score_raw(wavs)
        assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
        assert np.array_equal(e.debug_feats(wavs[2])[0], feats) and np.all(np.isfinite(feats))
        gc, miv, iv = stack_models([ubm] + spk)
        raw_o, _ = oracle.gmm_score_batch(oracle.default_cfg(cmn_window=101), wavs, gc, miv, iv, nthreads=8)
        assert np.abs(after[0] - raw_o).max() <= SCORE_TOL
    finally:
        e.close()


@pytest.mark.parametrize("over", [dict(preemph=1.5), dict(preemph=-0.5), dict(num_mel_bins=2, num_ceps=2)],
                         ids=["preemph_1.5", "preemph_-0.5", "two_mel_bins"])
def test_options_kaldi_refuses_but_the_oracle_computes_are_accepted(oracle, over):
    """Kaldi refuses a pre-emphasis outside [0, 1] and fewer than 3 mel bins; the oracle computes finite results there
    (tests/test_oracle_frontend_options.py pins them against numpy), so the engine accepts them and must agree."""
    cfg = oracle.default_cfg(**over)
    e = Engine(0)
    try:
        e.set_frontend(**over)
        for w in _wavs():
            mg, mo = e.debug_mfcc(w), oracle.mfcc(cfg, w)
            assert mg.shape == mo.shape and np.all(np.isfinite(mg))
            assert np.abs(mg.astype(np.float64) - mo).max() <= FEAT_TOL
            fg, Tg = e.debug_feats(w)
            fo, To = oracle.frontend(cfg, w)
            assert Tg == To and fg.shape == fo.shape and np.all(np.isfinite(fg))
            assert np.abs(fg.astype(np.float64) - fo).max() <= FEAT_TOL
    finally:
        e.close()
