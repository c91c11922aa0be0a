"""Kaldi's dither, host side: the option's way from Kaldi conf text and the system constructors into fb_frontend_cfg, and
the float64 numpy restatement of dithered compute-mfcc-feats that tests/test_gpu_dither.py judges the device with --
validated here, at dither 0, against the CPU oracle before it judges anything."""
import warnings

import numpy as np
import pytest

from fakebob_amd import _native
from fakebob_amd.config import frontend_overrides
from fakebob_amd.models import DiagGmm, synthetic_audio, synthetic_ubm_moments

FLT_EPS = float(np.finfo(np.float32).eps)
STOCK_MFCC_CONF = "--sample-frequency=16000\n--frame-length=25 # the default is 25\n--low-freq=20\n--high-freq=7600\n--num-mel-bins=30\n--num-ceps=24\n--snip-edges=false\n"


def np_mfcc_dither(wav, z=None, dither=0.0, L=400, shift=160, P=512, nb=30, nc=24, lo=20.0, hi=7600.0, fs=16000.0, pre=0.97,
                   lift=22.0, snip_edges=False, remove_dc=True, use_energy=True, raw_energy=True, energy_floor=0.0):
    """np_mfcc of tests/test_oracle_frontend.py with Kaldi's dither: after a frame is extracted (reflection included) and
    before DC removal, raw energy, pre-emphasis and the window, sample i of frame t becomes x + dither * z[t, i] -- z is
    (T, L), one normal per (frame, sample-in-frame), NOT per waveform sample.  Float64 throughout."""
    wav = wav.astype(np.float64)
    n = wav.size
    if snip_edges:
        T = 0 if n < L else 1 + (n - L) // shift
        idx = (np.arange(T)[:, None] * shift) + np.arange(L)[None, :]
    else:
        T = (n + shift // 2) // shift
        idx = (np.arange(T)[:, None] * shift + shift // 2 - L // 2) + np.arange(L)[None, :]
    while ((idx < 0) | (idx >= n)).any():          # Kaldi reflects repeatedly for very short waves
        idx = np.where(idx < 0, -idx - 1, idx)
        idx = np.where(idx >= n, 2 * n - 1 - idx, idx)
    fr = wav[idx]
    if dither != 0.0:
        z = np.asarray(z)
        assert z.shape == (T, L)
        fr = fr + float(dither) * z.astype(np.float64)
    if remove_dc:
        fr = fr - fr.mean(axis=1, keepdims=True)
    log_e = np.log(np.maximum((fr ** 2).sum(axis=1), FLT_EPS))
    fr = np.concatenate([fr[:, :1] * (1 - pre), fr[:, 1:] - pre * fr[:, :-1]], axis=1)
    win = (0.5 - 0.5 * np.cos(2 * np.pi * np.arange(L) / (L - 1))) ** 0.85
    fr = fr * win.astype(np.float32).astype(np.float64)
    if not raw_energy:
        log_e = np.log(np.maximum((fr ** 2).sum(axis=1), FLT_EPS))
    if energy_floor > 0.0:
        log_e = np.maximum(log_e, np.log(energy_floor))
    spec = np.abs(np.fft.rfft(fr, n=P, axis=1)) ** 2
    mel = lambda f: 1127.0 * np.log(1.0 + f / 700.0)
    edges = np.linspace(mel(lo), mel(hi if hi > 0 else fs / 2 + hi), nb + 2)
    fmel = mel(np.arange(P // 2) * fs / P)
    W = np.zeros((nb, P // 2 + 1))
    for b in range(nb):
        l, c, r = edges[b], edges[b + 1], edges[b + 2]
        up = (fmel - l) / (c - l)
        dn = (r - fmel) / (r - c)
        w = np.where(fmel <= c, up, dn)
        W[b, :P // 2] = np.where((fmel > l) & (fmel < r), w, 0.0).astype(np.float32)
    lm = np.log(np.maximum(spec @ W.T, FLT_EPS))
    k = np.arange(nc)[:, None]
    nn = np.arange(nb)[None, :]
    dct = np.sqrt(2.0 / nb) * np.cos(np.pi / nb * (nn + 0.5) * k)
    dct[0] = np.sqrt(1.0 / nb)
    cep = lm @ dct.astype(np.float32).astype(np.float64).T
    if lift != 0.0:
        cep = cep * (1.0 + 0.5 * lift * np.sin(np.pi * np.arange(nc) / lift)).astype(np.float32)
    if use_energy:
        cep[:, 0] = log_e
    return cep


def dither_wavs():
    """speech-like, Gaussian and full-scale random int16 inputs, and a short wave whose every frame reflects"""
    rng = np.random.default_rng(3)
    return [(synthetic_audio(0, 16000) * 32768).astype(np.int16),
            (rng.normal(size=8000) * 3000).astype(np.int16),
            rng.integers(-32768, 32767, size=4321).astype(np.int16),
            (rng.normal(size=250) * 2000).astype(np.int16)]


def test_restatement_at_dither_0_matches_the_oracle(oracle):
    cfg = oracle.default_cfg()
    for w in dither_wavs() + [np.zeros(1600, np.int16)]:
        got = oracle.mfcc(cfg, w).astype(np.float64)
        want = np_mfcc_dither(w)
        assert got.shape == want.shape
        assert np.abs(got - want).max() <= 3e-6 * max(1.0, np.abs(want).max())


def test_restatement_adds_the_noise_per_frame_and_sample():
    """one unit of noise on sample 0 of frame 1 alone moves frame 1 and no other, although frames 0 .. 2 share that
    waveform sample"""
    w = dither_wavs()[0][:1600]
    T = 10
    z = np.zeros((T, 400), np.float32)
    base = np_mfcc_dither(w, z, 1.0)
    assert np.array_equal(base, np_mfcc_dither(w))
    z[1, 0] = 1.0
    moved = np.abs(np_mfcc_dither(w, z, 50.0) - base).max(axis=1)
    assert moved[1] > 0 and moved[0] == 0 and np.all(moved[2:] == 0)


# ------------------------------------------------------------------------------------------ conf text -> overrides
def test_default_output_and_warning_are_unchanged():
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        o = frontend_overrides(STOCK_MFCC_CONF)
    assert o == {"sample_freq": 16000.0, "frame_length": 400, "padded_length": 512, "low_freq": 20.0, "high_freq": 7600.0,
                 "num_mel_bins": 30, "num_ceps": 24, "snip_edges": 0}
    assert [str(w.message) for w in rec] == [
        "Kaldi would run with dither=1 (Kaldi's default, mfcc.conf does not set it): its features are random at the 1-LSB "
        "level; the engine always uses dither=0, so scores differ from a Kaldi run by that noise"]
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        o = frontend_overrides("--dither=0.5")
    assert o == {}
    assert [str(w.message) for w in rec] == [
        "Kaldi would run with dither=0.5 (set in mfcc.conf): its features are random at the 1-LSB level; the engine always "
        "uses dither=0, so scores differ from a Kaldi run by that noise"]
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        assert frontend_overrides("--dither=0") == {}
    assert not rec


def test_opt_in_returns_the_configured_dither_without_a_warning():
    fields = {f[0] for f in _native.FrontendCfg._fields_}
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        stock = frontend_overrides(STOCK_MFCC_CONF, dither="conf")
        half = frontend_overrides(STOCK_MFCC_CONF + "--dither=0.5\n", dither="conf")
        num = frontend_overrides(STOCK_MFCC_CONF + "--dither=0.5\n", dither=2)
        off = frontend_overrides(STOCK_MFCC_CONF, dither=0)
    assert stock["dither"] == 1.0 and half["dither"] == 0.5 and num["dither"] == 2.0 and off["dither"] == 0.0
    for o in (stock, half, num, off):
        assert set(o) <= fields
        assert {k: v for k, v in o.items() if k != "dither"} == {k: v for k, v in stock.items() if k != "dither"}
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            frontend_overrides("", dither=bad)


def test_dither_is_the_last_double_of_the_struct():
    assert _native.FrontendCfg._fields_[-1][0] == "dither"
    assert _native.FrontendCfg._fields_[-1][1].__name__ == "c_double"
    assert {"fb_set_dither_seed", "fb_debug_dither_noise", "fb_debug_mfcc_dither", "fb_debug_feats_dither"} <= set(_native.EXPORTS)


# ------------------------------------------------------------------------------------------ system constructors
class FakeEngine(object):
    """Captures what the constructors hand to the engine (as tests/test_host_api.py's)."""

    def __init__(self):
        self.frontend = []
        self.task = None

    def set_frontend(self, **kw):
        self.frontend.append(dict(kw))

    def load_gmm(self, models):
        self.n_models = len(models)

    def set_system(self, task, zm=None, zs=None):
        self.task = task

    def load_ivector(self, system, task):
        self.task, self.n_models = task, system.S


def _dummy_gmm(seed):
    w, mu, var = synthetic_ubm_moments(4, 72, seed=seed)
    return DiagGmm.from_moments(w, mu, var)


def _gmm_systems(tmp_path, **kw):
    from fakebob_amd.systems import gmm_CSI, gmm_OSI, gmm_SV
    ml = [["s%d" % i, "u%d" % i, _dummy_gmm(i), 0.0, 1.0] for i in range(3)]
    ubm = _dummy_gmm(99)
    return [gmm_OSI(str(tmp_path / "o"), ml, ubm, pre_model_dir=str(tmp_path), engine=FakeEngine(), **kw),
            gmm_CSI(str(tmp_path / "c"), ml, pre_model_dir=str(tmp_path), engine=FakeEngine(), **kw),
            gmm_SV(str(tmp_path / "s"), ml[0], ubm, pre_model_dir=str(tmp_path), engine=FakeEngine(), **kw)]


def _iv_systems(tmp_path, **kw):
    from fakebob_amd.models import synthetic_ivector_system
    from fakebob_amd.systems import iv_CSI, iv_OSI, iv_SV
    sy = synthetic_ivector_system(C=8, D=72, R=6, L=4, n_speakers=2, seed=1)
    ml = []
    for i in range(2):
        p = tmp_path / ("e%d.npy" % i)
        np.save(str(p), sy.enrolled[i])
        ml.append(["s%d" % i, "u%d" % i, sy.enrolled[i], 0.0, 1.0])
    return [iv_OSI(str(tmp_path / "io"), ml, pre_model_dir=str(tmp_path), engine=FakeEngine(), system=sy, **kw),
            iv_CSI(str(tmp_path / "ic"), ml, pre_model_dir=str(tmp_path), engine=FakeEngine(), system=sy, **kw),
            iv_SV(str(tmp_path / "is"), ml[0], pre_model_dir=str(tmp_path), engine=FakeEngine(), system=sy, **kw)]


def _handed(system):
    merged = {}
    for kw in system.engine.frontend:
        merged.update(kw)
    return merged


@pytest.mark.parametrize("make", [_gmm_systems, _iv_systems], ids=["gmm", "iv"])
def test_system_classes_hand_dither_through(make, tmp_path, monkeypatch):
    monkeypatch.delenv("FB_DITHER", raising=False)
    for s in make(tmp_path):                                   # not asked for: the engine's dither is not touched
        assert "dither" not in _handed(s)
    for s in make(tmp_path, dither=0.5):
        assert _handed(s)["dither"] == 0.5
    for s in make(tmp_path, dither="conf"):                    # no conf directory: Kaldi's default
        assert _handed(s)["dither"] == 1.0
    monkeypatch.setenv("FB_DITHER", "2")
    for s in make(tmp_path):
        assert _handed(s)["dither"] == 2.0
    for s in make(tmp_path, dither=0):                         # the keyword wins over the environment
        assert _handed(s)["dither"] == 0.0


def test_gmm_systems_read_the_configured_dither(tmp_path, monkeypatch):
    monkeypatch.delenv("FB_DITHER", raising=False)
    (tmp_path / "conf").mkdir()
    (tmp_path / "conf" / "mfcc.conf").write_text(STOCK_MFCC_CONF + "--dither=0.25\n")
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        for s in _gmm_systems(tmp_path, dither="conf"):
            assert _handed(s)["dither"] == 0.25 and _handed(s)["num_mel_bins"] == 30
    with pytest.warns(UserWarning, match="the engine always uses dither=0"):
        systems = _gmm_systems(tmp_path)
    for s in systems:
        assert "dither" not in _handed(s)


def test_attack_main_takes_the_dither_options(monkeypatch):
    import fakebob_amd.attack_main as am
    seen = {}

    class Stop(Exception):
        pass

    def fake_make_model(architecture, task, model_list, pre_model_dir, threshold, group_id, dither=None):
        seen["dither"] = dither
        raise Stop()

    monkeypatch.setattr(am, "make_model", fake_make_model)
    monkeypatch.setattr(am, "load_spk_models", lambda *a: [])
    with pytest.raises(Stop):
        am.main(["-spk_id", "a", "--dither", "conf", "--dither-seed", "7", "--streams", "1"])
    assert seen["dither"] == "conf"
