"""White-box gradients on the device (fb_get_grad_wb / fb_attack_wb; the "white-box gradients" section of
include/fakebob_hip.h) against the PyTorch float64 restatement (tests/whitebox_ref.py), which tests/test_whitebox_ref_host.py
pins to the CPU oracle and to finite differences.

Three comparisons carry a tolerance, each a relative L2 error ||g - g_ref|| / ||g_ref||:
  the GMM backward hook against the closed form            measured worst MEASURED_GMM,  bar BAR_GMM
  the front-end backward hook against autograd              measured worst MEASURED_VJP,  bar BAR_VJP
  fb_get_grad_wb against the restatement's loss gradient    measured worst MEASURED_GRAD, bar BAR_GRAD
Each bar is four times the worst error measured over the listed cases on the first run on an MI355X, rounded up to one digit;
none may exceed 1e-2 (a transposition, sign, offset or missing-term error is of order 1).  Everything else is exact: the
forward is fb_get_grad's bit for bit, the gradient is bit-identical between calls and engines, and a whole attack equals
its replay on the host bit for bit.
"""
import os
import pickle

import numpy as np
import pytest

from fakebob_amd import _native as N
from fakebob_amd.engine import Engine, nes_params
from fakebob_amd.models import DiagGmm, stack_models, synthetic_audio, synthetic_gmm_system, synthetic_ubm_moments
from tests import whitebox_ref as R

pytestmark = pytest.mark.gpu

MEASURED_GMM, BAR_GMM = 2.23e-5, 9e-5        # worst: D = 72, C = 256, Tv = 257 (float32 MFMA products, float32 soft-max state)
MEASURED_VJP, BAR_VJP = 5.0e-15, 2e-14       # worst: remove_dc = 0, N = 4000 (float64 throughout)
MEASURED_GRAD, BAR_GRAD = 1.75e-4, 7e-4      # worst: full_system (C = 2048: two speakers' nearly equal posteriors cancel); small_system 2.5e-5


def rel_l2(g, ref):
    return float(np.linalg.norm(np.asarray(g, np.float64) - ref) / np.linalg.norm(ref))


def quantize(audio, bits=16):
    v = np.trunc(np.asarray(audio, np.float64) * float(2 ** (bits - 1))).astype(np.int64)
    return (v & 0xFFFF).astype(np.uint16).view(np.int16)


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


def _stack(system, task):
    ubm, spk = system
    return stack_models(spk if task == "CSI" else ([ubm] + spk if task == "OSI" else [ubm, spk[0]]))


Z_MEAN = np.array([-70.0, -71.0, -69.5])
Z_STD = np.array([1.5, 2.0, 1.2])


def _load(e, system, task):
    models = _stack(system, task)
    e.load_gmm_arrays(*models)
    if task == "CSI":
        e.set_system("CSI", Z_MEAN[:models[0].shape[0]], Z_STD[:models[0].shape[0]])
    else:
        e.set_system(task)
    return models


# ------------------------------------------------------------------------------------- 1. the GMM backward hook
def _hook_system(C, D, other_vars):
    """UBM + 3 speakers; other_vars: the speakers' variances differ from the UBM's and from each other's"""
    ubm, spk = synthetic_gmm_system(n_speakers=3, C=C, D=D)
    if other_vars:
        w, _mu, _var = synthetic_ubm_moments(C, D, 2001)
        spk = [DiagGmm.from_internal(w, (m.means() / (m.variances() * (1.0 + 0.1 * (i + 1)))).astype(np.float32),
                                     (1.0 / (m.variances() * (1.0 + 0.1 * (i + 1)))).astype(np.float32)) for i, m in enumerate(spk)]
    return stack_models([ubm] + spk)


@pytest.fixture(scope="module")
def hook_feats(eng):
    """rows of fb_debug_feats per feature dimension: 280 voiced rows of a four-second utterance"""
    out = {}
    wav = quantize(R.test_audio(64000))
    try:
        for D, order in ((72, 2), (48, 1), (24, 0)):
            eng.set_frontend(delta_order=order)
            out[D] = eng.debug_feats(wav)[0]
            assert out[D].shape[0] >= 257 and out[D].shape[1] == D
    finally:
        eng.set_frontend(delta_order=2)
    return out


W_CASES = {"one": [0.0, 0.0, -1.0, 0.0], "two": [1.0, 0.0, -1.0, 0.0], "three": [0.5, -1.0, 0.0, 0.625], "none": [0.0, 0.0, 0.0, 0.0]}
GMM_CASES = ([(72, 256, tv, "two", False) for tv in (1, 31, 32, 33, 257)] +
             [(72, 100, 33, "three", False), (48, 256, 33, "two", False), (24, 256, 33, "two", False), (24, 100, 17, "one", False),
              (72, 256, 33, "one", False), (72, 256, 33, "three", True), (72, 256, 33, "none", False), (72, 100, 257, "three", True)])


@pytest.mark.parametrize("D,C,tv,wname,other_vars", GMM_CASES)
def test_gmm_backward_hook_against_the_closed_form(eng, hook_feats, D, C, tv, wname, other_vars):
    gc, miv, iv = _hook_system(C, D, other_vars)
    if other_vars:
        assert not np.array_equal(iv[1], iv[0]) and not np.array_equal(iv[1], iv[2])
    try:
        eng.set_frontend(delta_order=D // 24 - 1)
        eng.load_gmm_arrays(gc, miv, iv)
        feats = hook_feats[D][:tv]
        w = np.array(W_CASES[wname])
        got = eng.debug_gmm_feat_grad(feats, w)
        again = eng.debug_gmm_feat_grad(feats, w)
    finally:
        eng.set_frontend(delta_order=2)
    assert np.array_equal(got.view(np.uint64), again.view(np.uint64))
    if wname == "none":
        assert not got.any()            # exact zeros
        return
    want = R.gmm_feat_grad(feats, w, gc, miv, iv)
    err = rel_l2(got, want)
    print("GMM backward D=%d C=%d Tv=%d w=%s other_vars=%s: relative L2 error %.3g" % (D, C, tv, wname, other_vars, err))
    assert np.isfinite(got).all()
    assert err < BAR_GMM


# ------------------------------------------------------------------------------------- 2. the front-end backward hook
def _zeros_audio():
    a = R.test_audio(4000)
    a[1600:2400] = 0.0
    return a


VJP_CASES = [("recipe", {}, n) for n in (200, 240, 1040, 4000, 47840, 48000, 48160, 20000)] + [
    ("snip_edges", dict(snip_edges=1), 4000), ("no_remove_dc", dict(remove_dc=0), 4000), ("no_use_energy", dict(use_energy=0), 4000),
    ("no_raw_energy", dict(raw_energy=0), 4000), ("delta_order_0", dict(delta_order=0), 4000), ("delta_order_1", dict(delta_order=1), 4000),
    ("cmn_window_20", dict(cmn_window=20), 4000)]


@pytest.mark.parametrize("name,over,n", VJP_CASES, ids=["%s-%d" % (c[0], c[2]) for c in VJP_CASES])
def test_frontend_backward_hook_against_autograd(eng, name, over, n):
    wav = quantize(R.test_audio(n))
    try:
        eng.set_frontend(**over)
        if name == "cmn_window_20":
            assert eng._num_frames(n) == 25
        feats, T = eng.debug_feats(wav)
        cot = np.random.default_rng(n + len(name)).normal(size=feats.shape)
        dwav, mask = eng.debug_frontend_vjp(wav, cot)
        want, ref_mask = R.frontend_vjp(eng.cfg, wav, cot)
    finally:
        eng.set_frontend(snip_edges=0, remove_dc=1, use_energy=1, raw_energy=1, delta_order=2, cmn_window=300)
    assert np.array_equal(mask, ref_mask) and int(mask.sum()) == feats.shape[0]
    assert np.isfinite(dwav).all()
    if T == 1:      # CMVN over one frame leaves exactly nothing: the features are constant zeros, and so is the product
        assert not want.any() and not dwav.any()
        return
    err = rel_l2(dwav, want)
    print("front-end backward %s N=%d (T=%d, Tv=%d): relative L2 error %.3g" % (name, n, T, feats.shape[0], err))
    assert err < BAR_VJP


def test_frontend_backward_with_active_floors(eng):
    """800 exact zeros in the middle: the frames inside them sit on the energy floor and on every mel floor.  The result is
    finite everywhere, and the samples that only such frames cover (frames start at 160 f - 120: those at 1640, 1800 and 1960
    lie inside the zeros, and they alone cover samples 1880 .. 2119) get exactly nothing."""
    wav = quantize(_zeros_audio())
    feats, T = eng.debug_feats(wav)
    cot = np.random.default_rng(5).normal(size=feats.shape)
    dwav, mask = eng.debug_frontend_vjp(wav, cot)
    want, ref_mask = R.frontend_vjp(eng.cfg, wav, cot)
    err = rel_l2(dwav, want)
    print("front-end backward with active floors: Tv=%d of %d, relative L2 error %.3g" % (feats.shape[0], T, err))
    assert np.array_equal(mask, ref_mask)
    assert np.isfinite(dwav).all()
    assert not dwav[1880:2120].any() and not want[1880:2120].any()
    assert err < BAR_VJP


# ------------------------------------------------------------------------------------- 3. fb_get_grad_wb
BRANCHES = [("osi_targeted_speaker", "OSI", "targeted", dict(target=1, threshold=-10.0)),
            ("osi_targeted_threshold", "OSI", "targeted", dict(target=1, threshold=10.0)),
            ("osi_untargeted", "OSI", "untargeted", dict(threshold=0.5)),
            ("csi_targeted", "CSI", "targeted", dict(target=2)),
            ("csi_untargeted", "CSI", "untargeted", dict(true=0)),
            ("sv", "SV", "untargeted", dict(threshold=0.1))]


def _ref_kw(task, kw):
    return dict(kw, z_mean=Z_MEAN, z_std=Z_STD) if task == "CSI" else kw


def _check_grad(e, system, task, attack, kw, audio, bits=16, label=""):
    models = _load(e, system, task)
    p = nes_params(task, attack, samples_per_draw=0, bits_per_sample=bits, **kw)
    grad, al, sc = e.get_grad_wb(p, audio)
    _fl, _g, al0, sc0 = e.get_grad(p, audio, want_grad=False)
    # the same forward -- ONE row scored --, bit for bit.  (Row 0 of a larger NES batch is the same function under another
    # split of the components into chunks, whose float32 partial sums merge in another order: equal bits at C = 256, 7e-8 apart
    # at C = 2048 when measured.  That is fb_get_grad against itself at two batch sizes; here it is bounded by the 1e-5 of
    # the forward comparison with the oracle.)
    assert al == al0 and np.array_equal(sc, sc0)
    for spd in (6, 50):
        _fl, _g, alb, scb = e.get_grad(nes_params(task, attack, samples_per_draw=spd, bits_per_sample=bits, **kw), audio, want_grad=False)
        print("%s: adver_loss %.17g, fb_get_grad's at samples_per_draw = %d %.17g" % (label, al, spd, alb))
        assert abs(al - alb) < 1e-5 and np.abs(sc - scb).max() < 1e-5
    zk = {} if task != "CSI" else dict(z_mean=Z_MEAN[:models[0].shape[0]], z_std=Z_STD[:models[0].shape[0]])
    r = R.loss_and_grad(e.cfg, models, task, attack, audio, bits=bits, **dict(kw, **zk))
    err = rel_l2(grad, r.grad)
    print("%s: Tv=%d, min |c0 - thr| %.3g, loss %.9g (restatement %.9g), relative L2 error %.3g" % (label, r.tv, r.margin, al, r.loss, err))
    assert r.margin > 1e-3
    assert abs(al - r.loss) < 1e-3 and np.abs(sc - r.scores).max() < 1e-3
    assert np.isfinite(grad).all()
    assert err < BAR_GRAD
    return grad


@pytest.mark.parametrize("n", [4000, 20000])
@pytest.mark.parametrize("name,task,attack,kw", BRANCHES, ids=[b[0] for b in BRANCHES])
def test_get_grad_wb_against_the_restatement(eng, small_system, name, task, attack, kw, n):
    _check_grad(eng, small_system, task, attack, kw, R.test_audio(n), label="%s N=%d" % (name, n))


def test_get_grad_wb_full_system(eng, full_system):
    _check_grad(eng, full_system, "OSI", "targeted", dict(target=3, threshold=-10.0), R.test_audio(20000), label="full_system OSI targeted")


def test_get_grad_wb_bits_per_sample_8(eng, small_system):
    audio = R.test_audio(4000)
    g8 = _check_grad(eng, small_system, "SV", "untargeted", dict(threshold=0.1), audio, bits=8, label="sv bits=8")
    g16 = _check_grad(eng, small_system, "SV", "untargeted", dict(threshold=0.1), audio, bits=16, label="sv bits=16")
    assert not np.array_equal(g8, g16)


# ------------------------------------------------------------------------------------- 4. determinism
def test_the_gradient_is_bit_identical(eng, small_system):
    audio = R.test_audio(20000)
    p = nes_params("OSI", "targeted", target=1, threshold=-10.0)
    _load(eng, small_system, "OSI")
    a = eng.get_grad_wb(p, audio)
    b = eng.get_grad_wb(p, audio)
    eng.attack(nes_params("OSI", "targeted", target=2, threshold=0.0, max_iter=2, samples_per_draw=6), R.test_audio(4000))
    c = eng.get_grad_wb(p, audio)
    fresh = Engine(0)
    try:
        _load(fresh, small_system, "OSI")
        d = fresh.get_grad_wb(p, audio)
    finally:
        fresh.close()
    for other in (b, c, d):
        assert np.array_equal(a[0].view(np.uint64), other[0].view(np.uint64)) and a[1] == other[1] and np.array_equal(a[2], other[2])


# ------------------------------------------------------------------------------------- 5. whole attacks
def replay(e, p, audio):
    """FakeBob.attack (FAKEBOB.py:157-220) on the host in numpy float64, the gradient from fb_get_grad_wb at every iterate"""
    audio = np.asarray(audio, np.float64)
    adver, grad_m, lr, ls, rows = audio.copy(), np.zeros_like(audio), p.max_lr, [], []
    lower, upper = np.clip(audio - p.epsilon, -1.0, 1.0), np.clip(audio + p.epsilon, -1.0, 1.0)
    last = p.max_iter - 1
    for it in range(p.max_iter):
        g, al, sc = e.get_grad_wb(p, adver)
        dist = np.max(np.abs(audio - adver))
        if al < 0:
            rows.append([dist, al, lr] + list(sc))
            last = it
            break
        grad_m = p.momentum * grad_m + (1.0 - p.momentum) * g
        ls = (ls + [al])[-p.plateau_length:]
        if ls[-1] > ls[0] and len(ls) == p.plateau_length:
            if lr > p.min_lr:
                lr = max(lr / p.plateau_drop, p.min_lr)
            ls = []
        adver = np.clip(adver - lr * np.sign(grad_m), lower, upper)
        rows.append([dist, al, lr] + list(sc))
    bits = p.bits_per_sample or 16
    return quantize(adver, bits), (1 if last < p.max_iter - 1 else -1), adver, np.array(rows)


ATTACKS = {
    "osi_targeted_m0.9": ("OSI", dict(attack_type="targeted", target=1, threshold=0.0, max_iter=12)),
    "csi_untargeted_m0": ("CSI", dict(attack_type="untargeted", true=1, adver_thresh=1e3, momentum=0.0, max_iter=12)),     # never stops
    # (settings fixed on the CPU with the restatement as the gradient: the loss starts at 0.254 and falls by 0.03 - 0.09 per
    #  one-LSB step; it crosses zero at iteration 6)
    "sv_stops_early": ("SV", dict(attack_type="untargeted", threshold=0.2, max_lr=2.0 ** -15, max_iter=12)),
    "sv_plateau_to_min_lr": ("SV", dict(attack_type="untargeted", threshold=1e3, max_iter=12, momentum=0.0, max_lr=2e-3,
                                        min_lr=1e-3, plateau_length=2, plateau_drop=4.0)),
    "sv_single_step": ("SV", dict(attack_type="untargeted", threshold=1e3, max_iter=1)),
}


@pytest.mark.parametrize("batch", ["1", "4"])
@pytest.mark.parametrize("case", sorted(ATTACKS))
def test_a_whole_attack_is_its_replay(eng, small_system, monkeypatch, case, batch):
    task, kw = ATTACKS[case]
    kw = dict(kw)
    p = nes_params(task, kw.pop("attack_type"), **kw)
    _load(eng, small_system, task)
    audio = R.test_audio(4000)
    monkeypatch.setenv("FB_ATTACK_BATCH", batch)
    adv, flag, adv_f, trace = eng.attack_wb(p, audio)
    secs = eng.attack_iter_seconds(trace.shape[0])
    it0 = eng.stats()["nes_iters"]
    r_adv, r_flag, r_adv_f, r_trace = replay(eng, p, audio)
    print("%s batch %s: %d rows, flag %d, loss %s, lr %s" % (case, batch, trace.shape[0], flag, trace[:, 1], trace[:, 2]))
    assert eng.stats()["nes_iters"] - it0 == trace.shape[0]
    assert trace.shape == r_trace.shape and np.array_equal(trace.view(np.uint64), r_trace.view(np.uint64))
    assert flag == r_flag and np.array_equal(adv_f.view(np.uint64), r_adv_f.view(np.uint64)) and np.array_equal(adv, r_adv)
    assert (secs > 0).all()
    if case == "sv_stops_early":        # a loose threshold: it succeeds, and the sign is right end to end
        assert flag == 1 and trace[-1, 1] < 0 and 3 <= trace.shape[0] < 12
        assert trace[1, 1] <= trace[0, 1] and trace[2, 1] <= trace[1, 1]
    if case == "sv_plateau_to_min_lr":
        assert flag == -1 and trace.shape[0] == 12 and trace[0, 2] == 2e-3 and trace[-1, 2] == 1e-3
    if case == "sv_single_step":
        assert flag == -1 and trace.shape[0] == 1
    if case == "csi_untargeted_m0":
        assert flag == -1 and trace.shape[0] == 12
    assert np.abs(adv_f - audio).max() <= p.epsilon + 1e-15


# ------------------------------------------------------------------------------------- 6. refusals
@pytest.fixture(scope="module")
def nes_baseline(small_system):
    """an fb_attack on a fresh engine: what the same call must return after every refusal"""
    e = Engine(0)
    try:
        _load(e, small_system, "OSI")
        return e.attack(NES_P, R.test_audio(4000))
    finally:
        e.close()


NES_P = nes_params("OSI", "targeted", target=1, threshold=0.0, max_iter=3, samples_per_draw=6, seed=9)
WB_P = nes_params("OSI", "targeted", target=1, threshold=0.0, max_iter=3)


def _refused(e, code, audio, p=WB_P):
    for call in (lambda: e.get_grad_wb(p, audio), lambda: e.attack_wb(p, audio)):
        with pytest.raises(N.NativeError) as ex:
            call()
        assert ex.value.code == code, str(ex.value)
    return str(ex.value)


def _same_attack(e, nes_baseline):
    got = e.attack(NES_P, R.test_audio(4000))
    for a, b in zip(got, nes_baseline):
        assert np.array_equal(a, b)


STATE_CASES = {
    "eot": (lambda e: e.set_eot(2), lambda e: e.set_eot(1), "fb_set_eot"),
    "companions": (lambda e: e.set_companions([R.test_audio(4000)]), lambda e: e.set_companions(None), "companions"),
    "input_transform": (lambda e: e.set_input_transform("qt:64"), lambda e: e.set_input_transform(None), "input-transform"),
    "air_channel": (lambda e: e.set_air_channel("t60:100-200,drr:6,taps:256,delay:8"), lambda e: e.set_air_channel(None), "air channel"),
    "codec": (lambda e: e.set_codec("ulaw"), lambda e: e.set_codec(None), "codec"),
    "feature_compression": (lambda e: e.set_feature_compression(0.5, 2), lambda e: e.set_feature_compression(None), "feature compression"),
    "dither": (lambda e: e.set_frontend(dither=1.0), lambda e: e.set_frontend(dither=0.0), "dither"),
}


@pytest.mark.parametrize("case", sorted(STATE_CASES))
def test_refusals_of_a_defended_victim(eng, small_system, nes_baseline, case):
    on, off, word = STATE_CASES[case]
    _load(eng, small_system, "OSI")
    audio = R.test_audio(4000)
    on(eng)
    try:
        msg = _refused(eng, N.FB_E_STATE, audio)
    finally:
        off(eng)
    assert word in msg
    _same_attack(eng, nes_baseline)
    assert np.isfinite(eng.get_grad_wb(WB_P, audio)[0]).all()


def test_refusal_of_an_ivector_system(eng, small_system, nes_baseline):
    from fakebob_amd.models import synthetic_ivector_system
    sy = synthetic_ivector_system(C=64, D=72, R=32, L=16, n_speakers=2, seed=4)
    eng.load_ivector(sy, "OSI")
    assert "i-vector" in _refused(eng, N.FB_E_STATE, R.test_audio(4000))
    _load(eng, small_system, "OSI")
    _same_attack(eng, nes_baseline)


def test_argument_refusals(eng, small_system, nes_baseline):
    _load(eng, small_system, "OSI")
    audio = R.test_audio(4000)
    assert "one frame" in _refused(eng, N.FB_E_ARG, audio[:40])
    assert "target" in _refused(eng, N.FB_E_ARG, audio, nes_params("OSI", "targeted", target=3, max_iter=3))
    assert "task" in _refused(eng, N.FB_E_ARG, audio, nes_params("SV", "targeted", max_iter=3))
    assert "bits_per_sample" in _refused(eng, N.FB_E_ARG, audio, nes_params("OSI", "targeted", target=1, max_iter=3, bits_per_sample=17))
    _load(eng, small_system, "CSI")
    assert "true label" in _refused(eng, N.FB_E_ARG, audio, nes_params("CSI", "untargeted", true=7, max_iter=3))
    _load(eng, small_system, "OSI")
    with pytest.raises(N.NativeError) as ex:
        eng.attack_wb(nes_params("OSI", "targeted", target=1, max_iter=0), audio)
    assert ex.value.code == N.FB_E_ARG
    for call in (lambda: eng.get_grad_wb(WB_P, np.zeros(4000)), lambda: eng.attack_wb(WB_P, np.zeros(4000))):
        with pytest.raises(N.NativeError) as ex:
            call()
        assert ex.value.code == N.FB_E_NO_VOICED
    _same_attack(eng, nes_baseline)


# ------------------------------------------------------------------------------------- 7. PGD and the driver
def test_pgd_returns_fakebobs_pair_and_checkpoint(small_system, tmp_path):
    from fakebob_amd.attack import FakeBob
    from fakebob_amd.pgd import PGD
    from fakebob_amd.systems import gmm_SV
    ubm, spk = small_system
    model = gmm_SV(str(tmp_path / "sv"), ["spk0", "utt0", spk[0], 0.0, 1.0], ubm, pre_model_dir=str(tmp_path), threshold=0.0)
    audio = R.test_audio(4000)
    pgd = PGD("SV", "targeted", model, max_iter=12, max_lr=2.0 ** -15, verbose=False)
    cp = str(tmp_path / "pgd.cp")
    adv, flag = pgd.attack(audio, cp, threshold=0.2)
    fb = FakeBob("SV", "targeted", model, max_iter=2, samples_per_draw=6, seed=1, verbose=False)
    cp_fb = str(tmp_path / "fb.cp")
    adv_fb, flag_fb = fb.attack(audio, cp_fb, threshold=1e3)
    assert adv.dtype == adv_fb.dtype == np.int16 and adv.shape == adv_fb.shape == (4000, 1) and flag == 1 and flag_fb == -1
    with open(cp, "rb") as r:
        rows = pickle.load(r)
    with open(cp_fb, "rb") as r:
        rows_fb = pickle.load(r)
    assert 3 <= len(rows) < 12 and rows[-1][1][0] < 0 and rows[-1][3] == 0.0
    for row in rows:
        assert [type(x) for x in row] == [type(x) for x in rows_fb[0]] and len(row) == 4
        assert row[1].shape == rows_fb[0][1].shape and np.shape(row[2]) == np.shape(rows_fb[0][2])
    g, al, sc = pgd.get_grad(audio)
    assert g.shape == (4000, 1) and al.shape == (1,) and np.ndim(sc) == 0
    # the same trajectory as the engine's own call
    adv2, flag2, _f, trace2 = model.engine.attack_wb(pgd._params(), audio)
    assert np.array_equal(adv2, adv[:, 0]) and flag2 == flag and len(rows) == trace2.shape[0]


def test_attack_main_pgd_on_the_synthetic_site(tmp_path, capsys):
    from fakebob_amd import attack_main as AM
    from fakebob_amd.systems import gmm_OSI
    from tests.test_gpu_driver import _site
    ids, _ubm, _spk = _site(tmp_path)
    ml = AM.load_spk_models(str(tmp_path / "model"), ids, "gmm")
    probe = gmm_OSI(str(tmp_path / "probe"), ml, str(tmp_path / "pre-models" / "final.dubm"), pre_model_dir=str(tmp_path / "pre-models"),
                    threshold=0.0)
    voices = AM.collect_voices(str(tmp_path / "data" / "illegal-set"))
    thr = float(probe.score([v[2] for v in voices]).max()) + 0.002
    site = ["--model_dir", str(tmp_path / "model"), "--pre_model_dir", str(tmp_path / "pre-models"), "--test_dir",
            str(tmp_path / "data" / "test-set"), "--illegal_dir", str(tmp_path / "data" / "illegal-set"), "--out_dir", str(tmp_path / "out")]
    argv = ["-spk_id"] + ids + ["-archi", "gmm", "-task", "OSI", "-type", "targeted", "-thresh", str(thr), "-max_iter", "8", "--attack",
                                "pgd", "--streams", "1", "--seed", "7"] + site
    np.random.seed(3)
    g, results, _thr = AM.main(argv)
    out = capsys.readouterr().out
    assert "load data done, total num: 12" in out and "attack successful rate" in out
    assert g[1] == 12 and len(results) == 12 and g[2] > 0
    n = 0
    for root, _dirs, files in os.walk(str(tmp_path / "out" / "checkpoint" / "gmm-OSI-targeted")):
        for f in files:
            with open(os.path.join(root, f), "rb") as r:
                rows = pickle.load(r)
            assert 1 <= len(rows) <= 8 and len(rows[0]) == 4
            n += 1
    assert n == 12
    for extra in (["--eot-size", "2"], ["--companions", "1"], ["--input-transform", "ms:7"], ["--codec", "ulaw"], ["--feco", "0.5"],
                  ["--air-channel", "t60:200-600"], ["--dither", "1.0"], ["-archi", "iv"]):
        with pytest.raises(SystemExit):
            AM.main(argv + extra)
    capsys.readouterr()
