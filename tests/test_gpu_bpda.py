"""White-box gradients through a defended victim on the device (fb_set_wb_bpda, fb_get_grad_wb_iter; "Defended victims: BPDA
and EOT" in include/fakebob_hip.h) against the PyTorch float64 restatement tests/bpda_ref.py, which tests/test_bpda_ref_host.py
pins to the numpy twins, to the adjoint identity and to finite differences.

Two comparisons carry a tolerance, each a relative L2 error ||g - g_ref|| / ||g_ref||:
  fb_debug_defence_vjp against autograd through the surrogate     measured worst MEASURED_VJP,  bar BAR_VJP
  fb_get_grad_wb(_iter) against the restatement's loss gradient   measured worst MEASURED_GRAD, bar BAR_GRAD
Each bar is four times the worst error measured over the listed cases on the first run on an MI355X, rounded up to one digit;
none may exceed 1e-2.  Everything else is exact: the transformed rows equal the numpy twins, integer-tap
chains transpose exactly, the forward is fb_get_grad's bit for bit, the gradient is bit-identical between engines, and a whole
attack equals its replay on the host.

The air channel's transpose is not in this version: it stays refused with the switch on (section 7 below)."""
import os
import pickle

import numpy as np
import pytest

from fakebob_amd import _native as N
from fakebob_amd import input_transform as IT
from fakebob_amd.engine import Engine, nes_params
from tests import bpda_ref as B
from tests import whitebox_ref as R
from tests.test_gpu_whitebox import Z_MEAN, Z_STD, _load, quantize, rel_l2

pytestmark = pytest.mark.gpu

MEASURED_VJP, BAR_VJP = 1.03e-15, 5e-15     # worst: ds:2:511 (two 511-tap transposes), N = 9000; float64 throughout
MEASURED_GRAD, BAR_GRAD = 3.22e-5, 2e-4     # worst: ds:2, OSI targeted (the GMM backward's float32 products: 2.5e-5 undefended)

SEED, STREAM = 77, 3


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


def _clear(e):
    e.set_input_transform(None)
    e.set_codec(None)
    e.set_eot(1)
    e.set_wb_bpda(False)


def _chain(spec):
    return [tuple(s) for s in IT.parse(spec)]


def _normals(e, chain, n, it, replica):
    """the normals the noise stages of `chain` draw for (SEED, STREAM, epoch it, utterance 0, replica): the generator's own hook"""
    return {s: e.debug_tf_noise(SEED, STREAM, it, 0, replica, s, 0, n) for s, st in enumerate(chain) if st[0] == B.NOISE}


def _full_range(n):
    a = R.test_audio(n)
    w = np.clip(np.rint(a / np.abs(a).max() * 40000.0), -32768, 32767).astype(np.int16)      # peaks flattened at a rail ...
    flat = np.flatnonzero(np.abs(w.astype(np.int32)) >= 32767)
    w[flat[::2]] = -w[flat[::2]].astype(np.int32).clip(-32767, 32767)                              # ... every second one at the other
    return w


FIR5_GAIN2 = IT.fir(IT.lowpass_taps(4000.0, 5, gain=2.0))
# (id, chain, codec, n, full-range audio, EOT size, exact: masks and copies only -- a median's gather adds up to k cotangents)
HOOK_CASES = [
    ("qt64", "qt:64", None, 4000, False, 1, True),
    ("ms3", "ms:3", None, 4000, False, 1, False),
    ("ms31-9000", "ms:31", None, 9000, False, 1, False),
    ("fir5", IT.lowpass(4000.0, 5), None, 4000, False, 1, False),
    ("fir101", IT.lowpass(4000.0, 101), None, 4000, False, 1, False),
    ("fir511-9000", IT.lowpass(4000.0, 511), None, 9000, False, 1, False),
    ("ds2", "ds:2", None, 4000, False, 1, False),
    ("ds2-9001", "ds:2", None, 9001, False, 1, False),
    ("ds2x511-9000", "ds:2:511", None, 9000, False, 1, False),          # H = 510: more than 64 KB of LDS, the opt-in path
    ("dec3-9001", "dec:3", None, 9001, False, 1, True),
    ("noise40", "noise:40", None, 4000, False, 1, True),
    ("at20", "at:20", None, 4000, False, 1, True),
    ("noise40-eot3", "noise:40", None, 4000, False, 3, True),
    ("chain", "ms:7,qt:512,ds:2,noise:40", None, 4000, False, 1, False),
    ("chain-eot2-9001", "ms:7,qt:512,ds:2,noise:40", None, 9001, False, 2, False),
    ("ulaw-9001", None, "ulaw", 9001, False, 1, True),
    ("alaw", None, "alaw", 4000, False, 1, True),
    ("adpcm", None, "adpcm", 4000, False, 1, True),
    ("chain+codec", "ms:7,qt:512", "ulaw", 4000, False, 1, False),
    ("full-fir5-gain2", FIR5_GAIN2, None, 4000, True, 1, False),
    ("full-qt64-noise", "qt:64,noise:400", None, 4000, True, 1, True),
    ("empty-eot2", None, None, 4000, False, 2, True),
]


# ------------------------------------------------------------------------------------- 1. the hook, stage by stage
@pytest.mark.parametrize("name,spec,codec,n,full,r,exact", HOOK_CASES, ids=[c[0] for c in HOOK_CASES])
def test_defence_vjp_hook_against_the_restatement(eng, name, spec, codec, n, full, r, exact):
    wav = _full_range(n) if full else quantize(R.test_audio(n))
    chain = _chain(spec)
    cot = np.random.default_rng(n + len(name)).normal(size=(r, n))
    it = 5 if r > 1 else 0
    try:
        eng.set_input_transform(spec)
        eng.set_codec(codec)
        eng.set_eot(r)
        dwav, out = eng.debug_defence_vjp(wav, cot, SEED, STREAM, it)
        route = eng.debug_wb_route()
        worst, saturated = 0.0, 0
        for j in range(r):
            want, ref_out = B.defence_vjp(wav, chain, codec, _normals(eng, chain, n, it, j), cot[j])
            assert np.array_equal(out[j], ref_out), "replica %d: the transformed row is not the twins'" % j
            saturated += int(((ref_out == 32767) | (ref_out == -32768)).sum())
            assert np.isfinite(dwav[j]).all()
            if exact:
                assert np.array_equal(dwav[j], want)
            else:
                worst = max(worst, rel_l2(dwav[j], want))
    finally:
        _clear(eng)
    print("defence vjp %s N=%d r=%d: relative L2 error %.3g (samples at a rail: %d)" % (name, n, r, worst, saturated))
    assert route == dict(ctl=0, ctl_rep=0, backward=0, chain_t=r)
    if full:
        assert saturated > 0        # the saturation rule was exercised
    if r > 1 and chain:
        assert not np.array_equal(out[0], out[1])
    assert worst < BAR_VJP


# ------------------------------------------------------------------------------------- 2. the full gradient
BRANCHES = [("osi_targeted", "OSI", "targeted", dict(target=1, threshold=-10.0)),
            ("csi_untargeted", "CSI", "untargeted", dict(true=0))]
GRAD_CASES = [("ms7-qt512", "ms:7,qt:512", None, 1, 0), ("ds2", "ds:2", None, 1, 0), ("ulaw", None, "ulaw", 1, 0),
              ("adpcm", None, "adpcm", 1, 0), ("noise40-r1-it0", "noise:40", None, 1, 0), ("noise40-r1-it5", "noise:40", None, 1, 5),
              ("noise40-r2-it0", "noise:40", None, 2, 0), ("noise40-r3-it0", "noise:40", None, 3, 0), ("noise40-r3-it5", "noise:40", None, 3, 5)]


def _p(task, attack, kw, **more):
    return nes_params(task, attack, samples_per_draw=0, seed=SEED, stream=STREAM, **dict(kw, **more))


def _ref_grad(e, models, task, attack, kw, audio, chain, codec, r, it):
    zk = {} if task != "CSI" else dict(z_mean=Z_MEAN[:models[0].shape[0]], z_std=Z_STD[:models[0].shape[0]])
    nz = [_normals(e, chain, audio.size, it, j) for j in range(r)]
    return B.loss_and_grad(e.cfg, models, task, attack, audio, chain, codec, nz, **dict(kw, **zk))


@pytest.mark.parametrize("name,spec,codec,r,it", GRAD_CASES, ids=[c[0] for c in GRAD_CASES])
@pytest.mark.parametrize("bname,task,attack,kw", BRANCHES, ids=[b[0] for b in BRANCHES])
def test_get_grad_wb_through_the_defences(eng, small_system, bname, task, attack, kw, name, spec, codec, r, it):
    audio = R.test_audio(4000)
    models = _load(eng, small_system, task)
    chain = _chain(spec)
    try:
        eng.set_input_transform(spec)
        eng.set_codec(codec)
        eng.set_eot(r)
        eng.set_wb_bpda(True)
        grad, al, sc = eng.get_grad_wb_iter(_p(task, attack, kw), audio, it)
        route = eng.debug_wb_route()
        ref = _ref_grad(eng, models, task, attack, kw, audio, chain, codec, r, it)
    finally:
        _clear(eng)
    err = rel_l2(grad, ref.grad)
    print("%s %s: loss %.9g (restatement %.9g; per replica %s), min |c0 - thr| %.3g, relative L2 error %.3g"
          % (bname, name, al, ref.loss, ref.losses, ref.margin, err))
    assert route == dict(ctl=1 if r == 1 else 0, ctl_rep=r if r > 1 else 0, backward=r, chain_t=r if (chain or r > 1) else 0)
    assert ref.margin > 1e-3
    assert abs(al - ref.loss) < 1e-3 and np.abs(sc - ref.scores).max() < 1e-3
    assert np.isfinite(grad).all()
    assert err < BAR_GRAD


def test_the_draws_differ_between_epochs(eng, small_system):
    audio = R.test_audio(4000)
    _load(eng, small_system, "OSI")
    p = _p("OSI", "targeted", dict(target=1, threshold=-10.0))
    try:
        eng.set_input_transform("noise:40")
        eng.set_eot(3)
        eng.set_wb_bpda(True)
        g0, al0, _ = eng.get_grad_wb(p, audio)
        g0b, al0b, _ = eng.get_grad_wb_iter(p, audio, 0)
        g5, al5, _ = eng.get_grad_wb_iter(p, audio, 5)
    finally:
        _clear(eng)
    assert np.array_equal(g0, g0b) and al0 == al0b                    # fb_get_grad_wb is iter = 0
    assert al0 != al5 and not np.array_equal(g0, g5)


# ------------------------------------------------------------------------------------- 3. forward parity
PARITY = [("chain", "ms:7,qt:512", None, 1), ("codec", None, "ulaw", 1), ("chain+codec", "ds:2", "adpcm", 1), ("eot3-noise", "noise:40", None, 3)]


@pytest.mark.parametrize("name,spec,codec,r", PARITY, ids=[c[0] for c in PARITY])
def test_the_forward_is_get_grads(eng, small_system, name, spec, codec, r):
    audio = R.test_audio(4000)
    _load(eng, small_system, "OSI")
    p = _p("OSI", "targeted", dict(target=1, threshold=-10.0))
    try:
        eng.set_input_transform(spec)
        eng.set_codec(codec)
        eng.set_eot(r)
        eng.set_wb_bpda(True)
        for it in (0, 5):
            _g, al, sc = eng.get_grad_wb_iter(p, audio, it)
            _fl, _gg, al0, sc0 = eng.get_grad(p, audio, it=it, want_grad=False)
            assert al == al0 and np.array_equal(sc, sc0), (name, it)
    finally:
        _clear(eng)


# ------------------------------------------------------------------------------------- 4. determinism
@pytest.mark.parametrize("spec,codec,r", [("noise:40", None, 3), ("ms:7,ds:2", "ulaw", 1)], ids=["eot3", "chain+codec"])
def test_two_fresh_engines_give_equal_bits(small_system, spec, codec, r):
    audio = R.test_audio(4000)
    p = _p("OSI", "targeted", dict(target=1, threshold=-10.0))
    got = []
    for _ in range(2):
        e = Engine(0)
        try:
            _load(e, small_system, "OSI")
            e.set_input_transform(spec)
            e.set_codec(codec)
            e.set_eot(r)
            e.set_wb_bpda(True)
            got.append(e.get_grad_wb_iter(p, audio, 2))
        finally:
            e.close()
    a, b = got
    assert np.array_equal(a[0].view(np.uint64), b[0].view(np.uint64)) and a[1] == b[1] and np.array_equal(a[2], b[2])


# ------------------------------------------------------------------------------------- 5. nothing changes when nothing is set
def test_the_switch_alone_changes_nothing(eng, small_system):
    audio = R.test_audio(4000)
    _load(eng, small_system, "OSI")
    p = nes_params("OSI", "targeted", target=1, threshold=0.0, max_iter=4)
    off = eng.get_grad_wb(p, audio)
    off_route, off_nes = eng.debug_wb_route(), eng.debug_nes_route()
    off_attack = eng.attack_wb(p, audio)
    off_attack_route = eng.debug_wb_route()
    try:
        eng.set_wb_bpda(True)
        on = eng.get_grad_wb(p, audio)
        on_route, on_nes = eng.debug_wb_route(), eng.debug_nes_route()
        on_attack = eng.attack_wb(p, audio)
        on_attack_route = eng.debug_wb_route()
    finally:
        _clear(eng)
    assert np.array_equal(off[0].view(np.uint64), on[0].view(np.uint64)) and off[1] == on[1] and np.array_equal(off[2], on[2])
    assert off_route == on_route == dict(ctl=1, ctl_rep=0, backward=1, chain_t=0) and off_nes == on_nes
    assert off_attack_route == on_attack_route and off_attack_route["chain_t"] == 0
    for x, y in zip(off_attack, on_attack):
        assert np.array_equal(x, y)


def test_the_switch_takes_0_or_1(eng):
    with pytest.raises(N.NativeError) as ex:
        N.check(eng._L.fb_set_wb_bpda(eng._h, 2))
    assert ex.value.code == N.FB_E_ARG


WB_P = nes_params("OSI", "targeted", target=1, threshold=0.0, max_iter=3)
OFF_CASES = {
    "eot": (lambda e: e.set_eot(2), "fb_set_eot"),
    "input_transform": (lambda e: e.set_input_transform("qt:64"), "input-transform"),
    "codec": (lambda e: e.set_codec("ulaw"), "codec"),
}


def _refused(e, audio, p=WB_P):
    for call in (lambda: e.get_grad_wb(p, audio), lambda: e.get_grad_wb_iter(p, audio, 1), lambda: e.attack_wb(p, audio)):
        with pytest.raises(N.NativeError) as ex:
            call()
        assert ex.value.code == N.FB_E_STATE, str(ex.value)
    return str(ex.value)


@pytest.mark.parametrize("case", sorted(OFF_CASES))
def test_switch_off_refuses_as_before(eng, small_system, case):
    on, word = OFF_CASES[case]
    _load(eng, small_system, "OSI")
    on(eng)
    try:
        assert word in _refused(eng, R.test_audio(4000))
    finally:
        _clear(eng)


# ------------------------------------------------------------------------------------- 6. a whole attack is its replay
def replay(e, p, audio):
    """FakeBob.attack (FAKEBOB.py:157-220) on the host in numpy float64, the gradient from fb_get_grad_wb_iter at every
    iterate with the loop index as the epoch of the draws"""
    audio = np.asarray(audio, np.float64)
    adver, grad_m, lr, ls, rows = audio.copy(), np.zeros_like(audio), p.max_lr, [], []
    lower, upper = np.clip(audio - p.epsilon, -1.0, 1.0), np.clip(audio + p.epsilon, -1.0, 1.0)
    last = p.max_iter - 1
    for it in range(p.max_iter):
        g, al, sc = e.get_grad_wb_iter(p, adver, it)
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
    return quantize(adver), (1 if last < p.max_iter - 1 else -1), adver, np.array(rows)


@pytest.mark.parametrize("batch", ["1", "4"])
def test_a_whole_attack_is_its_replay(eng, small_system, monkeypatch, batch):
    _load(eng, small_system, "OSI")
    audio = R.test_audio(4000)
    # (adver_thresh keeps the mean loss above zero: the unshifted one crosses it at the third iteration)
    p = nes_params("OSI", "targeted", target=1, threshold=0.0, adver_thresh=50.0, max_iter=4, plateau_length=2, seed=SEED, stream=STREAM)
    monkeypatch.setenv("FB_ATTACK_BATCH", batch)
    try:
        eng.set_input_transform("noise:40")
        eng.set_eot(2)
        eng.set_wb_bpda(True)
        adv, flag, adv_f, trace = eng.attack_wb(p, audio)
        route = eng.debug_wb_route()
        r_adv, r_flag, r_adv_f, r_trace = replay(eng, p, audio)
    finally:
        _clear(eng)
    print("batch %s: %d rows, flag %d, loss %s, lr %s" % (batch, trace.shape[0], flag, trace[:, 1], trace[:, 2]))
    assert route == dict(ctl=0, ctl_rep=8, backward=8, chain_t=8)
    assert trace.shape == r_trace.shape == (4, 6) and np.array_equal(trace.view(np.uint64), r_trace.view(np.uint64))
    assert flag == r_flag and np.array_equal(adv_f.view(np.uint64), r_adv_f.view(np.uint64)) and np.array_equal(adv, r_adv)
    assert len(set(trace[:, 1])) == 4


# ------------------------------------------------------------------------------------- 7. still refused with the switch on
ON_CASES = {
    "companions": (lambda e: e.set_companions([R.test_audio(4000)]), lambda e: e.set_companions(None), "companions"),
    "feature_compression": (lambda e: e.set_feature_compression(0.5, 2), lambda e: e.set_feature_compression(None), "feature compression"),
    "dither": (lambda e: e.set_frontend(dither=1.0), lambda e: e.set_frontend(dither=0.0), "dither"),
    # the channel's transpose is not in this version
    "air_channel": (lambda e: e.set_air_channel("t60:100-200,drr:6,taps:256,delay:8"), lambda e: e.set_air_channel(None), "air channel"),
}
NES_P = nes_params("OSI", "targeted", target=1, threshold=0.0, max_iter=3, samples_per_draw=6, seed=9)


@pytest.fixture(scope="module")
def nes_baseline(small_system):
    e = Engine(0)
    try:
        _load(e, small_system, "OSI")
        return e.attack(NES_P, R.test_audio(4000))
    finally:
        e.close()


def _same_attack(e, nes_baseline):
    for a, b in zip(e.attack(NES_P, R.test_audio(4000)), nes_baseline):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("case", sorted(ON_CASES))
def test_still_refused_with_the_switch_on(eng, small_system, nes_baseline, case):
    on, off, word = ON_CASES[case]
    _load(eng, small_system, "OSI")
    eng.set_wb_bpda(True)
    on(eng)
    try:
        assert word in _refused(eng, R.test_audio(4000))
    finally:
        off(eng)
        _clear(eng)
    _same_attack(eng, nes_baseline)


def test_an_ivector_system_is_still_refused(eng, small_system, nes_baseline):
    from fakebob_amd.models import synthetic_ivector_system
    sy = synthetic_ivector_system(C=64, D=72, R=32, L=16, n_speakers=2, seed=4)
    eng.load_ivector(sy, "OSI")
    eng.set_wb_bpda(True)
    try:
        assert "i-vector" in _refused(eng, R.test_audio(4000))
    finally:
        _clear(eng)
    _load(eng, small_system, "OSI")
    _same_attack(eng, nes_baseline)


# ------------------------------------------------------------------------------------- 8. it does what it is for
def test_bpda_beats_the_transferred_attack(eng, small_system):
    """30 PGD iterations against qt:512,ms:7: once through the defence (BPDA), once on the undefended gradient with the result
    then scored through the defended victim.  Both runs are deterministic; the two losses are in DESIGN.md section 6."""
    _load(eng, small_system, "SV")
    audio = R.test_audio(4000)
    p = nes_params("SV", "untargeted", threshold=1e3, max_iter=30, seed=SEED, stream=STREAM)       # (never stops early)
    score = nes_params("SV", "untargeted", threshold=1e3, samples_per_draw=0, seed=SEED, stream=STREAM)
    spec = "qt:512,ms:7"
    try:
        _adv, _flag, transfer_f, _trace = eng.attack_wb(p, audio)
        eng.set_input_transform(spec)
        clean = eng.get_grad(score, audio, want_grad=False)[2]
        transfer = eng.get_grad(score, transfer_f, want_grad=False)[2]
        eng.set_wb_bpda(True)
        _adv, _flag, bpda_f, _trace = eng.attack_wb(p, audio)
        bpda = eng.get_grad(score, bpda_f, want_grad=False)[2]
    finally:
        _clear(eng)
    print("defended adver_loss: clean %.9g, after the transferred attack %.9g, after the BPDA attack %.9g" % (clean, transfer, bpda))
    assert bpda < transfer


# ------------------------------------------------------------------------------------- 9. AdaptivePGD and the driver
def test_adaptive_pgd_returns_fakebobs_pair_and_checkpoint(small_system, tmp_path):
    from fakebob_amd.pgd import AdaptivePGD
    from fakebob_amd.systems import gmm_SV
    ubm, spk = small_system
    model = gmm_SV(str(tmp_path / "sv"), ["spk0", "utt0", spk[0], 0.0, 1.0], ubm, pre_model_dir=str(tmp_path), threshold=0.0,
                   input_transform="ms:7,noise:40")
    audio = R.test_audio(4000)
    pgd = AdaptivePGD("SV", "targeted", model, bpda=True, eot_size=2, max_iter=5, seed=11, verbose=False)
    assert model.engine.eot == 2 and model.engine.wb_bpda
    cp = str(tmp_path / "pgd.cp")
    adv, flag = pgd.attack(audio, cp, threshold=1e3)
    assert adv.dtype == np.int16 and adv.shape == (4000, 1) and flag == -1
    with open(cp, "rb") as r:
        rows = pickle.load(r)
    assert len(rows) == 5
    for row in rows:
        assert len(row) == 4 and row[1].shape == (1,) and np.ndim(row[2]) == 0 and isinstance(row[3], float)
    g, al, sc = pgd.get_grad(audio)
    assert g.shape == (4000, 1) and al.shape == (1,) and np.ndim(sc) == 0 and np.isfinite(g).all()
    adv2, flag2, _f, trace2 = model.engine.attack_wb(pgd._params(), audio)      # the same trajectory as the engine's own call
    assert np.array_equal(adv2, adv[:, 0]) and flag2 == flag and trace2.shape[0] == 5
    assert model.engine.debug_wb_route() == dict(ctl=0, ctl_rep=10, backward=10, chain_t=10)


def test_attack_main_pgd_bpda_on_the_synthetic_site(tmp_path, capsys):
    from fakebob_amd import attack_main as AM
    from fakebob_amd.systems import gmm_OSI
    from tests.test_gpu_driver import _site
    ids, _ubm, _spk = _site(tmp_path)
    ml = AM.load_spk_models(str(tmp_path / "model"), ids, "gmm")
    probe = gmm_OSI(str(tmp_path / "probe"), ml, str(tmp_path / "pre-models" / "final.dubm"), pre_model_dir=str(tmp_path / "pre-models"),
                    threshold=0.0, input_transform="ms:7")
    voices = AM.collect_voices(str(tmp_path / "data" / "illegal-set"))
    thr = float(probe.score([v[2] for v in voices]).max()) + 0.002
    site = ["--model_dir", str(tmp_path / "model"), "--pre_model_dir", str(tmp_path / "pre-models"), "--test_dir",
            str(tmp_path / "data" / "test-set"), "--illegal_dir", str(tmp_path / "data" / "illegal-set"), "--out_dir", str(tmp_path / "out")]
    argv = ["-spk_id"] + ids + ["-archi", "gmm", "-task", "OSI", "-type", "targeted", "-thresh", str(thr), "-max_iter", "4", "--attack",
                                "pgd", "--bpda", "--input-transform", "ms:7", "--eot-size", "2", "--streams", "1", "--seed", "7"] + site
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
            assert 1 <= len(rows) <= 4 and len(rows[0]) == 4
            n += 1
    assert n == 12
    for extra in (["--companions", "1"], ["--feco", "0.5"], ["--air-channel", "t60:200-600"], ["--dither", "1.0"], ["-archi", "iv"]):
        with pytest.raises(SystemExit):
            AM.main(argv + extra)
    with pytest.raises(SystemExit):
        AM.main([a for a in argv if a != "--bpda"])          # the undefended driver's refusals stand without the flag
    capsys.readouterr()
