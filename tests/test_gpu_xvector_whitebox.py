"""White-box gradients through the x-vector (TDNN) victim (fb_set_wb_xvector; the x-vector part of the "white-box gradients"
contract of include/fakebob_hip.h) against the PyTorch restatement tests/xvector_vjp_ref.py, which
tests/test_xvector_vjp_host.py ties to tests/xvector_ref.py and to a finite difference.

Accuracy: err = the relative L2 error against the float64 restatement, per utterance, for the device (err_dev) and for the
float32 restatement (err_32: feature rows rounded to float32, frame layers in float32 -- what a float32 implementation of the same
function gives); err_dev <= 4 * err_32, the factor tests/test_gpu_xvector.py grants another summation order at equal precision.
Both restatements are given the DEVICE's ReLU decisions (debug_xv_masks), and both figures are printed.

Conditions of the fixture, not tolerances: the device's masks equal the float64 restatement's own on every unit with
|z| >= 1e-4 max |z| of its layer, at most 0.2 % of a case's units lie below that margin, no pooled variance lies in
(1e-12, 1e-8), and -- for whole gradients -- the VAD margin is >= 1e-3 as the GMM tests assert.
tests/test_xvector_vjp_host.py shows that the restatement alone meets them for these shapes, lengths and seeds.

Whole gradients: the front end's forward is float32 on the device and float64 in the restatement, so the feature rows the TDNN is
evaluated at differ by the front end's own error.  The bar holds all the same (worst ratio measured: 1.57); it is applied a second
time with both restatements handed the device's own feature rows (debug_feats), their values straight-through, which takes the
front end's forward out of the comparison (worst ratio 1.32).  Both pairs of figures are printed."""
import functools
import pickle

import numpy as np
import pytest
import torch

from fakebob_amd import _native as N
from fakebob_amd import companions as CP
from fakebob_amd import input_transform as IT
from fakebob_amd.cw2 import CW2
from fakebob_amd.engine import Engine, nes_params
from fakebob_amd.models import stack_models, synthetic_audio, synthetic_gmm_system, synthetic_ivector_system
from fakebob_amd.pgd import XvectorPGD
from fakebob_amd.psy import Imperceptible
from tests import bpda_ref as B
from tests import xvector_vjp_ref as V
from tests.test_gpu_whitebox import quantize, rel_l2
from tests.test_gpu_xvector import LENGTHS, SHAPES, _agrees, _ranged, _rows, _sv_setting, _system

pytestmark = pytest.mark.gpu
FACTOR = 4.0
EDGE, NEAR_SHARE, VAD_MARGIN = 1e-4, 0.002, 1e-3
SEED, STREAM = 77, 3


@pytest.fixture(scope="module")
def eng():
    """delta_order = 0 (D = 24): the hook's shapes"""
    e = Engine(0)
    e.set_frontend(delta_order=0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def eng72():
    """the default front end (D = 72): whole gradients"""
    e = Engine(0)
    yield e
    e.close()


def _ebar(sy, n, seed=17):
    rng = np.random.default_rng(seed)
    return [rng.normal(size=sy.R) for _ in range(n)]


def _split(a, lengths):
    off = np.concatenate([[0], np.cumsum(lengths)])
    return [a[off[b]:off[b + 1]] for b in range(len(lengths))]


def _conditions(what, zs, masks, var):
    flips, near, near_floor = V.mask_conditions(zs, masks, var, EDGE)
    assert flips == 0, "%s: %d mask decisions differ away from the edge" % (what, flips)
    assert near_floor == 0, "%s: %d pooled variances near the floor" % (what, near_floor)
    return near


# ------------------------------------------------------------------------------------- 1, 2. the hook against autograd
def _check_hook(eng, name, sy):
    mats = _rows(sy.D)
    ebar = _ebar(sy, len(mats))
    eng.load_xvector(sy, "OSI")
    nl = len(sy.layers)
    dev = {s: eng.debug_xv_backward(mats, ebar, s) for s in range(nl + 1, -1, -1)}     # (stage 0 last: every launch)
    masks = [_split(eng.debug_xv_masks(l), LENGTHS) for l in range(nl)]
    assert eng.debug_wb_xv_route() == dict(backend_t=0, segment_t=1, pool_t=1, act_t=nl, affine_t=nl, unsplice=nl)
    worst, near, units, floored = 0.0, 0, 0, 0
    for b, x in enumerate(mats):
        mb = [masks[l][b] for l in range(nl)]
        r64 = V.feat_grad(sy, x, ebar[b], torch.float64, mb)
        r32 = V.feat_grad(sy, x, ebar[b], torch.float32, mb)
        near += _conditions("%s utterance %d" % (name, b), r64.zs, mb, r64.var) * sum(z.size for z in r64.zs)
        units += sum(z.size for z in r64.zs)
        floored += int(np.sum(r64.var <= 1e-10))
        for s in range(nl + 2):
            got = np.asarray(dev[s][b], np.float64)
            want, f32 = r64.grads[s], r32.grads[s]
            assert got.shape == want.shape and np.all(np.isfinite(got))
            if not want.any():      # (a one-row utterance whose statistics pass nothing further is exactly zero)
                assert not got.any() and not f32.any()
                continue
            err_dev, err_32 = rel_l2(got, want), rel_l2(f32, want)
            if s > nl:              # the statistics' cotangent is float64 on both sides: the bar is float64's own
                assert err_dev <= 1e-13, (name, b, s, err_dev)
                continue
            print("%s utterance %d (%d rows) stage %d: err_dev %.3g err_32 %.3g ratio %.2f" % (name, b, x.shape[0], s, err_dev, err_32, err_dev / err_32))
            assert err_32 > 0.0
            assert err_dev <= FACTOR * err_32, (name, b, s, err_dev, err_32)
            worst = max(worst, err_dev / err_32)
    print("%s: worst err_dev / err_32 %.2f; %.4f %% of units near an edge; %d floored channels" % (name, worst, 100.0 * near / units, floored))
    assert near <= NEAR_SHARE * units
    if nl > 1:
        assert floored > sy.P
    return worst


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_backward_hook_against_autograd(eng, name):
    _check_hook(eng, name, _system(eng.feat_dim, **SHAPES[name]))


def test_backward_hook_with_cotangents_outside_f16s_range(eng):
    sy = _ranged(_system(eng.feat_dim))
    r = V.feat_grad(sy, _rows(sy.D)[2], _ebar(sy, 3)[2])
    big = max(np.abs(g).max() for g in r.grads[1:-1])
    small = min(np.abs(g).max() for g in r.grads[1:-1])
    assert small < 2.0 ** -14, (big, small)      # below f16's normal range: the case is what it says
    _check_hook(eng, "ranged", sy)


# ------------------------------------------------------------------------------------- 3. bit identity
@pytest.mark.parametrize("name", ["stock", "partial-tiles"])
def test_a_run_repeats_and_a_cotangent_does_not_depend_on_its_batch(eng, name):
    sy = _system(eng.feat_dim, **SHAPES[name])
    eng.load_xvector(sy, "OSI")
    mats = _rows(sy.D)
    ebar = _ebar(sy, len(mats))
    nl = len(sy.layers)
    full = eng.debug_xv_backward(mats, ebar, 0)
    for s in (0, 1, nl, nl + 1):
        a, b = eng.debug_xv_backward(mats, ebar, s), eng.debug_xv_backward(mats, ebar, s)
        assert all(np.array_equal(np.asarray(u).view(np.uint8), np.asarray(v).view(np.uint8)) for u, v in zip(a, b)), s
    other = _rows(sy.D, [5, 40, 129, 7], seed=9)
    oe = _ebar(sy, 4, seed=5)
    for i, m in enumerate(mats):
        alone = eng.debug_xv_backward([m], [ebar[i]], 0)[0]
        first = eng.debug_xv_backward([m] + other, [ebar[i]] + oe, 0)[0]
        last = eng.debug_xv_backward(other + [m], oe + [ebar[i]], 0)[-1]
        between = eng.debug_xv_backward(other[:2] + [m] + other[2:], oe[:2] + [ebar[i]] + oe[2:], 0)[2]
        for what, got in (("alone", alone), ("first", first), ("last", last), ("between", between)):
            assert np.array_equal(got.view(np.uint64), full[i].view(np.uint64)), (name, i, m.shape[0], what)
    assert len({full[i].tobytes() for i in range(len(mats))}) == len(mats)


# ------------------------------------------------------------------------------------- 4. the whole gradient
BRANCHES = {"osi_targeted": ("OSI", "targeted", dict(target=1, threshold=-10.0)),
            "osi_untargeted": ("OSI", "untargeted", dict(threshold=-10.0)),
            "csi_targeted": ("CSI", "targeted", dict(target=2)),
            "sv": ("SV", "targeted", dict(threshold=-10.0))}


@functools.lru_cache(maxsize=None)
def _sys72(name, n_speakers):
    return _system(72, n_speakers=n_speakers, **SHAPES[name])


def _device_masks(e, sy, lengths):
    return [_split(e.debug_xv_masks(l), lengths) for l in range(len(sy.layers))]


def _grad_errors(e, sy, task, at, kw, wav, masks, grad, al, what):
    """-> (err_dev, err_32, err_dev_f, err_32_f): against the restatement on its own feature rows, and with both restatements
    handed the device's feature rows; the fixture's conditions asserted on the way"""
    audio = wav.astype(np.float64) / 32768.0
    r64 = V.loss_and_grad_xv(e.cfg, sy, task, at, audio, masks=masks, **kw)
    assert r64.margin >= VAD_MARGIN, (what, r64.margin)
    assert r64.tv == masks[0].shape[0], (what, r64.tv, masks[0].shape)
    near = _conditions(what, r64.zs, masks, r64.var)
    assert near <= NEAR_SHARE
    assert abs(al - r64.loss) <= 1e-3 * max(1.0, abs(r64.loss)), (what, al, r64.loss)
    r32 = V.loss_and_grad_xv(e.cfg, sy, task, at, audio, masks=masks, frame_dtype=torch.float32, **kw)
    feats = e.debug_feats(wav)[0]
    f64 = V.loss_and_grad_xv(e.cfg, sy, task, at, audio, masks=masks, feats=feats, **kw)
    f32 = V.loss_and_grad_xv(e.cfg, sy, task, at, audio, masks=masks, feats=feats, frame_dtype=torch.float32, **kw)
    return rel_l2(grad, r64.grad), rel_l2(r32.grad, r64.grad), rel_l2(grad, f64.grad), rel_l2(f32.grad, f64.grad), r64


GRAD_CASES = [(name, n, br) for name in ("stock", "partial-tiles") for n in (2000, 4000, 20000) for br in sorted(BRANCHES)]


@pytest.mark.parametrize("name,n,branch", GRAD_CASES, ids=["%s-%d-%s" % c for c in GRAD_CASES])
def test_get_grad_wb_against_the_restatement(eng72, name, n, branch):
    task, at, kw = BRANCHES[branch]
    sy = _sys72(name, 1 if task == "SV" else 3)
    e = eng72
    e.load_xvector(sy, task)
    audio = synthetic_audio(0, n)
    p = nes_params(task, at, samples_per_draw=0, **kw)
    e.set_wb_xvector(True)
    try:
        grad, al, sc = e.get_grad_wb(p, audio)
        tv = e.debug_xv_masks(0).shape[0]
        masks = [m[0] for m in _device_masks(e, sy, [tv])]
        route, xroute = e.debug_wb_route(), e.debug_wb_xv_route()
        _fl, _g, al0, sc0 = e.get_grad(p, audio, want_grad=False)
        again, _al, _sc = e.get_grad_wb(p, audio)
    finally:
        e.set_wb_xvector(False)
    assert al == al0 and np.array_equal(sc, sc0)                  # the same scoring call, bit for bit
    assert np.array_equal(grad.view(np.uint64), again.view(np.uint64))
    nl = len(sy.layers)
    assert xroute == dict(backend_t=1, segment_t=1, pool_t=1, act_t=nl, affine_t=nl, unsplice=nl)
    assert route == dict(ctl=0, ctl_rep=0, backward=1, chain_t=0)
    if n == 20000:
        assert tv < e._num_frames(n)                              # the VAD compaction ran
    wav = quantize(audio)
    err_dev, err_32, err_dev_f, err_32_f, r64 = _grad_errors(e, sy, task, at, kw, wav, masks, grad, al, "%s N=%d %s" % (name, n, branch))
    print("%s N=%d %s (%d voiced rows): err_dev %.3g err_32 %.3g ratio %.2f; at the device's feature rows: err_dev %.3g err_32 %.3g ratio %.2f"
          % (name, n, branch, tv, err_dev, err_32, err_dev / err_32, err_dev_f, err_32_f, err_dev_f / err_32_f))
    assert err_32 > 0.0 and err_32_f > 0.0
    assert err_dev <= FACTOR * err_32, (err_dev, err_32)
    assert err_dev_f <= FACTOR * err_32_f, (err_dev_f, err_32_f)


# ------------------------------------------------------------------------------------- 5. BPDA and EOT
def _chain(spec):
    return [tuple(s) for s in IT.parse(spec)]


def _clear(e):
    e.set_input_transform(None)
    e.set_codec(None)
    e.set_eot(1)
    e.set_wb_bpda(False)
    e.set_wb_xvector(False)


def test_get_grad_wb_through_a_chain_and_eot_behind_a_deterministic_chain(eng72):
    e = eng72
    task, at, kw = BRANCHES["osi_targeted"]
    sy = _sys72("stock", 3)
    e.load_xvector(sy, task)
    audio = synthetic_audio(0, 4000)
    spec = "qt:512,ms:7"
    chain = _chain(spec)
    p = nes_params(task, at, samples_per_draw=0, seed=SEED, stream=STREAM, **kw)
    try:
        e.set_input_transform(spec)
        e.set_wb_bpda(True)
        e.set_wb_xvector(True)
        grad, al, sc = e.get_grad_wb(p, audio)
        tv = e.debug_xv_masks(0).shape[0]
        masks = [m[0] for m in _device_masks(e, sy, [tv])]
        route = e.debug_wb_route()
        _fl, _g, al0, sc0 = e.get_grad(p, audio, want_grad=False)
        e.set_eot(4)
        grad4, al4, sc4 = e.get_grad_wb(p, audio)
        route4, xroute4 = e.debug_wb_route(), e.debug_wb_xv_route()
    finally:
        _clear(e)
    assert al == al0 and np.array_equal(sc, sc0)
    assert route == dict(ctl=0, ctl_rep=0, backward=1, chain_t=1)
    wav = quantize(audio)
    _d, out = B.defence_vjp(wav, chain, None, None, np.zeros(wav.size))
    a_out = out.astype(np.float64) / 32768.0

    def through(r):
        return B.defence_vjp(wav, chain, None, None, r.grad / 32768.0)[0] * 32768.0
    r64 = V.loss_and_grad_xv(e.cfg, sy, task, at, a_out, masks=masks, **kw)
    assert r64.margin >= VAD_MARGIN and r64.tv == tv
    assert _conditions("chain", r64.zs, masks, r64.var) <= NEAR_SHARE
    feats = e.debug_feats(out)[0]
    f64 = V.loss_and_grad_xv(e.cfg, sy, task, at, a_out, masks=masks, feats=feats, **kw)
    f32 = V.loss_and_grad_xv(e.cfg, sy, task, at, a_out, masks=masks, feats=feats, frame_dtype=torch.float32, **kw)
    r32 = V.loss_and_grad_xv(e.cfg, sy, task, at, a_out, masks=masks, frame_dtype=torch.float32, **kw)
    err_dev, err_32 = rel_l2(grad, through(r64)), rel_l2(through(r32), through(r64))
    err_dev_f, err_32_f = rel_l2(grad, through(f64)), rel_l2(through(f32), through(f64))
    print("through qt:512,ms:7: loss %.9g (restatement %.9g); err_dev %.3g err_32 %.3g ratio %.2f; at the device's feature rows: "
          "err_dev %.3g err_32 %.3g ratio %.2f" % (al, r64.loss, err_dev, err_32, err_dev / err_32, err_dev_f, err_32_f, err_dev_f / err_32_f))
    assert abs(al - r64.loss) < 1e-3
    assert err_32 > 0.0 and err_dev <= FACTOR * err_32
    assert err_32_f > 0.0 and err_dev_f <= FACTOR * err_32_f
    # four replicas of a deterministic chain are four times the same row: weights 1 / 4, exact powers of two
    nl = len(sy.layers)
    assert route4 == dict(ctl=0, ctl_rep=4, backward=4, chain_t=4)
    assert xroute4 == dict(backend_t=4, segment_t=1, pool_t=1, act_t=nl, affine_t=nl, unsplice=nl)
    same = np.array_equal(grad4.view(np.uint64), grad.view(np.uint64))
    print("eot = 4 behind the deterministic chain: bit-identical to eot = 1: %s (relative difference %.3g)" % (same, rel_l2(grad4, grad)))
    assert rel_l2(grad4, grad) <= 1e-12
    assert abs(al4 - al) <= 1e-12 * abs(al) and np.allclose(sc4, sc, rtol=1e-12, atol=0)


def test_eot_gradient_is_the_mean_over_the_replicas_own_draws(eng72):
    e = eng72
    task, at, kw = BRANCHES["osi_targeted"]
    sy = _sys72("stock", 3)
    e.load_xvector(sy, task)
    n, it = 4000, 5
    audio = synthetic_audio(0, n)
    spec = "noise:8"
    chain = _chain(spec)
    p = nes_params(task, at, samples_per_draw=0, seed=SEED, stream=STREAM, **kw)
    nl = len(sy.layers)
    try:
        e.set_input_transform(spec)
        e.set_eot(2)
        e.set_wb_bpda(True)
        e.set_wb_xvector(True)
        grad, al, sc = e.get_grad_wb_iter(p, audio, it)
        raw_masks = [e.debug_xv_masks(l) for l in range(nl)]
        route, xroute = e.debug_wb_route(), e.debug_wb_xv_route()
        normals = [{s: e.debug_tf_noise(SEED, STREAM, it, 0, j, s, 0, n) for s, st in enumerate(chain) if st[0] == B.NOISE} for j in range(2)]
    finally:
        _clear(e)
    assert route == dict(ctl=0, ctl_rep=2, backward=2, chain_t=2)
    assert xroute == dict(backend_t=2, segment_t=1, pool_t=1, act_t=nl, affine_t=nl, unsplice=nl)
    wav = quantize(audio)
    outs = [B.defence_vjp(wav, chain, None, normals[j], np.zeros(n))[1] for j in range(2)]
    assert not np.array_equal(outs[0], outs[1])
    feats = [e.debug_feats(o)[0] for o in outs]
    tvs = [f.shape[0] for f in feats]
    assert sum(tvs) == raw_masks[0].shape[0]
    masks = [_split(m, tvs) for m in raw_masks]
    want, losses = {}, []
    for j in range(2):
        mj = [m[j] for m in masks]
        a_out = outs[j].astype(np.float64) / 32768.0
        for key, ft, dt in (("r64", None, torch.float64), ("r32", None, torch.float32), ("f64", feats[j], torch.float64), ("f32", feats[j], torch.float32)):
            r = V.loss_and_grad_xv(e.cfg, sy, task, at, a_out, masks=mj, feats=ft, frame_dtype=dt, **kw)
            if key == "r64":
                assert r.margin >= VAD_MARGIN and r.tv == tvs[j]
                assert _conditions("replica %d" % j, r.zs, mj, r.var) <= NEAR_SHARE
                losses.append(r.loss)
            want.setdefault(key, []).append(B.defence_vjp(wav, chain, None, normals[j], r.grad / 32768.0)[0] * 32768.0)
    mean = {k: 0.5 * (v[0] + v[1]) for k, v in want.items()}
    err_dev, err_32 = rel_l2(grad, mean["r64"]), rel_l2(mean["r32"], mean["r64"])
    err_dev_f, err_32_f = rel_l2(grad, mean["f64"]), rel_l2(mean["f32"], mean["f64"])
    apart = rel_l2(want["r64"][0], want["r64"][1])
    print("eot = 2 behind noise:8: loss %.9g (restatement %.9g); err_dev %.3g err_32 %.3g ratio %.2f; at the device's feature rows: "
          "err_dev %.3g err_32 %.3g ratio %.2f; the replicas' gradients are %.3g apart"
          % (al, 0.5 * (losses[0] + losses[1]), err_dev, err_32, err_dev / err_32, err_dev_f, err_32_f, err_dev_f / err_32_f, apart))
    assert abs(al - 0.5 * (losses[0] + losses[1])) < 1e-3
    assert apart > 1e-3                                             # the replicas differ: a mix-up would show
    assert err_32 > 0.0 and err_dev <= FACTOR * err_32
    assert err_32_f > 0.0 and err_dev_f <= FACTOR * err_32_f


# ------------------------------------------------------------------------------------- 6. attacks
def _losses(ck):
    with open(ck, "rb") as f:
        return [float(np.asarray(r[1]).reshape(-1)[0]) for r in pickle.load(f)]


@pytest.mark.parametrize("defended", [False, True])
def test_xvector_pgd_lowers_the_loss_and_the_flag_is_the_decision(tmp_path, defended):
    kw = dict(input_transform="qt:512,ms:7") if defended else {}
    model, audio, _init, thr = _sv_setting(tmp_path, **kw)
    try:
        pgd = XvectorPGD("SV", "targeted", model, bpda=defended, max_iter=12, epsilon=0.004, max_lr=0.002, seed=3, verbose=False)
        assert model.engine.wb_xvector and model.engine.wb_bpda == defended
        ck = str(tmp_path / "trace.pkl")
        adv, flag = pgd.attack(audio, ck, threshold=thr)
        losses = _losses(ck)
        xr = model.engine.debug_wb_xv_route()
        print("XvectorPGD on x-vector SV%s: adversarial loss %s, flag %d" % (" behind qt:512,ms:7" if defended else "", ["%.4g" % v for v in losses], flag))
        assert losses[0] > 0.0 and np.all(np.isfinite(losses))
        assert min(losses[1:]) < losses[0]
        assert flag == 1 or losses[-1] >= 0.0
        _agrees(model, adv, flag)
        nl = 5
        assert xr["segment_t"] >= len(losses) and xr["pool_t"] == xr["segment_t"] == xr["backend_t"]
        assert xr["act_t"] == xr["affine_t"] == xr["unsplice"] == nl * xr["segment_t"]
    finally:
        model.engine.close()


@pytest.mark.parametrize("cls,extra", [(CW2, {}), (Imperceptible, dict(window=512))], ids=["cw2", "psy"])
def test_cw2_and_imperceptible_run_a_search_step(tmp_path, cls, extra):
    model, audio, _init, thr = _sv_setting(tmp_path)
    try:
        a = cls("SV", "targeted", model, xvector=True, binary_search_steps=1, max_iter=4, initial_const=1.0, lr=1e-3, verbose=False, **extra)
        assert model.engine.wb_xvector
        ck = str(tmp_path / "trace.pkl")
        res = a.attack(audio, ck, threshold=thr)
        adv, flag = res
        losses = _losses(ck)
        print("%s on x-vector SV: adversarial loss %s, flag %d" % (cls.__name__, ["%.4g" % v for v in losses], flag))
        assert np.asarray(adv).size == audio.size and flag in (1, -1)
        assert len(losses) >= 1 and np.all(np.isfinite(losses))
        assert model.engine.debug_wb_xv_route()["segment_t"] >= len(losses)
        _agrees(model, adv, flag)
    finally:
        model.engine.close()


# ------------------------------------------------------------------------------------- 7. refusals
def _refused(call, text):
    with pytest.raises(N.NativeError) as ei:
        call()
    assert ei.value.code == N.FB_E_STATE and text in str(ei.value), str(ei.value)


def test_refusals_by_name_keep_the_loaded_system(eng72):
    e = eng72
    sy = _sys72("stock", 3)
    e.load_xvector(sy, "OSI")
    wavs = [CP.cast_i16(synthetic_audio(0, 6000), 16), CP.cast_i16(synthetic_audio(1, 3000), 16)]
    before, _ = e.score_raw(wavs)
    audio = synthetic_audio(0, 4000)
    p = nes_params("OSI", "targeted", target=1, max_iter=2)
    # the switch off: today's refusal, whatever the other five say
    others = (e.set_wb_ivector, e.set_wb_bpda, e.set_wb_air, e.set_wb_frontend, e.set_wb_universal)
    for on in (False, True, False):
        for setter in others:
            setter(on)
        _refused(lambda: e.get_grad_wb(p, audio), "x-vector system is loaded")
        _refused(lambda: e.attack_wb(p, audio), "not in this version")
    with pytest.raises(N.NativeError) as ei:
        e.set_wb_xvector(2)
    assert ei.value.code == N.FB_E_ARG and e.wb_xvector is False
    e.set_wb_xvector(True)
    try:
        g0, _al, _sc = e.get_grad_wb(p, audio)
        assert np.all(np.isfinite(g0)) and g0.any()
        # each of the four, its own switch on: refused by name
        e.set_wb_air(True)
        e.set_air_channel("t60:200-600,drr:6,taps:2048,delay:32")
        _refused(lambda: e.get_grad_wb(p, audio), "air channel")
        e.set_air_channel(None)
        e.set_wb_universal(True)
        e.set_companions([synthetic_audio(2, 4000)])
        _refused(lambda: e.get_grad_wb(p, audio), "companions")
        e.set_companions(None)
        e.set_play_offset(100)
        _refused(lambda: e.get_grad_wb(p, audio), "play offset")
        e.set_play_offset(None)
        e.set_wb_frontend(True)
        e.set_frontend(dither=1.0)
        e.load_xvector(sy, "OSI")
        _refused(lambda: e.get_grad_wb(p, audio), "dither")
        _refused(lambda: e.attack_wb(p, audio), "dither")
        e.set_frontend(dither=0.0)
        e.load_xvector(sy, "OSI")
        # EOT, a chain and a codec need the BPDA switch, as on a GMM-UBM system
        e.set_eot(2)
        _refused(lambda: e.get_grad_wb(p, audio), "fb_set_eot")
        e.set_eot(1)
        e.set_input_transform("qt:512")
        _refused(lambda: e.get_grad_wb(p, audio), "input-transform chain")
        e.set_input_transform(None)
        e.set_codec("ulaw")
        _refused(lambda: e.get_grad_wb(p, audio), "codec")
        e.set_codec(None)
        g1, _al, _sc = e.get_grad_wb(p, audio)
        assert np.array_equal(g1.view(np.uint64), g0.view(np.uint64))
    finally:
        e.set_air_channel(None)
        e.set_companions(None)
        e.set_play_offset(None)
        e.set_frontend(dither=0.0)
        for setter in (e.set_wb_air, e.set_wb_frontend, e.set_wb_universal, e.set_wb_xvector):
            setter(False)
        _clear(e)
    e.load_xvector(sy, "OSI")
    after, _ = e.score_raw(wavs)
    assert np.array_equal(after, before)


def test_the_switch_changes_no_launch_on_the_other_kinds(eng72):
    e = eng72
    audio = synthetic_audio(0, 4000)
    p = nes_params("OSI", "targeted", target=1, threshold=0.0, max_iter=3)
    ubm, spk = synthetic_gmm_system(n_speakers=3, C=256, D=72)
    iv = synthetic_ivector_system(C=64, D=72, R=32, L=16, n_speakers=3)
    try:
        for kind in ("gmm", "iv"):
            if kind == "gmm":
                e.load_gmm_arrays(*stack_models([ubm] + spk))
                e.set_system("OSI")
            else:
                e.load_ivector(iv, "OSI")
                e.set_wb_ivector(True)
            seen = []
            for on in (False, True):
                e.set_wb_xvector(on)
                g, al, sc = e.get_grad_wb(p, audio)
                seen.append((g.tobytes(), al, sc.tobytes(), tuple(sorted(e.debug_wb_route().items())), tuple(sorted(e.debug_wb_xv_route().items()))))
            assert seen[0] == seen[1], kind
            assert not any(v for _k, v in seen[0][4])
    finally:
        e.set_wb_xvector(False)
        e.set_wb_ivector(False)
