"""White-box gradients through the x-vector (TDNN) victim: the host side.  No GPU: the restatement tests/xvector_vjp_ref.py
against tests/xvector_ref.py and a finite difference, the pooling floor's rule, the fixture conditions of
tests/test_gpu_xvector_whitebox.py on the CPU, the transposed weight images against numpy, header text and exports, and
XvectorPGD / CW2 / Imperceptible on stub engines."""
import ctypes as C
import inspect
import re

import numpy as np
import pytest
import torch

from fakebob_amd import _native as N
from fakebob_amd import prepare
from fakebob_amd.cw2 import CW2
from fakebob_amd.engine import Engine
from fakebob_amd.models import STOCK_XV_CONTEXTS, synthetic_audio, synthetic_xvector_system
from fakebob_amd.pgd import PGD, AdaptivePGD, IvectorPGD, XvectorPGD
from fakebob_amd.psy import Imperceptible
from tests import whitebox_ref as W
from tests import xvector_ref as X
from tests import xvector_vjp_ref as V
from tests.test_whitebox_host import _Engine, _header

D = 24
LENGTHS = [33, 1, 70, 2, 32, 15, 31]
SHAPES = {"stock": dict(hidden=64), "hidden96": dict(hidden=96), "one-layer": dict(contexts=(STOCK_XV_CONTEXTS[0],)),
          "partial-tiles": dict(hidden=76, pool=100)}


def _system(hidden=64, contexts=STOCK_XV_CONTEXTS, n_speakers=3, seed=11, pool=96, dim=D):
    sy = synthetic_xvector_system(dim, hidden=hidden, pool=pool, R=64, L=32, n_speakers=n_speakers, seed=seed, contexts=contexts)
    return sy.with_enrolled(sy.enrolled, [-30.0, -50.0, -20.0][:n_speakers], [5.0, 8.0, 4.0][:n_speakers])


def _rows(dim=D, lengths=LENGTHS, seed=3):
    rng = np.random.default_rng(seed)
    return [(3.0 * rng.normal(size=(t, dim))).astype(np.float32) for t in lengths]


def _rel(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


# ------------------------------------------------------------------------------------------------ the restatement
def test_forward_is_xvector_refs():
    sy = _system()
    for x in _rows()[:4]:
        for dt in (torch.float64, torch.float32):
            outs, st, emb = X.stages(sy, x, dt)
            with torch.no_grad():
                f = V.embed(sy, torch.as_tensor(x.astype(np.float64)), dt)
            assert np.array_equal(f.emb.numpy(), emb) and np.array_equal(f.stats.numpy(), st)
            for h, o in zip(f.hs[1:], outs):
                assert np.array_equal(h.to(torch.float64).numpy(), o)
    emb = np.stack([X.stages(sy, x)[2] for x in _rows()[:3]])
    want = X.plda_llr(sy, emb)
    got = np.stack([V.backend_llr(sy, torch.as_tensor(e)).numpy() for e in emb])
    assert np.abs(got - want).max() <= 1e-9 * np.abs(want).max()


def test_masks_change_the_derivative_only():
    sy = _system()
    x = _rows()[0]
    ebar = np.random.default_rng(1).normal(size=sy.R)
    a = V.feat_grad(sy, x, ebar)
    own = [(z > 0).astype(np.uint8) for z in a.zs]
    b = V.feat_grad(sy, x, ebar, masks=own)
    assert np.array_equal(a.emb, b.emb)
    for ga, gb in zip(a.grads, b.grads):
        assert np.array_equal(ga, gb)
    flipped = [m.copy() for m in own]
    flipped[1][:, :8] ^= 1
    c = V.feat_grad(sy, x, ebar, masks=flipped)
    assert np.array_equal(a.emb, c.emb) and not np.array_equal(a.grads[0], c.grads[0])


def test_feature_gradient_against_a_central_difference():
    sy = _system()
    x = _rows()[5].astype(np.float64)                     # 15 rows
    ebar = np.random.default_rng(2).normal(size=sy.R)
    g = V.feat_grad(sy, x, ebar).grads[0]

    def f(v):
        with torch.no_grad():
            return float((V.embed(sy, torch.as_tensor(v)).emb * torch.as_tensor(ebar)).sum())
    rng = np.random.default_rng(3)
    worst = 0.0
    for _ in range(6):
        d = rng.normal(size=x.shape)
        d /= np.linalg.norm(d)
        h = 1e-6
        fd = (f(x + h * d) - f(x - h * d)) / (2 * h)
        worst = max(worst, abs(fd - float((g * d).sum())) / np.linalg.norm(g))
    print("directional derivative against a central difference: %.3g of |g|" % worst)
    assert worst <= 1e-6


def test_loss_gradient_against_a_central_difference_of_the_uncast_function():
    cfg = N.FrontendCfg()
    N.lib().fb_default_frontend(C.byref(cfg))
    cfg.delta_order = 0
    sy = _system()
    audio = synthetic_audio(0, 2000)
    kw = dict(threshold=0.1, adver_thresh=0.05, target=1)
    r = V.loss_and_grad_xv(cfg, sy, "OSI", "targeted", audio, cast=False, **kw)
    rng = np.random.default_rng(4)
    worst = 0.0
    for _ in range(3):
        d = rng.normal(size=audio.shape)
        d /= np.linalg.norm(d)
        h = 1e-7
        lp = V.loss_and_grad_xv(cfg, sy, "OSI", "targeted", audio + h * d, cast=False, want_grad=False, **kw).loss
        lm = V.loss_and_grad_xv(cfg, sy, "OSI", "targeted", audio - h * d, cast=False, want_grad=False, **kw).loss
        worst = max(worst, abs((lp - lm) / (2 * h) - float(r.grad @ d)) / np.linalg.norm(r.grad))
    print("loss: directional derivative against a central difference: %.3g of |g|" % worst)
    assert worst <= 1e-5
    # the cast is straight-through: the same derivative at the truncated audio, and the forward is get_grad's loss
    rc = V.loss_and_grad_xv(cfg, sy, "OSI", "targeted", audio, **kw)
    assert _rel(rc.grad, r.grad) <= 1e-3 and abs(rc.loss - r.loss) <= 1e-3 * abs(r.loss)


def test_the_variance_floor_passes_nothing():
    sy = _system()
    layers = [dict(ly) for ly in sy.layers]
    layers[-1]["bn_scale"] = layers[-1]["bn_scale"].copy()
    layers[-1]["bn_scale"][:5] = 0.0                      # five constant channels: their variance is zero
    P, R = sy.P, sy.R
    only_std = sy.seg_W.copy()
    only_std[:, :P] = 0.0                                 # the embedding reads the standard deviations alone ...
    only_std[:, P + 5:] = 0.0                             # ... and of the floored channels alone
    fl = type(sy)(sy.D, layers, only_std, sy.seg_bias, sy.mean_vec, sy.lda, sy.plda_mean, sy.plda_transform, sy.plda_psi,
                  sy.enrolled, sy.z_mean, sy.z_std)
    ebar = np.random.default_rng(5).normal(size=R)
    r = V.feat_grad(fl, _rows()[0], ebar)
    assert np.all(r.var[:5] <= 1e-10) and np.all(r.stats[P:P + 5] == np.sqrt(1e-10))
    assert np.all(r.grads[-1][P:P + 5] != 0.0)            # the cotangent arrives at the statistics ...
    assert all(np.all(g == 0.0) for g in r.grads[:-1])    # ... and goes no further
    # a one-row utterance: every channel's variance is zero
    std_all = sy.seg_W.copy()
    std_all[:, :P] = 0.0
    one = type(sy)(sy.D, sy.layers, std_all, sy.seg_bias, sy.mean_vec, sy.lda, sy.plda_mean, sy.plda_transform, sy.plda_psi,
                   sy.enrolled, sy.z_mean, sy.z_std)
    r1 = V.feat_grad(one, _rows()[1], ebar)
    assert r1.grads[0].shape == (1, D) and all(np.all(g == 0.0) for g in r1.grads[:-1]) and np.any(r1.grads[-1] != 0.0)
    r33 = V.feat_grad(one, _rows()[0], ebar)
    assert np.any(r33.grads[0] != 0.0)                    # (with 33 rows the same system does pass a gradient)


# ------------------------------------------------------------------------------------------------ the GPU fixture, on the CPU
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_fixture_conditions_of_the_gpu_test_hold_on_the_cpu(name):
    sy = _system(**SHAPES[name])
    rng = np.random.default_rng(17)
    near = total = 0
    floored = 0
    errs = []
    for x in _rows():
        ebar = rng.normal(size=sy.R)
        r64 = V.feat_grad(sy, x, ebar)
        own64 = [(z > 0).astype(np.uint8) for z in r64.zs]
        r32own = V.feat_grad(sy, x, ebar, torch.float32)
        own32 = [(z > 0).astype(np.uint8) for z in r32own.zs]
        flips, frac, near_floor = V.mask_conditions(r64.zs, own32, r64.var)
        assert flips == 0 and near_floor == 0, (name, x.shape[0], flips, near_floor)
        near += sum(int(np.sum(np.abs(z) < 1e-4 * np.abs(z).max())) for z in r64.zs)
        total += sum(z.size for z in r64.zs)
        floored += int(np.sum(r64.var <= 1e-10))
        r32 = V.feat_grad(sy, x, ebar, torch.float32, masks=own64)
        if x.shape[0] > 1:
            errs.append(_rel(r32.grads[0], r64.grads[0]))
    print("%s: %.4f %% of units near an edge, %d floored channels, err_32 %.3g .. %.3g" %
          (name, 100.0 * near / total, floored, min(errs), max(errs)))
    assert near <= 0.0007 * total
    assert floored >= sy.P                                # the one-row utterance: every channel
    if len(sy.layers) > 1:
        assert floored > sy.P                             # ... and channels of longer utterances that a ReLU holds at zero
    assert 1e-7 < min(errs) and max(errs) < 3e-6


# ------------------------------------------------------------------------------------------------ host images
@pytest.mark.parametrize("l", [0, 1, 4])
def test_transposed_weight_images_against_numpy(l):
    sy = _system(pool=100)                                # 100 channels: the last K step of layer 4's image is partial
    img = prepare.xvector_buffer(sy, "wt%d" % l)
    kwt = int(prepare.xvector_buffer(sy, "kwt")[l])
    assert kwt == int(prepare.xvector_buffer(sy, "kw")[l])
    Wt = np.ascontiguousarray(sy.layers[l]["W"].T)        # [K][dout]
    K, dout = Wt.shape
    n_steps, tiles = (dout + 15) // 16, (K + 31) // 32
    assert img.size == tiles * n_steps * 2 * 64 * 8
    img = img.reshape(tiles, n_steps, 2, 2, 32, 8)        # tile, step, term, contraction half, column place, place
    Wp = np.zeros((tiles * 32, n_steps * 16), np.float32)
    Wp[:K, :dout] = np.ldexp(Wt, -kwt)
    hi = Wp.astype(np.float16)
    lo = (Wp - hi.astype(np.float32)).astype(np.float16)
    for term, part in ((0, hi), (1, lo)):
        want = part.view(np.uint16).reshape(tiles, 32, n_steps, 2, 8).transpose(0, 2, 3, 1, 4)
        assert np.array_equal(img[:, :, term], want), term
    # the forward's image is as it was
    fw = prepare.xvector_buffer(sy, "w%d" % l)
    assert fw.size == ((dout + 31) // 32) * ((K + 15) // 16) * 2 * 64 * 8
    with pytest.raises(N.NativeError) as ei:
        prepare.xvector_buffer(sy, "wt7")
    assert "no x-vector buffer" in str(ei.value)


# ------------------------------------------------------------------------------------------------ interface
def test_entry_points_are_declared_and_exported():
    pub, hooks = _header("fakebob_hip.h"), _header("fakebob_hip_test.h")
    assert re.search(r"int fb_set_wb_xvector\(fb_engine \*e, int on\);", pub)
    assert re.search(r"int fb_debug_xv_backward\(fb_engine \*e, const float \*feats, const int \*row_off, int B, "
                     r"const double \*ebar /\*\[B\]\[R\]\*/, int stage,\s+void \*out, int64_t cap\);", hooks)
    assert re.search(r"int fb_debug_xv_masks\(fb_engine \*e, int layer, unsigned char \*out, int64_t cap, int64_t \*size\);", hooks)
    assert re.search(r"int fb_debug_wb_xv_route\(fb_engine \*e, int \*info\);", hooks)
    for word in ("fb_set_wb_xvector", "k_wb_xv_segment_t", "k_wb_xv_pool_t", "k_wb_xv_act_t", "k_wb_xv_affine_t", "k_wb_xv_unsplice",
                 "y == bn_offset does not imply z <= 0", "mbar / T", "sbar (h - mean) / (T std)", "no floating-point atomics"):
        assert word in pub, word
    for word in ("FB_WB_XV_ROUTE_BACKEND_T 0", "FB_WB_XV_ROUTE_UNSPLICE 5", "FB_WB_XV_ROUTE_N 6", "FB_WB_ROUTE_N 9"):
        assert word in hooks, word
    lib = C.CDLL(N.LIB_PATH)
    for name in ("fb_set_wb_xvector", "fb_debug_xv_backward", "fb_debug_xv_masks", "fb_debug_wb_xv_route"):
        assert name in N.EXPORTS
        getattr(lib, name)


def test_signatures():
    assert list(inspect.signature(Engine.set_wb_xvector).parameters) == ["self", "on"]
    assert list(inspect.signature(Engine.debug_xv_backward).parameters) == ["self", "mats", "ebar", "stage"]
    assert list(inspect.signature(Engine.debug_xv_masks).parameters) == ["self", "layer"]
    assert list(inspect.signature(Engine.debug_wb_xv_route).parameters) == ["self"]
    assert "set_wb_xvector" in Engine.get_grad_wb_iter.__doc__ and "set_wb_xvector" in Engine.attack_wb.__doc__
    xv = inspect.signature(XvectorPGD.__init__).parameters
    assert list(xv)[:6] == ["self", "task", "attack_type", "model", "bpda", "eot_size"]
    assert xv["bpda"].default is False and xv["eot_size"].default == 1
    assert XvectorPGD.KINDS == ("gmm", "xv") and PGD.KINDS == ("gmm",) and IvectorPGD.KINDS == ("gmm", "iv")
    for name in ("attack", "get_grad", "estimate_threshold", "_params"):
        assert getattr(XvectorPGD, name) is getattr(PGD, name)


class _XvEngine(_Engine):
    def __init__(self, S, kind):
        _Engine.__init__(self, S)
        self.kind, self.switches = kind, []

    def set_wb_xvector(self, on):
        self.switches.append(("xvector", on))

    def set_wb_ivector(self, on):
        self.switches.append(("ivector", on))

    def set_wb_bpda(self, on):
        self.switches.append(("bpda", on))

    def set_eot(self, r):
        self.switches.append(("eot", r))


class _XvModel(object):
    def __init__(self, task, S, kind):
        self.task, self.engine = task, _XvEngine(S, kind)


@pytest.mark.parametrize("kind", ["xv", "gmm"])
@pytest.mark.parametrize("bpda,eot", [(False, 1), (True, 1), (True, 4)])
def test_xvector_pgd_sets_the_switch_and_marshals_as_pgd(tmp_path, kind, bpda, eot):
    m = _XvModel("OSI", 3, kind)
    pg = XvectorPGD("OSI", "targeted", m, bpda=bpda, eot_size=eot, adver_thresh=0.5, epsilon=0.003, max_iter=9, max_lr=2e-3, min_lr=1e-5,
                    momentum=0.0, plateau_length=4, plateau_drop=3.0, seed=7, verbose=False)
    assert m.engine.switches == [("xvector", True)] + ([("eot", eot), ("bpda", True)] if bpda else [])
    assert pg.bpda is bpda and pg.eot_size == eot
    adv, flag = pg.attack(np.linspace(-0.5, 0.5, 40), str(tmp_path / "a.cp"), threshold=0.25, target=2, bits_per_sample=12)
    assert adv.dtype == np.int16 and adv.shape == (40, 1) and flag == 1
    assert m.engine.calls == [("wb", 0, 9, 0.003, 2e-3, 1e-5, 0.0, 4, 3.0, 0.25, 2, 0, 0.5, 12)]
    assert pg._params().seed == (7 if bpda else 0)        # the seed keys a defended victim's draws only


def test_eot_needs_bpda_and_the_other_classes_refuse_an_xvector_engine():
    with pytest.raises(ValueError, match="bpda=True"):
        XvectorPGD("OSI", "targeted", _XvModel("OSI", 3, "xv"), eot_size=2)
    with pytest.raises(ValueError, match="eot_size"):
        XvectorPGD("OSI", "targeted", _XvModel("OSI", 3, "xv"), bpda=True, eot_size=33)
    for cls, kw in ((PGD, {}), (AdaptivePGD, dict(bpda=True)), (IvectorPGD, {})):
        m = _XvModel("OSI", 3, "xv")
        with pytest.raises(ValueError, match="x-vector"):
            cls("OSI", "targeted", m, **kw)
        assert m.engine.switches == []
    with pytest.raises(ValueError):
        XvectorPGD("OSI", "targeted", _XvModel("OSI", 3, "iv"))
    with pytest.raises(TypeError):
        XvectorPGD("OSI", "targeted", object())


@pytest.mark.parametrize("cls,extra", [(CW2, {}), (Imperceptible, dict(window=512))])
def test_cw2_and_imperceptible_take_xvector(cls, extra):
    m = _XvModel("OSI", 3, "xv")
    with pytest.raises(ValueError, match="xvector=True"):
        cls("OSI", "targeted", m, verbose=False, **extra)
    assert m.engine.switches == []
    a = cls("OSI", "targeted", m, xvector=True, verbose=False, **extra)
    assert m.engine.switches == [("xvector", True)] and a.xvector is True and a.ivector is False
    m2 = _XvModel("OSI", 3, "xv")
    cls("OSI", "targeted", m2, xvector=True, bpda=True, eot_size=2, verbose=False, **extra)
    assert m2.engine.switches == [("xvector", True), ("eot", 2), ("bpda", True)]
    g = _XvModel("OSI", 3, "gmm")
    b = cls("OSI", "targeted", g, verbose=False, **extra)
    assert g.engine.switches == [] and b.xvector is False
    iv = _XvModel("OSI", 3, "iv")
    with pytest.raises(ValueError, match="ivector=True"):
        cls("OSI", "targeted", iv, xvector=True, verbose=False, **extra)
