"""The restatement of the white-box gradient through feature compression and dither (tests/feco_vjp_ref.py) on the CPU: its
centres against tests/feco_ref.py's, the mean / gather pair against the adjoint identity, autograd against central differences
with the labels (and the dither normals) held constant, and the empty-cluster rule.  tests/test_gpu_wb_frontend.py compares the
kernels with it.

Bars: a centre of feco_ref is the float32 rounding of the float64 mean, so the two agree to half a float32 ulp (2^-24 relative,
plus the float64 mean's own 2^-50); the adjoint identity holds to float64 summation error (1e-12 relative); differences against
autograd as tests/test_whitebox_ref_host.py: 1e-6 relative."""
import numpy as np
import pytest
import torch

from fakebob_amd.models import stack_models
from tests import feco_vjp_ref as F
from tests import whitebox_ref as R
from tests.feco_ref import feco, feco_k

D = 72


def _stack(small_system, task):
    ubm, spk = small_system
    return stack_models(spk if task == "CSI" else ([ubm] + spk if task == "OSI" else [ubm, spk[0]]))


def _keys(T, seed):
    return np.random.RandomState(seed).randint(0, 2 ** 32, T, dtype=np.uint64).astype(np.uint32)


def _repeated_rows():
    """tests/test_gpu_feco.py's test_kernel_on_repeated_rows: 130 frames, 9 distinct rows"""
    rng = np.random.RandomState(12)
    base = (3.0 * rng.standard_normal((9, D))).astype(np.float32)
    return base[rng.randint(0, 9, 130)]


@pytest.mark.parametrize("T,ratio,iters", [(1, 0.5, 10), (65, 0.2, 1), (300, 0.5, 10), (300, 0.001, 10), (130, 1.0, 10)])
def test_centres_under_fecos_labels_are_fecos_centres(T, ratio, iters):
    X = (3.0 * np.random.RandomState(T).standard_normal((T, D))).astype(np.float32)
    C, labels = feco(X, _keys(T, 5), ratio, iters)
    k = feco_k(T, ratio)
    got = F.centres(torch.as_tensor(X.astype(np.float64)), labels, k, empty=C).numpy()
    err = np.abs(got - C.astype(np.float64))
    print("T=%d ratio=%g: max |centre - feco's| / |centre| %.3g" % (T, ratio, float((err / np.maximum(np.abs(got), 1e-30)).max())))
    assert got.shape == C.shape == (k, D)
    assert (err <= np.abs(got) * (2.0 ** -24 + 2.0 ** -50)).all()
    assert np.array_equal(got.astype(np.float32), C)


def test_the_mean_and_the_gather_are_adjoint():
    rng = np.random.default_rng(3)
    for X, ratio in (((3.0 * rng.standard_normal((257, D))).astype(np.float32), 0.2), (_repeated_rows(), 0.25)):
        T = X.shape[0]
        _C, labels = feco(X, _keys(T, 9), ratio, 10)
        k = feco_k(T, ratio)
        v, w = rng.normal(size=(T, D)), rng.normal(size=(k, D))
        Jv = F.centres(torch.as_tensor(v), labels, k, empty=np.zeros((k, D))).numpy()       # (linear: an empty centre is the constant 0)
        JTw = F.gather_t(w, labels, k)
        lhs, rhs = float((Jv * w).sum()), float((v * JTw).sum())
        print("T=%d k=%d: <J v, w> %.15g, <v, J' w> %.15g" % (T, k, lhs, rhs))
        assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), np.abs(Jv * w).sum())
        # and autograd agrees with the closed form
        f = torch.tensor(v, requires_grad=True)
        (F.centres(f, labels, k, empty=np.zeros((k, D))) * torch.as_tensor(w)).sum().backward()
        assert np.abs(f.grad.numpy() - JTw).max() <= 1e-15 * np.abs(w).max() * 4


def test_an_empty_cluster_contributes_zero():
    X = _repeated_rows()
    C, labels = feco(X, _keys(130, 9), 0.25, 10)
    k = feco_k(130, 0.25)
    n = np.bincount(labels, minlength=k)
    assert (n == 0).any() and n.sum() == 130                       # the case does hold an empty cluster
    w = np.random.default_rng(4).normal(size=(k, D))
    loud = w.copy()
    loud[n == 0] = 1e300                                            # whatever the back end sends to a centre without members
    assert np.array_equal(F.gather_t(w, labels, k), F.gather_t(loud, labels, k))
    f = torch.tensor(X.astype(np.float64), requires_grad=True)
    cen = F.centres(f, labels, k, empty=C)
    assert np.array_equal(cen.detach().numpy()[n == 0], C[n == 0].astype(np.float64))     # the value it kept, a constant
    (cen * torch.as_tensor(np.where((n == 0)[:, None], 1e6, w))).sum().backward()
    assert np.allclose(f.grad.numpy(), F.gather_t(w, labels, k), rtol=1e-13, atol=0.0)
    with pytest.raises(ValueError):
        F.centres(f, labels, k)


def _directional(fn, grad, audio, tries=3, seed=11):
    rng = np.random.default_rng(seed)
    h = 1e-3 / 32768.0   # 1e-3 LSB
    worst = 0.0
    for _ in range(tries):
        d = rng.normal(size=audio.size)
        d /= np.linalg.norm(d) / np.sqrt(audio.size)
        fd, an = (fn(audio + h * d) - fn(audio - h * d)) / (2.0 * h), float(grad @ d)
        rel = abs(fd - an) / abs(fd)
        print("  directional derivative %.10g (differences) %.10g (autograd): relative error %.3g" % (fd, an, rel))
        worst = max(worst, rel)
    return worst


@pytest.mark.parametrize("task,attack,kw", [("OSI", "targeted", dict(target=1, threshold=-10.0)), ("SV", "untargeted", dict(threshold=0.1))])
def test_gradient_with_constant_labels_against_central_differences(oracle, small_system, task, attack, kw):
    cfg = oracle.default_cfg()
    models = _stack(small_system, task)
    audio = R.test_audio(4000)
    plain = F.loss_and_grad(cfg, models, task, attack, audio, cast=False, **kw)
    rows = plain.feats[0].astype(np.float32)
    C, labels = feco(rows, _keys(rows.shape[0], 7), 0.5, 10)
    fc = dict(labels=labels, k=C.shape[0], empty=C)
    r = F.loss_and_grad(cfg, models, task, attack, audio, feco=[fc], cast=False, **kw)
    print("%s: Tv %d -> k %d, loss %.9g (undefended %.9g)" % (task, rows.shape[0], C.shape[0], r.loss, plain.loss))
    assert r.margin > 1e-3 and C.shape[0] == feco_k(rows.shape[0], 0.5) and r.loss != plain.loss

    def f(a):
        return F.loss_and_grad(cfg, models, task, attack, a, feco=[fc], cast=False, **kw).loss
    assert _directional(f, r.grad, audio) < 1e-6


def test_zero_dither_is_the_plain_front_end(oracle):
    cfg = oracle.default_cfg()
    x = torch.tensor(oracle.quantize(R.test_audio(4000)).astype(np.float64))
    T = R.num_frames(cfg, 4000)
    plain = R.mfcc(cfg, x).numpy()
    through_frames = F.mfcc(cfg, x, np.zeros((T, cfg.frame_length), np.float32), 1.0).numpy()
    assert plain.shape == through_frames.shape and np.abs(plain - through_frames).max() < 1e-12
    assert np.array_equal(F.mfcc(cfg, x, None, 1.0).numpy(), plain)
    z = np.random.default_rng(1).normal(size=(T, cfg.frame_length)).astype(np.float32)
    assert np.abs(F.mfcc(cfg, x, z, 1.0).numpy() - plain).max() > 1e-6         # and a real draw moves it


@pytest.mark.parametrize("with_feco", [False, True])
def test_gradient_through_the_dithered_front_end_against_central_differences(oracle, small_system, with_feco):
    cfg = oracle.default_cfg()
    models = _stack(small_system, "OSI")
    kw = dict(target=1, threshold=-10.0)
    audio = R.test_audio(4000)
    z = np.random.default_rng(2).normal(size=(R.num_frames(cfg, 4000), cfg.frame_length)).astype(np.float32)
    first = F.loss_and_grad(cfg, models, "OSI", "targeted", audio, dither=[z], amp=1.0, cast=False, **kw)
    fc = None
    if with_feco:
        rows = first.feats[0].astype(np.float32)
        C, labels = feco(rows, _keys(rows.shape[0], 8), 0.5, 10)
        fc = dict(labels=labels, k=C.shape[0], empty=C)
    r = F.loss_and_grad(cfg, models, "OSI", "targeted", audio, feco=[fc], dither=[z], amp=1.0, cast=False, **kw)
    undithered = F.loss_and_grad(cfg, models, "OSI", "targeted", audio, feco=[fc] if not with_feco else [None], cast=False, **kw)
    print("dither 1.0%s: loss %.9g (without either %.9g), min |c0 - thr| %.3g" % (" + FeCo" if with_feco else "", r.loss, undithered.loss, r.margin))
    assert r.margin > 1e-3 and r.loss != undithered.loss

    def f(a):
        return F.loss_and_grad(cfg, models, "OSI", "targeted", a, feco=[fc], dither=[z], amp=1.0, cast=False, **kw).loss
    assert _directional(f, r.grad, audio) < 1e-6
