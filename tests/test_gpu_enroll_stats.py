"""Enrolment statistics on rows handed in as they are (Engine.debug_gmm_acc_rows: the launches of fb_gmm_acc_stats without
its front-end) against the plain numpy references of tests/enroll_ref.py, at the edges of the kernels: the dump's padded
32-component tile and its component chunks, k_gmm_post_stats' 64-component slabs, 64-row staging rounds and its four
dimension groups, k_gmm_lse's 64 lanes.  Three assertions, each with its own reference:

  (a) the dump, per component:  |ll_dev - ll64| <= 2e-6 max(1, S) for every (row, component)
  (b) k_gmm_lse + k_gmm_post_stats alone, against float64 on the DEVICE'S OWN ll (the dump's error cancels):
      |occ_dev - occ_ref|_k <= gamma occ_ref,k, |F_dev - F_ref|_kd <= gamma A_kd, |sum occ_dev - T| <= gamma T,
      gamma = max(32 ulp, 4 g_K), g_K the distance of the Kaldi-order float32 soft-max from float64 on the same ll
  (c) end to end against float64: the first-order bound that follows from (a) and (b)

The models are the synthetic UBM with its means pulled together (enroll_ref.overlapping_ubm): a frame's posterior is
shared among 6 .. 100 components and every component is occupied (tests/test_enroll_ref_host.py asserts it).

Measured worst error / tolerance (MI355X):
  rows                                   kernel  (a) error / bound          (b)     (c)
  shared  C   64 D 39 T   65             fx2     0.170  (3.4e-7 S)          0.048   0.036
  shared  C   65 D 77 T  129             fx2     0.147  (2.9e-7 S)          0.052   0.021
  shared  C  100 D 60 T  130             fx2     0.134  (2.7e-7 S)          0.047   0.021
  shared  C  160 D 72 T  300             fx2     0.162  (3.2e-7 S)          0.058   0.020
  shared  C   96 D 80 T 1100             fx2     0.150  (3.0e-7 S)          0.030   0.015
  shared  C 2048 D 72 T  130             fx2     0.168  (3.4e-7 S)          0.018   0.040   (gamma 7.9e-6: g_K = 2.0e-6)
  shared  C  100 D 60 T  130             bx3     0.122  (2.4e-7 S)          0.051   0.019
  shared  C   65 D 77 T  129             bx3     0.130  (2.6e-7 S)          0.043   0.022
  prefixes of 1 .. 129 rows, both models fx2     0.068 .. 0.147             0.047 .. 0.082   0.021 .. 0.057
                                         bx3     0.060 .. 0.130             0.043 .. 0.054   0.019 .. 0.053
  shared + far + zero + huge + shared    fx2     0.300, 0.311  (6.2e-7 S)   0.044, 0.045
                                         bx3     0.391, 0.301  (7.8e-7 S)   0.044, 0.043
gamma is its floor, 32 ulp = 1.9e-6, everywhere but at C = 2048; g_K = 1.7e-7 .. 4.7e-7 below C = 2048.  The dump's
per-component error is that of the same formula in float32 on the CPU (2.8e-7 S).

What the mixed batch found: k_gmm_fx2 moved the frame operands of a whole WAVE of 32 frames down by one power of two when
one of them left f16's range, so the ordinary rows next to the rows of magnitude 1e4 lost their operands' second terms:
(a) 70.5 and 80.3 (1.4e-4 S and 1.6e-4 S; bx3: 0.39, 0.30).  The shift is now every frame's own (gmm_split.h).
"""
import os

import numpy as np
import pytest

from fakebob_amd import _native as N
from fakebob_amd import enroll as EN
from fakebob_amd.engine import Engine
from fakebob_amd.models import synthetic_audio, synthetic_gmm_system
from tests import enroll_ref as ER

pytestmark = pytest.mark.gpu
EDGE_MODELS = [(100, 60, 130), (65, 77, 129)]
MODES = [None, "bx3"]                       # None: the engine's own choice, fx2 for these parameters
# a model's dimension has to be the front-end's (num_ceps x (delta_order + 1)), though no front-end runs here
FRONTEND = {39: dict(num_ceps=13, delta_order=2), 60: dict(num_ceps=20, delta_order=2), 72: dict(),
            77: dict(num_ceps=77, num_mel_bins=77, delta_order=0), 80: dict(num_ceps=20, delta_order=3, delta_window=2)}


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    for k in list(os.environ):
        if k.startswith("FB_GMM_"):
            monkeypatch.delenv(k)
    return monkeypatch


def _engine(gmm, mode, monkeypatch):
    if mode:
        monkeypatch.setenv("FB_GMM_MODE", mode)
    e = Engine(0)
    try:
        e.set_frontend(**FRONTEND[gmm.dim])
        e.load_gmm([gmm])
        assert e.gmm_kernel == (mode or "fx2")
    except Exception:
        e.close()
        raise
    return e


def _fresh(gmm, mode, monkeypatch, x):
    e = _engine(gmm, mode, monkeypatch)
    try:
        occ, F, ll = e.debug_gmm_acc_rows(x, want_ll=True)
    finally:
        e.close()
    assert ll.shape == (x.shape[0], gmm.num_gauss) and ll.dtype == np.float32   # no padded column comes back
    assert occ.shape == (gmm.num_gauss,) and F.shape == (gmm.num_gauss, gmm.dim)
    return occ, F, ll


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _check(label, gmm, x, occ, F, ll, with_c=True):
    """print, then assert (a), (b) and (c)"""
    gc, miv, iv = ER.params(gmm)
    assert np.isfinite(ll).all() and np.isfinite(occ).all() and np.isfinite(F).all()
    ra, at = ER.ratio_a(ll, gc, miv, iv, x, where=True)
    rb, g, g_K, _ = ER.ratios_b(occ, F, ll, x)
    rc = ER.ratio_c(occ, F, gc, miv, iv, x, g) if with_c else float("nan")
    err_S = ra * ER.EPS_LL
    print("%s: (a) %.3f (%.2e S)  (b) %.3f (gamma %.2e, g_K %.2e)  (c) %.3f" % (label, ra, err_S, rb, g, g_K, rc))
    assert ra <= 1.0, "(a) the dump, worst at (row, component) %s" % (at,)
    assert rb <= 1.0, "(b) k_gmm_lse + k_gmm_post_stats"
    if with_c:
        assert rc <= 1.0, "(c) end to end"


@pytest.mark.parametrize("C,D,T,mode", [s + (None,) for s in ER.SHAPES] + [s + ("bx3",) for s in EDGE_MODELS])
def test_shared_rows(C, D, T, mode, clean_env):
    gmm = ER.overlapping_ubm(C, D)
    x = ER.shared(C, D, T)
    occ, F, ll = _fresh(gmm, mode, clean_env, x)
    _check("shared C %d D %d T %d %s" % (C, D, T, mode or "fx2"), gmm, x, occ, F, ll)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("C,D,T", EDGE_MODELS)
def test_row_counts_and_stale_buffers(C, D, T, mode, clean_env):
    """1, 63, 64, 65, 128, 129 rows (prefixes of the same rows), each on a fresh engine; then 129, 1, 65, 64 on ONE engine,
    the stale mx / inv_sum / dump rows of a longer call behind a shorter one: the same bits."""
    gmm = ER.overlapping_ubm(C, D)
    x = ER.shared(C, D, 129)
    fresh = {}
    for n in (1, 63, 64, 65, 128, 129):
        fresh[n] = _fresh(gmm, mode, clean_env, x[:n])
        _check("prefix %d of C %d D %d %s" % (n, C, D, mode or "fx2"), gmm, x[:n], *fresh[n])
    e = _engine(gmm, mode, clean_env)
    try:
        for n in (129, 1, 65, 64):
            got = e.debug_gmm_acc_rows(x[:n], want_ll=True)
            for a, b, what in zip(got, fresh[n], ("occ", "F", "ll")):
                assert np.array_equal(_bits(a), _bits(b)), (n, what)
            occ2, F2 = e.debug_gmm_acc_rows(x[:n])                      # without the dump copied out: the same statistics
            assert np.array_equal(_bits(occ2), _bits(got[0])) and np.array_equal(_bits(F2), _bits(got[1]))
    finally:
        e.close()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("C,D,T", EDGE_MODELS)
def test_rows_the_front_end_never_makes(C, D, T, mode, clean_env):
    gmm = ER.overlapping_ubm(C, D)
    sh = ER.shared(C, D, T)
    x = np.concatenate([sh, ER.far(C, D, 70), ER.zero(D, 7), ER.huge(D, 40), sh])
    occ, F, ll = _fresh(gmm, mode, clean_env, x)
    # (c) says nothing here: for the huge rows 2e-6 S is thousands of nats, a float64 posterior is not the device's
    _check("mixed C %d D %d T %d %s" % (C, D, x.shape[0], mode or "fx2"), gmm, x, occ, F, ll, with_c=False)
    _check("its shared rows alone", gmm, sh, *_fresh(gmm, mode, clean_env, sh))


@pytest.mark.parametrize("C,D,T", EDGE_MODELS)
def test_component_with_no_mass(C, D, T, clean_env):
    """rows on components 0 .. 31 of the UNSHRUNK UBM (one-hot posteriors; the other components' mass is tiny), and the
    same pushed out to 8 mu_k, where float32 gives most components exactly nothing: empty in the Kaldi-order soft-max of
    the device's ll = empty on the device, and MAP adaptation leaves such a component's parameters bit-identical."""
    ubm, _ = synthetic_gmm_system(1, C, D)
    w, _, _ = ER.moments(C, D)
    e = Engine(0)
    try:
        e.set_frontend(**FRONTEND[D])
        e.load_gmm([ubm])
        for out, n_empty in [(1.0, 0), (8.0, 8)]:
            x = ER.one_hot_rows(C, D, T, out=out)
            occ, F, ll = e.debug_gmm_acc_rows(x, want_ll=True)
            assert np.isfinite(ll).all() and np.isfinite(occ).all() and np.isfinite(F).all()
            occ_k, F_k, _ = ER.stats_kaldi(ll, x)
            empty = occ_k == 0.0
            print("C %d D %d rows at %g mu (%s): %d components empty in the twin, %d on the device; |sum occ - T| = %.2e"
                  % (C, D, out, e.gmm_kernel, empty.sum(), (occ == 0.0).sum(), abs(occ.sum() - T)))
            assert empty.sum() >= n_empty
            assert np.all(occ[empty] == 0.0) and np.all(F[empty] == 0.0)
            g = ER.ratios_b(occ, F, ll, x)[1]
            assert abs(occ.sum() - T) <= g * T
            new = EN.map_adapt_means(ubm, w, occ, F)
            keep = occ == 0.0
            assert np.array_equal(_bits(new.means_invvars[keep]), _bits(ubm.means_invvars[keep]))
            assert np.array_equal(_bits(new.inv_vars), _bits(ubm.inv_vars))
            moved = np.abs(new.means_invvars - ubm.means_invvars).max(axis=1)
            assert np.all(moved[occ > 0.5] > 0)
    finally:
        e.close()


def test_hook_and_product_call_run_the_same_code(clean_env):
    """fb_gmm_acc_stats = its front-end + the launches of the hook.  The product call sizes the dump for all frames of the
    utterance, the hook for the voiced ones: the chunk counts may differ, a component's value does not depend on them."""
    gmm = ER.overlapping_ubm(160, 72)
    e = _engine(gmm, None, clean_env)
    try:
        for utt, n in [(21, 48000), (22, 160000)]:
            wav = (synthetic_audio(utt, n) * 32768.0).astype(np.int16)
            occ, F, tv = e.gmm_acc_stats(wav)
            feats, n_frames = e.debug_feats(wav)
            assert feats.shape[0] == tv and tv < n_frames
            occ_h, F_h = e.debug_gmm_acc_rows(feats)
            assert np.array_equal(_bits(occ), _bits(occ_h)) and np.array_equal(_bits(F), _bits(F_h))
    finally:
        e.close()
    e2 = Engine(0)                                                     # as fb_gmm_acc_stats: the UBM loaded alone
    try:
        u, s = synthetic_gmm_system(2, 64, 72)
        e2.load_gmm([u] + s)
        with pytest.raises(N.NativeError) as ei:
            e2.debug_gmm_acc_rows(np.zeros((3, 72), np.float32))
        assert ei.value.code == N.FB_E_STATE
    finally:
        e2.close()
