"""tests/enroll_ref.py without a GPU: the conditions tests/test_gpu_enroll_stats.py relies on for every one of its shapes,
the distance of the Kaldi-order soft-max from float64 (the unit of that file's tolerance (b)), the oracle's
fbo_gmm_acc_stats against the numpy twin, and that the three assertions of the GPU tests catch four one-line mistakes of a
posterior kernel (run here on a numpy model of k_gmm_lse + k_gmm_post_stats)."""
import ctypes
import ctypes.util

import numpy as np
import pytest

from fakebob_amd.models import stack_models, synthetic_audio, synthetic_gmm_system
from tests import enroll_ref as ER


@pytest.mark.parametrize("C,D,T", ER.SHAPES)
def test_shared_rows_share_their_posteriors_and_fill_every_component(C, D, T):
    gmm = ER.overlapping_ubm(C, D)
    gc, miv, iv = ER.params(gmm)
    x = ER.shared(C, D, T)
    assert x.shape == (T, D) and x.dtype == np.float32
    p = ER.posteriors64(ER.ll64(gc, miv, iv, x))
    top, occ = p.max(axis=1).mean(), p.sum(axis=0)
    neff = (1.0 / (p * p).sum(axis=1)).mean()
    s_over_ll = (ER.S(gc, miv, iv, x) / np.abs(ER.ll64(gc, miv, iv, x))).max()
    print("C %d D %d T %d: mean largest posterior %.3f, effective components %.1f, smallest occ %.4f, S / |ll| <= %.3f"
          % (C, D, T, top, neff, occ.min(), s_over_ll))
    assert top <= 0.5
    assert occ.min() > 1e-3
    # the parameters fit f16's range, so the engine's default dump is fx2
    assert np.abs(miv).max() < 2.0 and 0.5 * iv.max() < 7.0 and np.abs(gc).max() < 89.0


@pytest.mark.parametrize("C,D,T", ER.SHAPES + [(1000, 72, 130)])
def test_kaldi_order_softmax_distance_from_float64(C, D, T):
    """Both soft-maxes fed the SAME float32 ll.  The sequential float32 sum of C terms in (0, 1] is off by at most
    (C - 1) ulps of the sum, the 64-lane order by ceil(C / 64) - 1 + 6; exp, the reciprocal, the product and the rounding of
    ll - max add a few more (|ll - max| < 32 wherever the posterior matters: 16 ulps of 1)."""
    gc, miv, iv = ER.params(ER.overlapping_ubm(C, D))
    x = ER.shared(C, D, T)
    ll32 = ER.ll64(gc, miv, iv, x).astype(np.float32)
    ref = ER.stats64(ll32, x)
    g_seq = ER.twin_distance(ER.stats_kaldi(ll32, x), ref)
    g_lanes = ER.twin_distance(ER.stats_lanes(ll32, x), ref)
    print("C %d D %d T %d: g_K sequential %.2e, 64 lanes + butterfly %.2e" % (C, D, T, g_seq, g_lanes))
    u = 2.0 ** -24
    assert g_seq <= (C - 1 + 20) * u
    assert g_lanes <= ((C + 63) // 64 - 1 + 6 + 20) * u
    assert g_lanes <= ER.gamma(g_seq)                       # the order of the device's sum fits tolerance (b)


def _oracle_ll32(gc, miv, iv, feats):
    """fbo_gmm_acc_stats' component log-likelihoods, operation by operation"""
    x = feats.astype(np.float64)
    x2 = (feats * feats).astype(np.float32).astype(np.float64)
    a = np.zeros((feats.shape[0], gc.shape[0]))
    b = np.zeros_like(a)
    m, v = miv.astype(np.float64), iv.astype(np.float64)
    for d in range(feats.shape[1]):
        a += m[None, :, d] * x[:, d:d + 1]
        b += v[None, :, d] * x2[:, d:d + 1]
    return (gc.astype(np.float64)[None, :] + a - 0.5 * b).astype(np.float32)


def test_oracle_acc_stats_is_the_kaldi_twin(oracle):
    ubm, _ = synthetic_gmm_system(1, 48, 72)
    gc, miv, iv = stack_models([ubm])
    cfg = oracle.default_cfg()
    wav = (synthetic_audio(5, 32000) * 32768.0).astype(np.int16)
    occ, F, tv = oracle.gmm_acc_stats(cfg, wav, gc[0], miv[0], iv[0])
    feats, _ = oracle.frontend(cfg, wav)
    assert feats.shape[0] == tv
    libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    libm.expf.restype, libm.expf.argtypes = ctypes.c_float, [ctypes.c_float]
    c_expf = np.frompyfunc(lambda v: libm.expf(float(v)), 1, 1)          # the oracle's own expf, not numpy's
    occ_t, F_t, A_t = ER.stats_kaldi(_oracle_ll32(gc[0], miv[0], iv[0], feats), feats,
                                     expf=lambda a: c_expf(a).astype(np.float32))
    # the same float64 additions in the same order
    assert np.abs(occ - occ_t).max() <= 1e-13 * occ.max()
    assert np.abs(F - F_t).max() <= 1e-13 * A_t.max()
    # and numpy's float32 exp in its place moves nothing past the twin's distance from float64
    occ_n, F_n, _ = ER.stats_kaldi(_oracle_ll32(gc[0], miv[0], iv[0], feats), feats)
    assert np.abs(occ - occ_n).max() <= 4 * 2.0 ** -24 * occ.max()


def _device_model(ll32, x, C, D, mutate=None):
    """numpy model of k_gmm_lse + k_gmm_post_stats on a [T][C] dump, with one mistake put in"""
    ll32 = np.ascontiguousarray(ll32, np.float32)
    T = ll32.shape[0]
    mx = ll32.max(axis=1, keepdims=True)
    e = np.exp((ll32 - mx).astype(np.float32))
    inv = (np.float32(1.0) / ER._lane_sum32(e)).astype(np.float32)
    if mutate == "inv_sum0":
        inv = np.full(T, inv[0], np.float32)
    p = (e * inv[:, None]).astype(np.float32).astype(np.float64)
    if mutate == "last_component":
        p[:, C - 1] = 0.0
    if mutate == "row63_for_64" and T > 64:
        p[64] = p[63]
    occ, F, _ = ER._accumulate(p, x)
    if mutate == "last_dim":
        F[:, D - 1] = 0.0
    return occ, F


@pytest.mark.parametrize("C,D,T", [(64, 39, 65), (65, 77, 129), (100, 60, 130)])
def test_the_assertions_catch_a_wrong_posterior_kernel(C, D, T):
    gc, miv, iv = ER.params(ER.overlapping_ubm(C, D))
    x = ER.shared(C, D, T)
    ll32 = ER.ll64(gc, miv, iv, x).astype(np.float32)
    occ, F = _device_model(ll32, x, C, D)
    rb, g, _, _ = ER.ratios_b(occ, F, ll32, x)
    rc = ER.ratio_c(occ, F, gc, miv, iv, x, g)
    print("C %d D %d T %d unmutated: (b) %.3f (c) %.3f" % (C, D, T, rb, rc))
    assert rb <= 1.0 and rc <= 1.0
    for m in ("last_component", "row63_for_64", "last_dim", "inv_sum0"):
        occ_m, F_m = _device_model(ll32, x, C, D, m)
        rb_m = ER.ratios_b(occ_m, F_m, ll32, x)[0]
        rc_m = ER.ratio_c(occ_m, F_m, gc, miv, iv, x, g)
        d_occ = np.abs(occ_m - occ).max()
        print("  %-15s moves occ by %.3g: (b) %.3g (c) %.3g" % (m, d_occ, rb_m, rc_m))
        assert rb_m > 1.0 and rc_m > 1.0, m


@pytest.mark.parametrize("C,D,T", [(65, 77, 129), (100, 60, 130)])
def test_first_order_bound_covers_errors_of_the_allowed_size(C, D, T):
    """(c): every ll moved by a uniform random error of up to eps_tk = 2e-6 max(1, S_tk) stays inside the bound"""
    gc, miv, iv = ER.params(ER.overlapping_ubm(C, D))
    x = ER.shared(C, D, T)
    eps = ER.EPS_LL * np.maximum(1.0, ER.S(gc, miv, iv, x))
    rng = np.random.default_rng(17)
    ll = (ER.ll64(gc, miv, iv, x) + eps * rng.uniform(-1.0, 1.0, eps.shape)).astype(np.float32)
    occ, F = _device_model(ll, x, C, D)
    rc = ER.ratio_c(occ, F, gc, miv, iv, x, ER.GAMMA_FLOOR)
    print("C %d D %d T %d: worst error / bound %.3f" % (C, D, T, rc))
    assert 0.02 <= rc <= 1.0                                  # covered, and by no more than a factor of 50


def test_one_hot_rows_leave_components_empty():
    """the component-with-no-mass case of the GPU tests: rows on components 0 .. 31 of the unshrunk UBM leave the others
    1e-4 or less, and pushed out to 8 mu_k they leave exact zeros in the Kaldi-order twin"""
    for C, D in [(100, 60), (65, 77)]:
        ubm, _ = synthetic_gmm_system(1, C, D)
        for out, n_empty in [(1.0, 0), (8.0, 8)]:
            x = ER.one_hot_rows(C, D, 130, out=out)
            ll32 = ER.ll64(ubm.gconsts, ubm.means_invvars, ubm.inv_vars, x).astype(np.float32)
            occ, _, _ = ER.stats_kaldi(ll32, x)
            print("C %d D %d rows at %g mu: %d components exactly empty, largest occ past component 31 %.2g"
                  % (C, D, out, (occ == 0.0).sum(), occ[32:].max()))
            assert (occ == 0.0).sum() >= n_empty and abs(occ.sum() - 130) < 1e-3
            if out == 1.0:
                assert occ[32:].max() < 1e-3


def test_nine_significant_digits_round_trip_a_float32():
    """build_spk_models writes i-vectors as "%.9g" text: reading them back gives the float32 bit for bit"""
    rng = np.random.default_rng(3)
    v = np.concatenate([rng.standard_normal(20000) * np.exp(rng.uniform(-60.0, 60.0, 20000)),
                        [0.0, 1.0, -1.0, np.finfo(np.float32).max, np.finfo(np.float32).tiny, 1e-45,
                         1.0 + 2.0 ** -23, 16777217.0]]).astype(np.float32)
    back = np.array([("%.9g" % x) for x in v], np.float32)
    assert np.array_equal(back.view(np.uint32), v.view(np.uint32))
