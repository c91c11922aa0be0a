"""The loaders' host preparation (fakebob_amd/csrc/fb_prepare.h) through the engine-free hooks, no GPU: invariants of the
delta plan, the image layouts decoded back to the parameters they were packed from, and the refusals."""
import ctypes as C

import numpy as np
import pytest

from fakebob_amd import _native, prepare
from fakebob_amd.models import stack_models, synthetic_gmm_system

KNOBS = ("FB_GMM_MODE", "FB_GMM_DELTA_P", "FB_GMM_DELTA_BUDGET", "FB_GMM_DELTA_F6")
FB_FXW_MAX_M = 10        # csrc/fb_gmm_limits.h
L2E = 1.4426950408889634
_systems = {}


@pytest.fixture(autouse=True)
def _no_knobs(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


def system(M, Cn=64, D=72):
    """(gconsts, means_invvars, inv_vars) of the synthetic UBM + M - 1 speakers; built once, never written"""
    key = (M, Cn, D)
    if key not in _systems:
        ubm, spk = synthetic_gmm_system(n_speakers=M - 1, C=Cn, D=D)
        _systems[key] = stack_models([ubm] + spk)
        for a in _systems[key]:
            a.flags.writeable = False
    return _systems[key]


def unfrag(img, terms, nk):
    """an MFMA fragment image [tiles][items][terms][nk][64 lanes][8] -> [tiles][items][terms][32 components][16 nk K places]
    (lane = 32 * (k % 16 // 8) + component, csrc/fb_prepare.h: fb_gmm_frag_index)"""
    a = img.reshape(-1, terms, nk, 2, 32, 8)
    a = a.transpose(0, 1, 4, 2, 3, 5).reshape(a.shape[0], terms, 32, 16 * nk)
    return a


def two_term_bound(x):
    """|a + b - x| for the two-term f16 split of x: each term carries 11 significant bits, the residual may be subnormal
    (absolute precision 2^-25)"""
    return 2.0 ** -22 * np.abs(x) + 2.0 ** -25


# ------------------------------------------------------------------ the plan
@pytest.mark.parametrize("M", [3, 11, 28])
@pytest.mark.parametrize("forced", [None, "1", "2", "3", "6"])
def test_plan_invariants(M, forced, monkeypatch):
    if forced:
        monkeypatch.setenv("FB_GMM_DELTA_P", forced)
    gc, miv, iv = system(M)
    plan, perm = prepare.gmm_plan(gc, miv, iv)
    Cn = gc.shape[1]
    n_tiles = Cn // 32
    assert plan["mode"] == 2 and plan["NKF"] == 5 and plan["n_tiles"] == n_tiles and plan["n_items"] == M + 1
    assert plan["delta_p"] in (1, 2, 3, 6)
    assert sorted(perm.tolist()) == list(range(Cn))
    assert 0 <= plan["t3"] <= plan["t6"] <= plan["t2"] <= n_tiles
    lo = plan["pass_lo"][:plan["n_pass"] + 1]
    assert plan["n_pass"] == -(-(M - 1) // (FB_FXW_MAX_M - 1))
    assert lo[0] == 1 and lo[-1] == M and all(b > a for a, b in zip(lo, lo[1:]))
    assert max(b - a for a, b in zip(lo, lo[1:])) <= FB_FXW_MAX_M - 1
    if forced:
        counts = {"3": plan["t3"], "6": plan["t6"] - plan["t3"], "2": plan["t2"] - plan["t6"], "1": n_tiles - plan["t2"]}
        assert counts[forced] == n_tiles and plan["delta_p"] == int(forced)
    # every pass's image holds {Q, base, its deltas} per tile; the buffers of passes that do not run are empty
    for p in range(3):
        fd = prepare.gmm_buffer(gc, miv, iv, "fd", p)
        want = n_tiles * (2 + lo[p + 1] - lo[p]) * 2 * 5 * 64 * 8 if p < plan["n_pass"] else 0
        assert fd.size == want


# ------------------------------------------------------------------ bx3
def test_bx3_terms_sum_to_the_parameters_exactly(monkeypatch):
    monkeypatch.setenv("FB_GMM_MODE", "bx3")
    M, Cn, D = 3, 48, 72                                 # 48 components: the second tile is half padding
    gc, miv, iv = system(M, Cn)
    plan, _ = prepare.gmm_plan(gc, miv, iv)
    assert plan["mode"] == 1 and plan["NK"] == 5 and plan["delta_p"] == 0 and plan["n_tiles"] == 2
    assert prepare.gmm_buffer(gc, miv, iv, "fx").size == 0
    items = prepare.gmm_buffer(gc, miv, iv, "item_model")
    assert items.tolist() == [-1, 0, 1, 2]
    bx = prepare.gmm_buffer(gc, miv, iv, "bx")
    terms = (bx.astype(np.uint32) << 16).view(np.float32).astype(np.float64)      # bf16 -> the float32 it stands for
    img = unfrag(terms, 3, 5).reshape(2, M + 1, 3, 32, 80)
    total = img.sum(axis=2).transpose(1, 0, 2, 3).reshape(M + 1, 64, 80)            # [item][component][K]
    assert np.array_equal(total[0, :Cn, :D], (np.float32(-0.5) * iv[0]).astype(np.float64))
    assert np.array_equal(total[1:, :Cn, :D], miv.astype(np.float64))
    assert np.all(total[:, Cn:, :D] == 0.0) and np.all(total[:, :, D + 3:] == 0.0)
    # gconst: its three bf16 terms stand in the FIRST term's K places D .. D + 2
    g3 = img[:, :, 0, :, D:D + 3].sum(axis=-1).transpose(1, 0, 2).reshape(M + 1, 64)
    assert np.array_equal(g3[1:, :Cn], gc.astype(np.float64))
    assert np.all(g3[1:, Cn:] == np.float64(np.float32(-1.0e30)))
    assert np.all(g3[0] == 0.0) and np.all(img[:, :, 1:, :, D:] == 0.0)


# ------------------------------------------------------------------ fx2
def test_fx2_terms_reproduce_the_scaled_parameters():
    M, Cn, D = 3, 64, 72
    gc, miv, iv = system(M)
    plan, _ = prepare.gmm_plan(gc, miv, iv)
    assert plan["mode"] == 2 and prepare.gmm_buffer(gc, miv, iv, "bx").size == 0
    kl, kq = plan["kacc"] - plan["kx"], plan["kacc"] - plan["kx2"]
    fx = prepare.gmm_buffer(gc, miv, iv, "fx").view(np.float16).astype(np.float64)
    img = unfrag(fx, 2, 5).reshape(2, M + 1, 2, 32, 80)
    total = img.sum(axis=2).transpose(1, 0, 2, 3).reshape(M + 1, Cn, 80)
    want_q = -0.5 * 2.0 ** kq * iv[0].astype(np.float64)
    want_l = 2.0 ** kl * miv.astype(np.float64)
    want_g = 2.0 ** kl * gc.astype(np.float64)
    for got, want in ((total[0, :, :D], want_q), (total[1:, :, :D], want_l), (total[1:, :, D], want_g)):
        err = np.abs(got - want)
        print("fx2 worst error / bound: %.3g" % np.max(err / two_term_bound(want)))
        assert np.all(err <= two_term_bound(want))
    assert np.all(total[0, :, D:] == 0.0) and np.all(total[1:, :, D + 1:] == 0.0)


# ------------------------------------------------------------------ delta images
# The three-term constant.  Three f16 terms carry 33 significant bits while all three are normal numbers; the third term of
# these constants is a subnormal f16 (a base constant of ~ -200 leaves a third term below 2^-16, a delta constant of ~1e-3
# already a second one), whose absolute precision is 2^-25: |c1 + c2 + c3 - c| <= 2^-33 |c| + 2^-25, the two-term bound's
# reasoning with one more term.  A purely relative 2^-33 is therefore missed, by the parent commit's bytes as by these
# (they are the same bytes): the worst relative error measured on the parent's bytes for these inputs is
# CONST_REL_MEASURED (M = 3: 2.13808e-05, M = 11: 3.88049e-05 -- delta constants near zero), and the relative bound is
# twice that.
CONST_REL_MEASURED = 3.88049e-05
CONST_REL_BOUND = 2.0 * CONST_REL_MEASURED


@pytest.mark.parametrize("M", [3, 11])
def test_delta_images_reproduce_the_balanced_log2_parameters(M, monkeypatch):
    monkeypatch.setenv("FB_GMM_DELTA_P", "3")
    Cn, D, W = 64, 72, 80
    gc, miv, iv = system(M)
    plan, perm = prepare.gmm_plan(gc, miv, iv)
    assert plan["delta_p"] == 3 and plan["t3"] == 2
    an = prepare.gmm_buffer(gc, miv, iv, "anchor")
    assert an.size == 2 * W + 2 * (2 * W + 4) + 2 * W        # the float table and the anchors' f16 copies (two per float)
    s_kd, s_kq = an[:D].astype(np.float64), an[W:W + D].astype(np.float64)     # 2^kd, 2^kq
    assert np.all(np.log2(s_kd) == np.round(np.log2(s_kd))) and np.array_equal(s_kq, s_kd * s_kd)
    gc64, miv64, iv64 = (a.astype(np.float64) for a in (gc, miv, iv))
    lo = plan["pass_lo"]
    worst_c = 0.0
    for p in range(plan["n_pass"]):
        models = [-1, 0] + list(range(lo[p], lo[p + 1]))
        fd = prepare.gmm_buffer(gc, miv, iv, "fd", p).view(np.float16).astype(np.float64)
        img = unfrag(fd, 2, 5).reshape(2, len(models), 2, 32, W)
        img = img.transpose(1, 2, 0, 3, 4).reshape(len(models), 2, Cn, W)        # [item][term][place][K]
        for it, m in enumerate(models):
            if m < 0:
                want = L2E * (np.float32(-0.5) * iv[0]).astype(np.float64)[perm] / s_kq
            elif m == 0:
                want = L2E * miv64[0][perm] / s_kd
            else:
                want = L2E * (miv[m] - miv[0]).astype(np.float64)[perm] / s_kd   # (the float32 difference)
            err = np.abs(img[it, 0, :, :D] + img[it, 1, :, :D] - want)
            assert np.all(err <= two_term_bound(want)), (p, m, np.max(err / two_term_bound(want)))
            if m < 0:
                assert np.all(img[it, 0, :, D + 3] == 1.0) and np.all(img[it, 0, :, D + 4] == 2048.0)
                continue
            cst = L2E * (gc64[0] if m == 0 else (gc[m] - gc[0]).astype(np.float64))[perm]
            err = np.abs(img[it, 0, :, D:D + 3].sum(axis=-1) - cst)
            assert np.all(err <= 2.0 ** -33 * np.abs(cst) + 2.0 ** -25), (p, m)
            worst_c = max(worst_c, float(np.max(err / np.abs(cst))))
    print("delta constants, worst relative error: %.3g (2^%.2f)" % (worst_c, np.log2(worst_c)))
    assert worst_c <= CONST_REL_BOUND


# ------------------------------------------------------------------ refusals
@pytest.mark.parametrize("name,value,text", [
    ("FB_GMM_DELTA_P", "7", "FB_GMM_DELTA_P must be 1, 2, 3 or 6 (got '7')"),
    ("FB_GMM_DELTA_BUDGET", "1e-3", "FB_GMM_DELTA_BUDGET must be in [1e-7, 1e-4] (got '1e-3')"),
    ("FB_GMM_MODE", "fp8", "FB_GMM_MODE must be fx2 or bx3 (got 'fp8')"),
])
def test_bad_environment_values_are_refused(name, value, text, monkeypatch):
    monkeypatch.setenv(name, value)
    gc, miv, iv = system(3)
    with pytest.raises(_native.NativeError) as ex:
        prepare.gmm_plan(gc, miv, iv)
    assert ex.value.code == _native.FB_E_ARG and text in str(ex.value)


def test_named_buffers_follow_size_then_fill():
    gc, miv, iv = system(3)
    L = _native.lib()
    args = (C.c_int(3), C.c_int(64), C.c_int(72), _native.ptr(gc), _native.ptr(miv), _native.ptr(iv), None, None)
    size = C.c_int64()
    assert L.fb_debug_prepare_gmm(*args, b"item_model", C.c_int(0), None, C.c_int64(0), C.byref(size)) == 0
    assert size.value == 4 * 4
    out = np.zeros(4, np.int32)
    assert L.fb_debug_prepare_gmm(*args, b"item_model", C.c_int(0), _native.ptr(out), C.c_int64(8), None) == _native.FB_E_ARG
    assert L.fb_debug_prepare_gmm(*args, b"item_model", C.c_int(0), _native.ptr(out), C.c_int64(16), None) == 0
    assert out.tolist() == [-1, 0, 1, 2]
    assert L.fb_debug_prepare_gmm(*args, b"nothing", C.c_int(0), None, C.c_int64(0), C.byref(size)) == _native.FB_E_ARG
    assert L.fb_debug_prepare_gmm(*args, b"fd", C.c_int(3), None, C.c_int64(0), C.byref(size)) == _native.FB_E_ARG


def test_ivector_and_frontend_tables_without_an_engine():
    from fakebob_amd.models import synthetic_ivector_system
    sy = synthetic_ivector_system(C=64, D=72, R=40, L=20, n_speakers=2)
    triD = 72 * 73 // 2
    tri = prepare.ivector_buffer(sy, "tri")
    r, c = np.tril_indices(72)
    assert np.array_equal(tri[:triD], r) and np.array_equal(tri[triD:], c)
    assert prepare.ivector_buffer(sy, "fg64").size == 64 * (triD + 72 + 1)
    assert prepare.ivector_buffer(sy, "fgL").size == 64 * (50 * 64 + 72 + 2)
    off = prepare.ivector_buffer(sy, "backend_offsets").tolist()
    assert off == [0, 40, 40 + 40 * 20, 60 + 40 * 20, 60 + 40 * 20 + 400, 80 + 40 * 20 + 400]
    backend = prepare.ivector_buffer(sy, "backend")
    assert backend.size == off[5] + 2 * 20
    assert np.array_equal(backend[off[1]:off[2]].reshape(40, 20), sy.lda.astype(np.float64).T)
    small = synthetic_ivector_system(C=64, D=60, R=40, L=20, n_speakers=2)
    assert prepare.ivector_buffer(small, "fgL").size == 0           # the Cholesky image is D = 72's
    # the diagonalised UBM is a valid single-model GMM for the GMM path
    dg = [prepare.ivector_buffer(sy, n) for n in ("dg_gc", "dg_miv", "dg_iv")]
    plan, _ = prepare.gmm_plan(dg[0].reshape(1, 64), dg[1].reshape(1, 64, 72), dg[2].reshape(1, 64, 72))
    assert plan["mode"] == 2 and plan["n_items"] == 2 and plan["delta_p"] == 0
    # front end: the stock tables, and a shape k_mfcc_f32 has no table for
    off = prepare.frontend_buffer("offsets").tolist()
    blob = prepare.frontend_buffer("blob")
    assert off[0] == 0 and all(o % 64 == 0 for o in off) and off == sorted(off) and blob.size % 64 == 0
    window = blob[off[0]:off[0] + 8 * 400].view(np.float64)
    assert window[0] == 0.0 and window[399] == 0.0 and abs(window[200] - 1.0) < 1e-4
    assert prepare.frontend_buffer("f32").size > 0
    assert prepare.frontend_buffer("f32", padded_length=256, frame_length=200, frame_shift=80, num_mel_bins=40).size == 0
    with pytest.raises(_native.NativeError) as ex:
        prepare.frontend_buffer("blob", low_freq=9000.0)
    assert ex.value.code == _native.FB_E_ARG and "bad mel frequency range" in str(ex.value)
