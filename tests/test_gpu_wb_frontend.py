"""White-box gradients through feature compression and dither on the device (fb_set_wb_frontend; "Feature compression and
dither" in include/fakebob_hip.h) against tests/feco_vjp_ref.py, which tests/test_feco_vjp_host.py pins to tests/feco_ref.py, to
the adjoint identity and to central differences.

Exact: the kept labels and counts and k_wb_feco_t's division (the hook), ratio 1.0 against the undefended call, the forward
(fb_get_grad's bit for bit), determinism between engines, the launches with the switch on and neither stage set, a whole attack
against its host replay.  One comparison carries a relative L2 bar, ||g - g_ref|| / ||g_ref||:
  fb_get_grad_wb_iter through FeCo / dither against the restatement's loss gradient
      GMM-UBM   measured worst MEASURED_GMM, bar BAR_GMM
      i-vector  measured worst MEASURED_IV,  bar BAR_IV
Each bar is four times the worst error measured over the listed cases on the first run on an MI355X, rounded up to one digit;
none may exceed 1e-2.  The undefended figures they sit near: 2.5e-5 (GMM), 4e-6 (i-vector).
Preconditions, asserted as conditions: the VAD margin of every replica is > 1e-3; without dither, the labels the device kept
equal tests/feco_ref.feco's on fb_debug_feats' float32 rows."""
import os
import pickle

import numpy as np
import pytest

from fakebob_amd import _native as N
from fakebob_amd import input_transform as IT
from fakebob_amd.engine import Engine, nes_params
from fakebob_amd.models import synthetic_ivector_system
from tests import feco_vjp_ref as F
from tests import whitebox_iv_ref as V
from tests import whitebox_ref as R
from tests.feco_ref import feco, feco_k
from tests.test_gpu_whitebox import _load, quantize, rel_l2

pytestmark = pytest.mark.gpu

MEASURED_GMM, BAR_GMM = 3.31e-5, 2e-4       # worst: dither 1.0 on the mfcc_f32 route, epoch 5; FeCo cases 9.1e-6 .. 2.7e-5 (0.2, epoch 0)
MEASURED_IV, BAR_IV = 1.87e-6, 8e-6         # worst: dither 1.0; FeCo 0.5: 1.33e-6

D = 72
SEED, STREAM = 77, 3
ROOM = "t60:100-200,drr:6,taps:256,delay:8"
FECO_REFUSAL = "white-box gradients: feature compression is on (fb_set_feature_compression: switch it off)"
DITHER_REFUSAL = "white-box gradients: dither 1 > 0 (the function is differentiated at a fixed victim)"
OSI_KW = dict(target=1, threshold=-10.0)
FC_LDS_MAX = 160 * 1024 - 2 * 4 * 1024 - 256     # feature_compress_kernel.hip: what the fast path may ask for


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


def _clear(e):
    e.set_feature_compression(None)
    e.set_frontend(dither=0.0, mfcc_f32=0)
    e.set_air_channel(None)
    e.set_input_transform(None)
    e.set_codec(None)
    e.set_companions(None)
    e.set_eot(1)
    e.set_wb_bpda(False)
    e.set_wb_ivector(False)
    e.set_wb_air(False)
    e.set_wb_frontend(False)


def _p(task, attack, kw, **more):
    return nes_params(task, attack, samples_per_draw=0, seed=SEED, stream=STREAM, **dict(kw, **more))


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


# ------------------------------------------------------------------------------------- 1. the hook, exactly
LENGTHS = [1, 2, 3, 63, 0, 64, 65, 257, 300, 700]          # tests/test_gpu_feco.py's batch: 700 takes the general path
HSEED, HSTREAM, HEPOCH = 0xC0FFEE1234567, 5, 9


@pytest.fixture(scope="module")
def mats():
    rng = np.random.RandomState(11)
    return [(3.0 * rng.standard_normal((T, D))).astype(np.float32) for T in LENGTHS]


def _hook_case(e, philox_keys, ms, r, ratio, iters):
    rng = np.random.default_rng(int(ratio * 1000) + iters + r)
    cots = [[rng.normal(size=(feco_k(m.shape[0], ratio), D)) for _ in range(r)] for m in ms]
    e.set_feature_compression(ratio, iters)
    try:
        labels, counts, xbar = e.debug_feature_compress_vjp(ms, r, HSEED, HSTREAM, HEPOCH, cots)
        assert e.debug_wb_feco_route() == 1
        plain = e.debug_feature_compress(ms, r, HSEED, HSTREAM, HEPOCH)
    finally:
        e.set_feature_compression(None)
    empties = 0
    for b, m in enumerate(ms):
        for j in range(r):
            T, k = m.shape[0], feco_k(m.shape[0], ratio)
            C, want = feco(m, philox_keys(b, j, T), ratio, iters)
            lab, cnt, xb = labels[b][j], counts[b][j], xbar[b][j]
            assert lab.shape == (T,) and cnt.shape == (k,) and xb.shape == (T, D), (b, j)
            assert np.array_equal(plain[b][j].view(np.uint32), C.view(np.uint32)), (b, j)      # the forward with keep on is the forward
            if T == 0:
                continue
            assert np.array_equal(lab, want), (b, j, "labels")
            assert np.array_equal(cnt, np.bincount(want, minlength=k)), (b, j, "counts")
            ref = cots[b][j][lab] / cnt[lab].astype(np.float64)[:, None]
            assert np.array_equal(_bits(xb), _bits(ref)), (b, j, "xbar")
            empties += int((cnt == 0).sum())
    return labels, counts, xbar, cots, empties


@pytest.fixture(scope="module")
def hook_keys(eng):
    def keys(b, j, T):
        return eng.debug_feco_keys(HSEED, HSTREAM, HEPOCH, b, j, T) if T > 0 else np.zeros(0, np.uint32)
    return keys


@pytest.mark.parametrize("iters", [1, 10])
@pytest.mark.parametrize("ratio", [0.001, 0.2, 0.5, 1.0])
def test_hook_labels_counts_and_division(eng, mats, hook_keys, ratio, iters):
    labels, counts, _xbar, _cots, _e = _hook_case(eng, hook_keys, mats, 1, ratio, iters)
    if ratio == 0.001:
        assert all(c[0].tolist() == [m.shape[0]] for c, m in zip(counts, mats) if m.shape[0])      # k = 1, n = T
    if ratio == 1.0:
        assert all(np.array_equal(l[0], np.arange(m.shape[0])) for l, m in zip(labels, mats))


@pytest.mark.parametrize("ratio", [0.2, 0.5])
def test_hook_with_three_replicas(eng, mats, hook_keys, ratio):
    sub = [mats[i] for i in (3, 4, 6, 8, 9)]                                # 63, 0, 65, 300, 700
    labels, _c, _x, _cots, _e = _hook_case(eng, hook_keys, sub, 3, ratio, 10)
    assert not np.array_equal(labels[3][0], labels[3][1])                   # a draw per replica


@pytest.mark.parametrize("ratio", [0.25, 1.0])
def test_hook_on_repeated_rows_drops_an_empty_centres_cotangent(eng, hook_keys, ratio):
    rng = np.random.RandomState(12)
    base = (3.0 * rng.standard_normal((9, D))).astype(np.float32)
    X = base[rng.randint(0, 9, 130)]
    Y = np.concatenate([X[:40], (3.0 * rng.standard_normal((40, D))).astype(np.float32)])
    labels, counts, xbar, cots, empties = _hook_case(eng, hook_keys, [X, Y], 2, ratio, 10)
    assert empties > 0                                                      # the case does hold an empty cluster
    loud = [[np.where((counts[b][j] == 0)[:, None], 1e300, cots[b][j]) for j in range(2)] for b in range(2)]
    eng.set_feature_compression(ratio, 10)
    try:
        _l, _c, xbar2 = eng.debug_feature_compress_vjp([X, Y], 2, HSEED, HSTREAM, HEPOCH, loud)
    finally:
        eng.set_feature_compression(None)
    for b in range(2):
        for j in range(2):
            assert np.array_equal(_bits(xbar2[b][j]), _bits(xbar[b][j])) and np.abs(xbar2[b][j]).max() < 1e10


# ------------------------------------------------------------------------------------- 2. ratio 1.0 is the undefended gradient
IV_SMALL = dict(C=64, D=72, R=32, L=16, n_speakers=2, seed=4)


@pytest.mark.parametrize("victim", ["gmm_osi_targeted", "gmm_csi_untargeted", "ivector"])
def test_ratio_one_is_the_undefended_gradient(eng, small_system, victim):
    audio = R.test_audio(4000)
    if victim == "ivector":
        eng.load_ivector(synthetic_ivector_system(**IV_SMALL), "OSI")
        p = _p("OSI", "targeted", OSI_KW)
    elif victim == "gmm_osi_targeted":
        _load(eng, small_system, "OSI")
        p = _p("OSI", "targeted", OSI_KW)
    else:
        _load(eng, small_system, "CSI")
        p = _p("CSI", "untargeted", dict(true=0))
    try:
        eng.set_wb_ivector(victim == "ivector")
        want = eng.get_grad_wb_iter(p, audio, 3)
        want_route = eng.debug_wb_route()
        eng.set_wb_frontend(True)
        eng.set_feature_compression(1.0, 10)
        got = eng.get_grad_wb_iter(p, audio, 3)
        route, launches = eng.debug_wb_route(), eng.debug_wb_feco_route()
        labels, counts = eng.debug_wb_feco_state(0)
    finally:
        _clear(eng)
        _load(eng, small_system, "OSI")
    assert np.array_equal(labels, np.arange(labels.size)) and (counts == 1).all() and counts.size == labels.size
    assert np.array_equal(_bits(got[0]), _bits(want[0])) and got[1] == want[1] and np.array_equal(got[2], want[2])
    assert route == want_route and launches == 1
    assert got[0].any()


# ------------------------------------------------------------------------------------- 3. the full gradient
def _chain(spec):
    return [tuple(s) for s in IT.parse(spec)] if spec else []


def _setup(e, ratio=None, iters=10, dither=0.0, f32=False, r=1, spec=None, air=False, bpda=None):
    e.set_feature_compression(ratio, iters) if ratio else e.set_feature_compression(None)
    e.set_frontend(dither=float(dither), mfcc_f32=1 if f32 else 0)
    e.set_input_transform(spec)
    e.set_air_channel(ROOM if air else None)
    e.set_eot(r)
    e.set_wb_bpda(bool(r > 1 or spec) if bpda is None else bpda)
    e.set_wb_air(bool(air))
    e.set_wb_frontend(True)


def _kept(e, r):
    return [e.debug_wb_feco_state(j) for j in range(r)]


def _dither_normals(e, n, it, r):
    T = e._num_frames(n)
    return [e.debug_dither_noise(SEED, STREAM, it, j, 0, T) for j in range(r)]


def _check_labels_against_feco_ref(e, row, it, j, ratio, iters, kept):
    """the precondition without dither: the device's labels are feco_ref's on fb_debug_feats' float32 rows of the row the front
    end read"""
    rows, _T = e.debug_feats(row)
    C, want = feco(rows, e.debug_feco_keys(SEED, STREAM, it, 0, j, rows.shape[0]), ratio, iters)
    assert np.array_equal(kept[0], want), "replica %d: the kept labels are not feco_ref's" % j
    assert np.array_equal(kept[1], np.bincount(want, minlength=C.shape[0]))
    return C


#            name                   n      ratio dither f32    r  spec      air   it
GMM_CASES = [("feco0.5_it0",        4000,  0.5,  0.0,   False, 1, None,     False, 0),
             ("feco0.5_it5",        4000,  0.5,  0.0,   False, 1, None,     False, 5),
             ("feco0.2_it0",        4000,  0.2,  0.0,   False, 1, None,     False, 0),
             ("feco0.2_it5",        4000,  0.2,  0.0,   False, 1, None,     False, 5),
             ("feco0.5_n64000",     64000, 0.5,  0.0,   False, 1, None,     False, 0),
             ("feco0.5_n96000",     96000, 0.5,  0.0,   False, 1, None,     False, 0),     # more voiced rows than the LDS holds
             ("dither_f64_it0",     4000,  None, 1.0,   False, 1, None,     False, 0),
             ("dither_f64_it5",     4000,  None, 1.0,   False, 1, None,     False, 5),
             ("dither_f32_it0",     4000,  None, 1.0,   True,  1, None,     False, 0),
             ("dither_f32_it5",     4000,  None, 1.0,   True,  1, None,     False, 5),
             ("feco_dither",        4000,  0.5,  1.0,   False, 1, None,     False, 5),
             ("feco_dither_r3",     4000,  0.5,  1.0,   False, 3, None,     False, 5),
             ("feco_qt512",         4000,  0.5,  0.0,   False, 1, "qt:512", False, 5),
             ("feco_air",           4000,  0.5,  0.0,   False, 1, None,     True,  5)]


@pytest.mark.parametrize("name,n,ratio,dither,f32,r,spec,air,it", GMM_CASES, ids=[c[0] for c in GMM_CASES])
def test_get_grad_wb_against_the_restatement(eng, small_system, name, n, ratio, dither, f32, r, spec, air, it):
    audio = R.test_audio(n)
    models = _load(eng, small_system, "OSI")
    p = _p("OSI", "targeted", OSI_KW)
    chain = _chain(spec)
    try:
        _setup(eng, ratio, 10, dither, f32, r, spec, air)
        grad, al, sc = eng.get_grad_wb_iter(p, audio, it)
        kept = _kept(eng, r) if ratio else [None] * r
        launches, route = eng.debug_wb_feco_route(), eng.debug_wb_route()
        _fl, _gg, al0, sc0 = eng.get_grad(p, audio, it=it, want_grad=False)
        z = _dither_normals(eng, n, it, r) if dither else [None] * r
        taps = [eng.debug_air_taps(SEED, STREAM, it, 0, j)[0] for j in range(r)] if air else None
        empty = [None] * r
        if ratio and not dither and not air:
            row = eng.debug_input_transform([quantize(audio)])[0] if spec else quantize(audio)
            empty = [_check_labels_against_feco_ref(eng, row, it, j, ratio, 10, kept[j]) for j in range(r)]
    finally:
        _clear(eng)
    fc = [None if not ratio else dict(labels=kept[j][0], k=kept[j][1].size, empty=empty[j]) for j in range(r)]
    ref = F.loss_and_grad(eng.cfg, models, "OSI", "targeted", audio, feco=fc, dither=z, amp=dither, chain=chain, taps=taps, **OSI_KW)
    err = rel_l2(grad, ref.grad)
    tv = [f.shape[0] for f in ref.feats]
    print("%s: Tv %s, k %s, loss %.9g (restatement %.9g), min |c0 - thr| %.3g, relative L2 error %.3g"
          % (name, tv, [None if k is None else k[1].size for k in kept], al, ref.loss, ref.margin, err))
    assert al == al0 and np.array_equal(sc, sc0)                # the forward is fb_get_grad's, bit for bit
    assert launches == (r if ratio else 0)
    assert route == dict(ctl=1 if r == 1 else 0, ctl_rep=r if r > 1 else 0, backward=r, chain_t=r if (chain or (r > 1 and not air)) else 0)
    if ratio:
        for j in range(r):
            assert kept[j][0].size == tv[j] and kept[j][1].size == feco_k(tv[j], ratio) and kept[j][1].sum() == tv[j]
    if name == "feco0.5_n96000":                                # fc_lds_bytes(T, k, D) of the kernel: the general path
        assert 4 * (feco_k(tv[0], ratio) * 72 + tv[0] * 73 + 5 * tv[0]) > FC_LDS_MAX
    assert ref.margin > 1e-3
    assert abs(al - ref.loss) < 1e-3 and np.abs(sc - ref.scores).max() < 1e-3
    assert np.isfinite(grad).all() and grad.any()
    assert err < BAR_GMM


@pytest.mark.parametrize("stage", ["feco", "dither"])
def test_get_grad_wb_on_the_small_ivector_system(eng, small_system, stage):
    from tests.test_gpu_whitebox_iv import VAD_MARGIN, _assert_margins
    sy = synthetic_ivector_system(**IV_SMALL)
    tab = V.IvTables(sy)
    eng.load_ivector(sy, "OSI")
    audio, it = R.test_audio(4000), 5
    p = _p("OSI", "targeted", OSI_KW)
    ratio, dither = (0.5, 0.0) if stage == "feco" else (None, 1.0)
    try:
        _setup(eng, ratio, 10, dither)
        eng.set_wb_ivector(True)
        grad, al, sc = eng.get_grad_wb_iter(p, audio, it)
        kept = eng.debug_wb_feco_state(0) if ratio else None
        sel, _info = eng.debug_iv_gselect()
        launches, route = eng.debug_wb_feco_route(), eng.debug_wb_route()
        _fl, _gg, al0, sc0 = eng.get_grad(p, audio, it=it, want_grad=False)
        z = _dither_normals(eng, 4000, it, 1)[0] if dither else None
        empty = _check_labels_against_feco_ref(eng, quantize(audio), it, 0, ratio, 10, kept) if ratio else None
    finally:
        _clear(eng)
        _load(eng, small_system, "OSI")
    fc = None if not ratio else dict(labels=kept[0], k=kept[1].size, empty=empty)
    r = F.loss_and_grad_iv(eng.cfg, tab, "OSI", "targeted", audio, feco=fc, dither=z, amp=dither, sel=sel, **OSI_KW)
    _assert_margins(r, sel, "i-vector " + stage)
    err = rel_l2(grad, r.grad)
    print("i-vector %s: Tv %d, rows scored %d, loss %.9g (restatement %.9g), relative L2 error %.3g" % (stage, r.tv, sel.shape[0], al, r.loss, err))
    assert al == al0 and np.array_equal(sc, sc0)
    assert launches == (1 if ratio else 0) and route["iv_post_t"] == 1 and route["backward"] == 1
    assert sel.shape[0] == (feco_k(r.tv, ratio) if ratio else r.tv)
    assert r.margin > VAD_MARGIN and abs(al - r.loss) < 1e-3
    assert np.isfinite(grad).all() and grad.any()
    assert err < BAR_IV


# ------------------------------------------------------------------------------------- 4. forward parity
PARITY = [("feco", 0.5, 0.0, 1), ("dither", None, 1.0, 1), ("both", 0.5, 1.0, 1), ("both_r3", 0.5, 1.0, 3)]


@pytest.mark.parametrize("name,ratio,dither,r", PARITY, ids=[c[0] for c in PARITY])
def test_forward_is_get_grads(eng, small_system, name, ratio, dither, r):
    audio = R.test_audio(4000)
    _load(eng, small_system, "OSI")
    p = _p("OSI", "targeted", OSI_KW)
    try:
        _setup(eng, ratio, 10, dither, r=r)
        for it in (0, 7):
            _g, al, sc = eng.get_grad_wb_iter(p, audio, it)
            _fl, _gg, al0, sc0 = eng.get_grad(p, audio, it=it, want_grad=False)
            assert al == al0 and np.array_equal(_bits(sc), _bits(sc0)), (name, it)
        plain = eng.get_grad(p, audio, it=0, want_grad=False)[2]
        _clear(eng)
        assert plain != eng.get_grad(p, audio, it=0, want_grad=False)[2]       # and the stage did something
    finally:
        _clear(eng)


# ------------------------------------------------------------------------------------- 5. draws
@pytest.mark.parametrize("stage", ["feco", "dither"])
def test_the_draws_differ_between_epochs(eng, small_system, stage):
    audio = R.test_audio(4000)
    _load(eng, small_system, "OSI")
    p = _p("OSI", "targeted", OSI_KW)
    try:
        _setup(eng, 0.5 if stage == "feco" else None, 10, 1.0 if stage == "dither" else 0.0)
        g0, al0, _ = eng.get_grad_wb(p, audio)
        g0b, al0b, _ = eng.get_grad_wb_iter(p, audio, 0)
        g5, al5, _ = eng.get_grad_wb_iter(p, audio, 5)
    finally:
        _clear(eng)
    assert np.array_equal(_bits(g0), _bits(g0b)) and al0 == al0b                # fb_get_grad_wb is iter = 0
    assert al0 != al5 and not np.array_equal(g0, g5)


def test_two_fresh_engines_give_equal_bits(small_system):
    audio = R.test_audio(4000)
    p = _p("OSI", "targeted", OSI_KW)
    got = []
    for _ in range(2):
        e = Engine(0)
        try:
            _load(e, small_system, "OSI")
            _setup(e, 0.5, 10, 1.0, r=3)
            got.append(e.get_grad_wb_iter(p, audio, 2))
        finally:
            e.close()
    a, b = got
    assert np.array_equal(_bits(a[0]), _bits(b[0])) and a[1] == b[1] and np.array_equal(a[2], b[2])


# ------------------------------------------------------------------------------------- 6. the switch
WB_P = nes_params("OSI", "targeted", target=1, threshold=0.0, max_iter=3)
NES_P = nes_params("OSI", "targeted", target=1, threshold=0.0, max_iter=3, samples_per_draw=6, seed=9)


def _refused(e, audio, p=WB_P):
    for call in (lambda: e.get_grad_wb(p, audio), lambda: e.get_grad_wb_iter(p, audio, 1), lambda: e.attack_wb(p, audio)):
        with pytest.raises(N.NativeError) as ex:
            call()
        assert ex.value.code == N.FB_E_STATE, str(ex.value)
    return str(ex.value)


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


def test_the_switch_takes_0_or_1(eng):
    assert eng.wb_frontend is False
    eng.set_wb_frontend(True)
    try:
        for bad in (2, -1):
            with pytest.raises(N.NativeError) as ex:
                eng.set_wb_frontend(bad)
            assert ex.value.code == N.FB_E_ARG and eng.wb_frontend is True     # the setting stays
    finally:
        eng.set_wb_frontend(False)


@pytest.mark.parametrize("others", range(8), ids=lambda m: "bpda%d_ivector%d_air%d" % (m & 1, (m >> 1) & 1, (m >> 2) & 1))
def test_switch_off_refuses_as_before(eng, small_system, nes_baseline, others):
    audio = R.test_audio(4000)
    if others & 2:
        eng.load_ivector(synthetic_ivector_system(**IV_SMALL), "OSI")
    else:
        _load(eng, small_system, "OSI")
    try:
        for stage, words in (("feco", FECO_REFUSAL), ("dither", DITHER_REFUSAL)):
            eng.set_wb_bpda(bool(others & 1))
            eng.set_wb_ivector(bool(others & 2))
            eng.set_wb_air(bool(others & 4))
            if stage == "feco":
                eng.set_feature_compression(0.5, 2)
            else:
                eng.set_frontend(dither=1.0)
            msg = _refused(eng, audio)
            assert words in msg, msg
            _clear(eng)
    finally:
        _clear(eng)
        _load(eng, small_system, "OSI")
    _same_attack(eng, nes_baseline)                     # after the refusals an NES attack reproduces its baseline ...
    eng.set_wb_frontend(True)
    try:
        _same_attack(eng, nes_baseline)                 # ... and with the switch on as well: it is the white-box calls' alone
    finally:
        _clear(eng)


def test_on_with_neither_stage_queues_the_same_launches(eng, small_system):
    audio = R.test_audio(4000)
    _load(eng, small_system, "OSI")
    p = nes_params("OSI", "targeted", target=1, threshold=0.0, max_iter=4)
    off = eng.get_grad_wb(p, audio)
    off_route, off_nes = eng.debug_wb_route(), eng.debug_nes_route()
    off_attack = eng.attack_wb(p, audio)
    off_attack_route = eng.debug_wb_route()
    try:
        eng.set_wb_frontend(True)
        on = eng.get_grad_wb(p, audio)
        on_route, on_nes, on_feco = eng.debug_wb_route(), eng.debug_nes_route(), eng.debug_wb_feco_route()
        on_attack = eng.attack_wb(p, audio)
        on_attack_route, on_attack_feco = eng.debug_wb_route(), eng.debug_wb_feco_route()
    finally:
        _clear(eng)
    assert np.array_equal(_bits(off[0]), _bits(on[0])) and off[1] == on[1] and np.array_equal(off[2], on[2])
    assert off_route == on_route == dict(ctl=1, ctl_rep=0, backward=1, chain_t=0) and off_nes == on_nes
    assert on_feco == 0 and on_attack_feco == 0 and off_attack_route == on_attack_route
    for x, y in zip(off_attack, on_attack):
        assert np.array_equal(x, y)


ON_CASES = {
    "companions": (lambda e: e.set_companions([R.test_audio(4000)]), "companions"),
    "eot_without_bpda": (lambda e: e.set_eot(2), "fb_set_eot"),
    "chain_without_bpda": (lambda e: e.set_input_transform("qt:64"), "input-transform"),
    "codec_without_bpda": (lambda e: e.set_codec("ulaw"), "codec"),
    "air_without_wb_air": (lambda e: e.set_air_channel(ROOM), "air channel"),
}


@pytest.mark.parametrize("case", sorted(ON_CASES))
def test_still_refused_with_the_switch_on(eng, small_system, nes_baseline, case):
    on, word = ON_CASES[case]
    _load(eng, small_system, "OSI")
    try:
        eng.set_wb_frontend(True)
        eng.set_feature_compression(0.5, 10)
        eng.set_frontend(dither=1.0)
        eng.set_wb_bpda(case == "companions" or case.startswith("air"))
        on(eng)
        assert word in _refused(eng, R.test_audio(4000))
    finally:
        _clear(eng)
    _same_attack(eng, nes_baseline)


def test_an_ivector_system_needs_its_switch_and_stays_at_r1(eng, small_system, nes_baseline):
    eng.load_ivector(synthetic_ivector_system(**IV_SMALL), "OSI")
    try:
        eng.set_wb_frontend(True)
        eng.set_feature_compression(0.5, 10)
        assert "i-vector" in _refused(eng, R.test_audio(4000))                  # without fb_set_wb_ivector
        eng.set_wb_ivector(True)
        eng.set_wb_bpda(True)
        eng.set_eot(2)
        msg = _refused(eng, R.test_audio(4000))
        assert "i-vector" in msg and "fb_set_eot" in msg
    finally:
        _clear(eng)
        _load(eng, small_system, "OSI")
    _same_attack(eng, nes_baseline)


# ------------------------------------------------------------------------------------- 7. a whole attack is its replay
def replay(e, p, audio):
    """FakeBob.attack (FAKEBOB.py:157-220) on the host in numpy float64, the gradient from fb_get_grad_wb_iter at every iterate
    with the loop index as the epoch of the draws (tests/test_gpu_air_vjp.py's replay, restated)"""
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
    # (adver_thresh keeps the mean loss above zero, so that all four iterations run)
    p = nes_params("OSI", "targeted", target=1, threshold=0.0, adver_thresh=50.0, max_iter=4, plateau_length=2, seed=SEED, stream=STREAM)
    monkeypatch.setenv("FB_ATTACK_BATCH", batch)
    try:
        _setup(eng, 0.5, 10, 1.0, r=2)
        adv, flag, adv_f, trace = eng.attack_wb(p, audio)
        launches, route = eng.debug_wb_feco_route(), eng.debug_wb_route()
        r_adv, r_flag, r_adv_f, r_trace = replay(eng, p, audio)
    finally:
        _clear(eng)
    print("batch %s: %d rows, flag %d, loss %s, lr %s" % (batch, trace.shape[0], flag, trace[:, 1], trace[:, 2]))
    assert launches == 8 and route == dict(ctl=0, ctl_rep=8, backward=8, chain_t=8)
    assert trace.shape == r_trace.shape == (4, 6) and np.array_equal(_bits(trace), _bits(r_trace))
    assert flag == r_flag and np.array_equal(_bits(adv_f), _bits(r_adv_f)) and np.array_equal(adv, r_adv)
    assert len(set(trace[:, 1])) == 4


# ------------------------------------------------------------------------------------- 8. what it is for
def test_the_adaptive_attack_against_feature_compression(eng, small_system):
    """Thirty AdaptivePGD steps at eot_size = 8 against FeCo 0.5:10 (epochs 0 .. 29 of the k-means draws) with the new gradient,
    and the same thirty steps on the undefended gradient; both results scored through the defended victim as the mean loss over
    16 held-out epochs (100 .. 115).  Both runs are deterministic; the three numbers are in DESIGN.md section 6 and the README."""
    from fakebob_amd.pgd import AdaptivePGD
    _load(eng, small_system, "SV")
    audio = R.test_audio(4000)
    model = type("M", (), dict(task="SV", engine=eng))()
    score = nes_params("SV", "untargeted", threshold=1e3, samples_per_draw=0, seed=SEED, stream=STREAM)
    hp = dict(max_iter=30, seed=SEED, verbose=False)          # (threshold=1e3: never stops early)

    def held_out(a):
        return float(np.mean([eng.get_grad(score, a, it=it, want_grad=False)[2] for it in range(100, 116)]))
    try:
        transferred_adv, _flag = AdaptivePGD("SV", "untargeted", model, bpda=False, **hp).attack(audio, None, threshold=1e3)
        eng.set_feature_compression(0.5, 10)
        adaptive_adv, _flag = AdaptivePGD("SV", "untargeted", model, bpda=True, eot_size=8, frontend=True, **hp).attack(audio, None, threshold=1e3)
        launches = eng.debug_wb_feco_route()
        eng.set_eot(1)
        clean = held_out(audio)
        transferred = held_out(transferred_adv[:, 0].astype(np.float64) / 32768.0)
        adaptive = held_out(adaptive_adv[:, 0].astype(np.float64) / 32768.0)
    finally:
        _clear(eng)
        _load(eng, small_system, "OSI")
    print("FeCo 0.5:10, mean adver_loss over 16 held-out epochs: clean %.9g, transferred %.9g, adaptive %.9g" % (clean, transferred, adaptive))
    assert launches == 30 * 8
    assert np.isfinite([clean, transferred, adaptive]).all()
    assert adaptive < transferred < clean      # (the first measured run: 1000.04902 / 998.665148 / 997.508256)


# ------------------------------------------------------------------------------------- 9. AdaptivePGD and the driver
def test_adaptive_pgd_frontend_returns_fakebobs_pair_and_checkpoint(small_system, tmp_path):
    from fakebob_amd.pgd import AdaptivePGD
    from fakebob_amd.systems import gmm_SV
    ubm, spk = small_system
    model = gmm_SV(str(tmp_path / "sv"), ["spk0", "utt0", spk[0], 0.0, 1.0], ubm, pre_model_dir=str(tmp_path), threshold=0.0,
                   feature_compression="0.5:10", dither=1.0)
    audio = R.test_audio(4000)
    pgd = AdaptivePGD("SV", "targeted", model, bpda=True, eot_size=2, frontend=True, max_iter=5, seed=11, verbose=False)
    assert model.engine.eot == 2 and model.engine.wb_bpda and model.engine.wb_frontend and pgd.frontend
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
    assert model.engine.debug_wb_feco_route() == 10
    # frontend=True alone: no other switch at r = 1
    model1 = gmm_SV(str(tmp_path / "sv1"), ["spk0", "utt0", spk[0], 0.0, 1.0], ubm, pre_model_dir=str(tmp_path), threshold=0.0,
                    feature_compression="0.5:10", dither=1.0)
    pgd1 = AdaptivePGD("SV", "targeted", model1, bpda=False, frontend=True, max_iter=3, seed=11, verbose=False)
    assert not model1.engine.wb_bpda and model1.engine.wb_frontend
    adv1, flag1 = pgd1.attack(audio, None, threshold=1e3)
    assert adv1.shape == (4000, 1) and flag1 == -1 and model1.engine.debug_wb_feco_route() == 3


def test_attack_main_pgd_wb_frontend_on_the_synthetic_site(tmp_path, capsys):
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
    argv = ["-spk_id"] + ids + ["-archi", "gmm", "-task", "OSI", "-type", "targeted", "-thresh", str(thr), "-max_iter", "4", "--attack",
                                "pgd", "--wb-frontend", "--feco", "0.5:10", "--dither", "1", "--bpda", "--eot-size", "2", "--streams", "1",
                                "--seed", "7"] + site
    np.random.seed(3)
    g, results, _thr = AM.main(argv)
    out = capsys.readouterr().out
    # (which illegal voices the defended, randomised victim rejects -- hence the attack list -- is its own: at most the site's 12)
    assert "load data done, total num: %d" % g[1] in out and "attack successful rate" in out
    assert 1 <= g[1] <= 12 and len(results) == g[1]
    n = 0
    for root, _dirs, files in os.walk(str(tmp_path / "out" / "checkpoint" / "gmm-OSI-targeted")):
        for f in files:
            with open(os.path.join(root, f), "rb") as r:
                rows = pickle.load(r)
            assert 1 <= len(rows) <= 4 and len(rows[0]) == 4
            n += 1
    assert n == g[1]
    with pytest.raises(SystemExit):
        AM.main([a for a in argv if a != "--wb-frontend"])       # without the flag --feco and --dither stay refused
    with pytest.raises(SystemExit):
        AM.main(argv + ["--companions", "1"])
    with pytest.raises(SystemExit):
        AM.main([("nes" if a == "pgd" else a) for a in argv])     # the flag belongs to --attack pgd
    capsys.readouterr()
