"""White-box gradients of a universal perturbation on the device (fb_set_wb_universal; "Universal perturbations" in
include/fakebob_hip.h) against tests/universal_vjp_ref.py, which tests/test_universal_vjp_host.py pins to
tests/companions_ref.py, to the adjoint identity, to central differences and to tests/whitebox_ref.py at K = 1.

Exact: k_wb_compose_t on integer-valued cotangents (the hook), the forward (fb_get_grad's bit for bit), K = 1 with the switch on,
original = None, a companion equal to the original, determinism between engines, the launch counts, a whole attack against its
host replay, the refusals.  One comparison carries a relative L2 bar, ||g - g_ref|| / ||g_ref||:
  fb_get_grad_wb_from at original != audio against the restatement's loss gradient
      GMM-UBM   measured worst MEASURED_GMM, bar BAR_GMM
      i-vector  measured worst MEASURED_IV,  bar BAR_IV
Each bar is four times the worst error measured over the listed cases on the first run on an MI355X, rounded up to one digit;
none may exceed 1e-2.  The single-row figures they sit near: 2.5e-5 (GMM), 4e-6 (i-vector).
Preconditions, asserted as conditions: the VAD margin of every replica is > 1e-3; at least 1 % of the loud companion's samples
clip; for an i-vector system tests/test_gpu_whitebox_iv.py's selection margins, replica by replica; the labels the device kept
under feature compression equal tests/feco_ref.feco's on the composed row."""
import os
import pickle

import numpy as np
import pytest

from fakebob_amd import _native as N
from fakebob_amd import input_transform as IT
from fakebob_amd.engine import Engine, kv_params, nes_params, pso_params
from fakebob_amd.models import synthetic_ivector_system
from tests import bpda_ref as B
from tests import universal_vjp_ref as U
from tests import whitebox_iv_ref as V
from tests import whitebox_ref as R
from tests.companions_ref import compose_row
from tests.test_gpu_whitebox import _load, quantize, rel_l2
from tests.test_universal_vjp_host import ATTACK_EPS, ATTACK_K1, ATTACK_LR, ATTACK_N, ATTACK_STEPS, ATTACK_THRESHOLD, _rail_case

pytestmark = pytest.mark.gpu

MEASURED_GMM, BAR_GMM = 2.51e-5, 2e-4        # worst: n = 20000, K = 2; the others 7.3e-6 .. 2.1e-5
MEASURED_IV, BAR_IV = 1.67e-6, 7e-6          # worst: eot = 3 through noise:40 without companions; K = 2 and 4: 1.4e-6, 1.5e-6

SEED, STREAM = 77, 3
ROOM = "t60:100-200,drr:6,taps:256,delay:8"
IV_SMALL = dict(C=64, D=72, R=32, L=16, n_speakers=2, seed=4)
OSI_KW = dict(target=1, threshold=-10.0)
COMPANIONS_REFUSAL = "white-box gradients: companions are set (fb_set_companions: clear them)"
IV_EOT_REFUSAL = "white-box gradients: fb_set_eot(2) is in force on an i-vector system (per-replica i-vector state is not kept: set 1)"
IV_REFUSAL = "white-box gradients: an i-vector system is loaded (GMM-UBM systems only in this version)"


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
    e.set_wb_universal(False)


def _p(task, attack, kw, **more):
    return nes_params(task, attack, samples_per_draw=0, seed=SEED, stream=STREAM, **dict(kw, **more))


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _chain(spec):
    return [tuple(s) for s in IT.parse(spec)] if spec else []


# ------------------------------------------------------------------------------------- 1. the hook, exactly
@pytest.mark.parametrize("K,eot", [(2, 1), (3, 2), (32, 1), (4, 8)])
def test_hook_compose_t_is_the_numpy_sum(eng, K, eot):
    for n in (1, 3, 255, 256, 257, 2049, 4000):
        rng = np.random.RandomState(1000 * K + n)
        q, a0, comp3 = _rail_case(n, n + K)
        comp = comp3[rng.randint(0, 3, K - 1)]               # K - 1 rows drawn from the three rail cases
        if K > 2:
            comp[1] = np.roll(comp3[1], 1)
        cots = rng.randint(-2 ** 20, 2 ** 20, (K * eot, n)).astype(np.float64)
        got = eng.debug_wb_compose_t(cots, q, a0, comp, eot)
        assert eng.debug_wb_universal_route() == 1
        want = U.compose_t(cots, q, a0, comp, eot)
        assert np.array_equal(_bits(got), _bits(want)), (K, eot, n)
        m = U.mask_rows(q, a0, comp)
        rows = compose_row(q, a0, comp)
        if n >= 255:
            assert (~m[1:]).any() and (m[1:] & (rows[1:] == 32767)).any() and (m[1:] & (rows[1:] == -32768)).any()
        dead = ~m[1:].any(axis=0)                            # every companion clipped there: utterance 0's cotangents alone
        own = np.zeros(n)
        for j in range(eot):
            own = own + cots[j]
        assert np.array_equal(_bits(got[dead]), _bits(own[dead]))
        only = eng.debug_wb_compose_t(np.concatenate([np.zeros((eot, n)), cots[eot:]]), q, a0, comp, eot)
        assert np.array_equal(_bits(only[dead]), _bits(np.zeros(int(dead.sum()))))      # masked positions are exactly +0.0


# ------------------------------------------------------------------------------------- 2. the full gradient
def _setup(e, comp, r=1, spec=None, air=False, ratio=None, bpda=None):
    e.set_feature_compression(ratio, 10) if ratio else e.set_feature_compression(None)
    e.set_input_transform(spec)
    e.set_air_channel(ROOM if air else None)
    e.set_eot(r)
    e.set_companions(comp if len(comp) else None)
    e.set_wb_bpda(bool(r > 1 or spec) if bpda is None else bpda)
    e.set_wb_air(bool(air))
    e.set_wb_frontend(bool(ratio))
    e.set_wb_universal(True)


def _normals(e, chain, n, it, rho):
    return {s: e.debug_tf_noise(SEED, STREAM, it, 0, rho, s, 0, n) for s, st in enumerate(chain) if st[0] == B.NOISE}


#            name             n      K1  r  spec           air    ratio
GMM_CASES = [("n4000_k1",     4000,  1,  1, None,          False, None),
             ("n4000_k3",     4000,  3,  1, None,          False, None),
             ("n20000_k1",    20000, 1,  1, None,          False, None),
             ("n20000_k3",    20000, 3,  1, None,          False, None),
             ("ms7_qt512",    4000,  3,  1, "ms:7,qt:512", False, None),
             ("noise40_r3",   4000,  1,  3, "noise:40",    False, None),
             ("air_r2",       4000,  1,  2, None,          True,  None),
             ("feco0.5",      4000,  1,  1, None,          False, 0.5),
             ("k31",          4000,  31, 1, None,          False, None)]


@pytest.mark.parametrize("name,n,K1,r,spec,air,ratio", GMM_CASES, ids=[c[0] for c in GMM_CASES])
def test_get_grad_wb_from_against_the_restatement(eng, small_system, name, n, K1, r, spec, air, ratio):
    from tests.test_gpu_wb_frontend import _check_labels_against_feco_ref
    audio, original, comp = U.perturbed_case(n, K1)
    models = _load(eng, small_system, "OSI")
    p = _p("OSI", "targeted", OSI_KW)
    chain, it, Rn = _chain(spec), 5, (K1 + 1) * r
    rows = compose_row(quantize(audio), quantize(original), comp)
    try:
        _setup(eng, comp, r, spec, air, ratio)
        grad, al, sc = eng.get_grad_wb_from(p, audio, original, it)
        launches, route, air_launches, feco_launches = eng.debug_wb_universal_route(), eng.debug_wb_route(), eng.debug_wb_air_route(), eng.debug_wb_feco_route()
        kept = [eng.debug_wb_feco_state(rho) for rho in range(Rn)] if ratio else None
        nz = [_normals(eng, chain, n, it, rho) for rho in range(Rn)] if chain else None
        taps = [eng.debug_air_taps(SEED, STREAM, it, 0, rho)[0] for rho in range(Rn)] if air else None
        fc = None
        if ratio:
            eng.set_companions(None)
            eng.set_eot(1)
            empty = [_check_labels_against_feco_ref(eng, rows[rho // r], it, rho, ratio, 10, kept[rho]) for rho in range(Rn)]
            fc = [dict(labels=kept[rho][0], k=kept[rho][1].size, empty=empty[rho]) for rho in range(Rn)]
    finally:
        _clear(eng)
    ref = U.loss_and_grad(eng.cfg, models, "OSI", "targeted", audio, original, comp, r, feco=fc, chain=chain, normals=nz, taps=taps, **OSI_KW)
    err = rel_l2(grad, ref.grad)
    print("%s: K %d, eot %d, Tv %s, clipped %s, loss %.9g (restatement %.9g), min |c0 - thr| %.3g, relative L2 error %.3g"
          % (name, K1 + 1, r, ref.tv, ref.clipped, al, ref.loss, ref.margin, err))
    assert np.array_equal(ref.rows, rows)
    assert ref.clipped[1] >= 0.01 * n and ref.clipped[0] == 0                # the clip is exercised, and delta is not zero
    assert launches == 1 and air_launches == (1 if air else 0) and feco_launches == (Rn if ratio else 0)
    assert route == dict(ctl=0, ctl_rep=Rn, backward=Rn, chain_t=Rn if chain else 0)
    assert ref.margin > 1e-3
    assert abs(al - ref.loss) < 1e-3 and np.abs(sc - ref.scores).max() < 1e-3
    assert np.isfinite(grad).all() and grad.any()
    assert err < BAR_GMM


#           name           K1 r  spec
IV_CASES = [("iv_k1",      1, 1, None),
            ("iv_k3",      3, 1, None),
            ("iv_eot3",    0, 3, "noise:40"),
            ("iv_k2_eot2", 1, 2, "noise:40")]


@pytest.mark.parametrize("name,K1,r,spec", IV_CASES, ids=[c[0] for c in IV_CASES])
def test_get_grad_wb_from_on_the_small_ivector_system(eng, small_system, name, K1, r, spec):
    from tests.test_gpu_whitebox_iv import VAD_MARGIN, _assert_margins
    sy = synthetic_ivector_system(**IV_SMALL)
    tab = V.IvTables(sy)
    eng.load_ivector(sy, "OSI")
    audio, original, comp = U.perturbed_case(4000, K1)
    p = _p("OSI", "targeted", OSI_KW)
    chain, it, Rn = _chain(spec), 5, (K1 + 1) * r
    try:
        _setup(eng, comp, r, spec)
        eng.set_wb_ivector(True)
        grad, al, sc = eng.get_grad_wb_from(p, audio, original, it)
        sel, _info = eng.debug_iv_gselect()
        launches, route = eng.debug_wb_universal_route(), eng.debug_wb_route()
        _fl, _gg, al0, sc0 = (eng.get_grad(p, audio, it=it, want_grad=False) if K1 == 0 else (None, None, al, sc))
        nz = [_normals(eng, chain, 4000, it, rho) for rho in range(Rn)] if chain else None
    finally:
        _clear(eng)
        _load(eng, small_system, "OSI")
    own = U.loss_and_grad_iv(eng.cfg, tab, "OSI", "targeted", audio, original, comp, r, chain=chain, normals=nz, **OSI_KW)
    assert sel.shape[0] == sum(own.tv)
    cuts = np.cumsum([0] + own.tv)
    sels = [sel[cuts[rho]:cuts[rho + 1]] for rho in range(Rn)]
    ref = U.loss_and_grad_iv(eng.cfg, tab, "OSI", "targeted", audio, original, comp, r, chain=chain, normals=nz, sels=sels, **OSI_KW)
    for rho in range(Rn):
        _assert_margins(ref.reps[rho], sels[rho], "%s replica %d" % (name, rho))
    err = rel_l2(grad, ref.grad)
    print("%s: K %d, eot %d, Tv %s, clipped %s, loss %.9g (restatement %.9g), relative L2 error %.3g" % (name, K1 + 1, r, ref.tv, ref.clipped, al, ref.loss, err))
    assert al == al0 and np.array_equal(sc, sc0)                # (K = 1: a_0 is not read, and the forward is fb_get_grad's)
    if K1:
        assert ref.clipped[1] >= 40 and ref.clipped[0] == 0
    assert launches == (1 if K1 else 0)
    assert route == dict(ctl=0, ctl_rep=Rn, backward=Rn, chain_t=Rn if (chain or not K1) else 0, iv_ctl=0, iv_backend_t=Rn, iv_solve=Rn,
                         iv_stats_t=Rn, iv_post_t=Rn)
    assert ref.margin > VAD_MARGIN and abs(al - ref.loss) < 1e-3 and np.abs(sc - ref.scores).max() < 1e-3
    assert np.isfinite(grad).all() and grad.any()
    assert err < BAR_IV


# ------------------------------------------------------------------------------------- 3. exact properties
@pytest.mark.parametrize("r", [1, 3])
@pytest.mark.parametrize("victim", ["gmm", "ivector"])
def test_forward_is_get_grads_with_companions(eng, small_system, victim, r):
    audio, comp = U.utterances(4000, 2)
    if victim == "ivector":
        eng.load_ivector(synthetic_ivector_system(**IV_SMALL), "OSI")
    else:
        _load(eng, small_system, "OSI")
    p = _p("OSI", "targeted", OSI_KW)
    try:
        _setup(eng, comp, r, "noise:40" if r > 1 else None)
        eng.set_wb_ivector(victim == "ivector")
        for it in (0, 7):
            _g, al, sc = eng.get_grad_wb_iter(p, audio, it)
            _fl, _gg, al0, sc0 = eng.get_grad(p, audio, it=it, want_grad=False)
            assert al == al0 and np.array_equal(_bits(sc), _bits(sc0)), (r, it)
        with_comp = eng.get_grad(p, audio, it=0, want_grad=False)[2]
        eng.set_companions(None)
        assert with_comp != eng.get_grad(p, audio, it=0, want_grad=False)[2]       # and the companions did something
    finally:
        _clear(eng)
        _load(eng, small_system, "OSI")


def test_one_utterance_with_the_switch_on_is_the_switch_off(eng, small_system):
    audio = R.test_audio(4000)
    _load(eng, small_system, "OSI")
    p = nes_params("OSI", "targeted", target=1, threshold=0.0, max_iter=4)
    off = eng.get_grad_wb(p, audio)
    off_route, off_nes = eng.debug_wb_route(), eng.debug_nes_route()
    off_attack = eng.attack_wb(p, audio)
    off_attack_route, off_attack_nes = eng.debug_wb_route(), eng.debug_nes_route()
    try:
        eng.set_wb_universal(True)
        on = eng.get_grad_wb(p, audio)
        on_route, on_nes, on_uni = eng.debug_wb_route(), eng.debug_nes_route(), eng.debug_wb_universal_route()
        frm = eng.get_grad_wb_from(p, audio, 0.5 * audio, 0)              # (a_0 is not read without companions)
        frm_route, frm_uni = eng.debug_wb_route(), eng.debug_wb_universal_route()
        on_attack = eng.attack_wb(p, audio)
        on_attack_route, on_attack_nes, on_attack_uni = eng.debug_wb_route(), eng.debug_nes_route(), eng.debug_wb_universal_route()
        eng.set_wb_bpda(True)
        eng.set_eot(2)
        eot_on = eng.get_grad_wb(p, audio)
        eot_on_route, eot_on_uni = eng.debug_wb_route(), eng.debug_wb_universal_route()
        eng.set_wb_universal(False)
        eot_off = eng.get_grad_wb(p, audio)
        eot_off_route = eng.debug_wb_route()
    finally:
        _clear(eng)
    for got in (on, frm):
        assert np.array_equal(_bits(off[0]), _bits(got[0])) and off[1] == got[1] and np.array_equal(off[2], got[2])
    assert off_route == on_route == frm_route == dict(ctl=1, ctl_rep=0, backward=1, chain_t=0) and off_nes == on_nes
    assert on_uni == 0 and frm_uni == 0 and on_attack_uni == 0 and eot_on_uni == 0
    assert off_attack_route == on_attack_route and off_attack_nes == on_attack_nes
    for x, y in zip(off_attack, on_attack):
        assert np.array_equal(x, y)
    assert np.array_equal(_bits(eot_on[0]), _bits(eot_off[0])) and eot_on[1] == eot_off[1]
    assert eot_on_route == eot_off_route == dict(ctl=0, ctl_rep=2, backward=2, chain_t=2)


def test_an_ivector_system_at_one_utterance_with_the_switch_on_is_the_switch_off(eng, small_system):
    audio = R.test_audio(4000)
    eng.load_ivector(synthetic_ivector_system(**IV_SMALL), "OSI")
    p = _p("OSI", "targeted", OSI_KW)
    try:
        eng.set_wb_ivector(True)
        off = eng.get_grad_wb_iter(p, audio, 1)
        off_route, off_nes = eng.debug_wb_route(), eng.debug_nes_route()
        eng.set_wb_universal(True)
        on = eng.get_grad_wb_iter(p, audio, 1)
        on_route, on_nes, on_uni = eng.debug_wb_route(), eng.debug_nes_route(), eng.debug_wb_universal_route()
    finally:
        _clear(eng)
        _load(eng, small_system, "OSI")
    assert np.array_equal(_bits(off[0]), _bits(on[0])) and off[1] == on[1] and np.array_equal(off[2], on[2])
    assert off_route == on_route and off_route["iv_ctl"] == 1 and off_route["ctl_rep"] == 0 and off_nes == on_nes and on_uni == 0


def test_original_none_is_get_grad_wb_iter(eng, small_system):
    audio, comp = U.utterances(4000, 2)
    _load(eng, small_system, "OSI")
    p = _p("OSI", "targeted", OSI_KW)
    try:
        _setup(eng, comp)
        a = eng.get_grad_wb_iter(p, audio, 2)
        b = eng.get_grad_wb_from(p, audio, None, 2)
        c = eng.get_grad_wb_from(p, audio, audio, 2)
        import ctypes as C
        grad = np.empty(4000)
        sc = np.empty(eng.n_speakers)
        al = C.c_double()
        N.check(eng._L.fb_get_grad_wb_from(eng._h, C.byref(p), N.ptr(np.ascontiguousarray(audio)), None, C.c_int64(4000), C.c_int(2),
                                           C.byref(al), N.ptr(grad), N.ptr(sc)))
    finally:
        _clear(eng)
    for got in (b, c, (grad, al.value, sc)):
        assert np.array_equal(_bits(a[0]), _bits(got[0])) and a[1] == got[1] and np.array_equal(a[2], got[2])
    assert a[0].any()


def test_a_companion_equal_to_the_original_doubles_the_halved_gradient(eng, small_system):
    """With a_1 = a_0 utterance 1's composed row is q + a_0 - a_0 = q, nothing clips, and both replicas score the same row: the
    mean loss is (l + l) / 2 = l, each replica's weights are w / 2 -- an exact scaling by a power of two all through the backward --
    and grad = (+0.0 + g / 2) + g / 2 = g, the single-row gradient, bit for bit (eot = 1, no random stage)."""
    original = R.test_audio(4000)
    audio = original + np.where(np.random.RandomState(3).randint(0, 2, 4000) == 1, 3.0, -3.0) / 32768.0
    _load(eng, small_system, "OSI")
    p = _p("OSI", "targeted", OSI_KW)
    single = eng.get_grad_wb_iter(p, audio, 0)
    try:
        _setup(eng, quantize(original)[None, :])
        double = eng.get_grad_wb_from(p, audio, original, 0)
        launches, route = eng.debug_wb_universal_route(), eng.debug_wb_route()
    finally:
        _clear(eng)
    assert launches == 1 and route == dict(ctl=0, ctl_rep=2, backward=2, chain_t=0)
    assert double[1] == single[1] and np.array_equal(_bits(double[2]), _bits(single[2]))
    assert np.array_equal(_bits(double[0]), _bits(single[0])) and single[0].any()


def test_two_fresh_engines_give_equal_bits(small_system):
    audio, original, comp = U.perturbed_case(4000, 2)
    p = _p("OSI", "targeted", OSI_KW)
    got = []
    for _ in range(2):
        e = Engine(0)
        try:
            _load(e, small_system, "OSI")
            _setup(e, comp, 2, "noise:40")
            got.append(e.get_grad_wb_from(p, audio, original, 2))
        finally:
            e.close()
    a, b = got
    assert np.array_equal(_bits(a[0]), _bits(b[0])) and a[1] == b[1] and np.array_equal(a[2], b[2])


# ------------------------------------------------------------------------------------- 4. a whole attack is its replay
def replay(e, p, audio):
    """tests/test_gpu_bpda.py's replay with a_0 held at the attack's start: FakeBob.attack (FAKEBOB.py:157-220) on the host in
    numpy float64, the gradient from fb_get_grad_wb_from at every iterate with the loop index as the epoch of the draws"""
    audio = np.asarray(audio, np.float64)
    adver, grad_m, lr, ls, rows = audio.copy(), np.zeros_like(audio), p.max_lr, [], []
    lower, upper = np.clip(audio - p.epsilon, -1.0, 1.0), np.clip(audio + p.epsilon, -1.0, 1.0)
    last = p.max_iter - 1
    for it in range(p.max_iter):
        g, al, sc = e.get_grad_wb_from(p, adver, audio, it)
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
@pytest.mark.parametrize("victim", ["gmm", "ivector"])
def test_a_whole_attack_is_its_replay(eng, small_system, monkeypatch, victim, batch):
    iters = 4 if victim == "gmm" else 3
    if victim == "ivector":
        eng.load_ivector(synthetic_ivector_system(**IV_SMALL), "OSI")
    else:
        _load(eng, small_system, "OSI")
    audio, comp = U.utterances(4000, 2)
    comp[0] = U.perturbed_case(4000, 2)[2][0]                # the loud companion: samples clip as the perturbation grows
    # (adver_thresh keeps the mean loss above zero, so that every iteration runs)
    p = nes_params("OSI", "targeted", target=1, threshold=0.0, adver_thresh=50.0, max_iter=iters, plateau_length=2, seed=SEED, stream=STREAM)
    monkeypatch.setenv("FB_ATTACK_BATCH", batch)
    try:
        _setup(eng, comp)
        eng.set_wb_ivector(victim == "ivector")
        adv, flag, adv_f, trace = eng.attack_wb(p, audio)
        launches, route = eng.debug_wb_universal_route(), eng.debug_wb_route()
        r_adv, r_flag, r_adv_f, r_trace = replay(eng, p, audio)
    finally:
        _clear(eng)
        _load(eng, small_system, "OSI")
    print("%s, batch %s: %d rows, flag %d, loss %s, lr %s" % (victim, batch, trace.shape[0], flag, trace[:, 1], trace[:, 2]))
    assert launches == iters and route["ctl_rep"] == route["backward"] == 3 * iters and route["chain_t"] == 0 and route["ctl"] == 0
    if victim == "ivector":
        assert route["iv_ctl"] == 0 and route["iv_solve"] == route["iv_post_t"] == 3 * iters
    S = 3 if victim == "gmm" else IV_SMALL["n_speakers"]
    assert trace.shape == r_trace.shape == (iters, 3 + S) and np.array_equal(_bits(trace), _bits(r_trace))
    assert flag == r_flag and np.array_equal(_bits(adv_f), _bits(r_adv_f)) and np.array_equal(adv, r_adv)
    assert len(set(trace[:, 1])) == iters
    m = U.mask_rows(adv, quantize(audio), comp)
    assert (~m[1]).any()                                     # and the clip was met on the way


# ------------------------------------------------------------------------------------- 5. refusals
WB_P = nes_params("OSI", "targeted", target=1, threshold=0.0, max_iter=3)
NES_P = nes_params("OSI", "targeted", target=1, threshold=0.0, max_iter=3, samples_per_draw=6, seed=9)


def _refused(e, audio, p=WB_P, code=N.FB_E_STATE):
    for call in (lambda: e.get_grad_wb(p, audio), lambda: e.get_grad_wb_iter(p, audio, 1), lambda: e.get_grad_wb_from(p, audio, audio, 1),
                 lambda: e.attack_wb(p, audio)):
        with pytest.raises(N.NativeError) as ex:
            call()
        assert ex.value.code == code, str(ex.value)
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


def _others(e, m):
    e.set_wb_bpda(bool(m & 1))
    e.set_wb_ivector(bool(m & 2))
    e.set_wb_air(bool(m & 4))
    e.set_wb_frontend(bool(m & 8))


def test_the_switch_takes_0_or_1(eng):
    assert eng.wb_universal is False
    eng.set_wb_universal(True)
    try:
        for bad in (2, -1):
            with pytest.raises(N.NativeError) as ex:
                eng.set_wb_universal(bad)
            assert ex.value.code == N.FB_E_ARG and eng.wb_universal is True     # the setting stays
    finally:
        eng.set_wb_universal(False)


def test_switch_off_refuses_companions_as_before(eng, small_system, nes_baseline):
    audio, comp = U.utterances(4000, 1)
    _load(eng, small_system, "OSI")
    try:
        for others in range(16):
            _others(eng, others)
            eng.set_companions(comp)
            msg = _refused(eng, audio)
            assert msg.endswith(COMPANIONS_REFUSAL + " (code %d)" % N.FB_E_STATE), (others, msg)
            _clear(eng)
            _same_attack(eng, nes_baseline)
    finally:
        _clear(eng)


def test_switch_off_refuses_ivector_eot_as_before(eng, small_system, nes_baseline):
    audio = R.test_audio(4000)
    eng.load_ivector(synthetic_ivector_system(**IV_SMALL), "OSI")
    try:
        for others in range(16):
            _others(eng, others)
            eng.set_eot(2)
            msg = _refused(eng, audio)
            assert msg.endswith((IV_EOT_REFUSAL if others & 2 else IV_REFUSAL) + " (code %d)" % N.FB_E_STATE), (others, msg)
            _clear(eng)
    finally:
        _clear(eng)
        _load(eng, small_system, "OSI")
    _same_attack(eng, nes_baseline)


ON_CASES = {
    "chain_without_bpda": (lambda e: e.set_input_transform("qt:64"), "input-transform"),
    "codec_without_bpda": (lambda e: e.set_codec("ulaw"), "codec"),
    "eot_without_bpda": (lambda e: e.set_eot(2), "fb_set_eot"),
    "air_without_wb_air": (lambda e: e.set_air_channel(ROOM), "air channel"),
    "feco_without_wb_frontend": (lambda e: e.set_feature_compression(0.5, 10), "feature compression"),
    "dither_without_wb_frontend": (lambda e: e.set_frontend(dither=1.0), "dither"),
}


@pytest.mark.parametrize("case", sorted(ON_CASES))
def test_still_refused_with_the_switch_on(eng, small_system, nes_baseline, case):
    on, word = ON_CASES[case]
    audio, comp = U.utterances(4000, 2)
    _load(eng, small_system, "OSI")
    try:
        eng.set_wb_universal(True)
        eng.set_companions(comp)
        eng.set_wb_bpda(case.startswith("air") or "frontend" in case)
        on(eng)
        assert word in _refused(eng, audio)
    finally:
        _clear(eng)
    _same_attack(eng, nes_baseline)


def test_the_other_attacks_still_refuse_companions(eng, small_system, nes_baseline):
    audio, comp = U.utterances(4000, 2)
    _load(eng, small_system, "OSI")
    try:
        eng.set_wb_universal(True)
        eng.set_companions(comp)
        for name, call in (("fb_attack_pso", lambda: eng.attack_pso(NES_P, pso_params(particles=4), audio)),
                           ("fb_attack_kenansville", lambda: eng.attack_kenansville(NES_P, kv_params(), audio)),
                           ("fb_estimate_threshold", lambda: eng.estimate_threshold(NES_P, 0.0, audio))):
            with pytest.raises(N.NativeError) as ex:
                call()
            assert ex.value.code == N.FB_E_STATE and name in str(ex.value) and "companion" in str(ex.value)
        assert "the companions" in _refused(eng, R.test_audio(4001), code=N.FB_E_ARG)        # N != the companions' N
        assert "the companions" in _refused(eng, R.test_audio(3999), code=N.FB_E_ARG)
    finally:
        _clear(eng)
    _same_attack(eng, nes_baseline)


def test_more_than_32_replicas_is_refused_at_the_setters(eng, small_system, nes_baseline):
    import ctypes as C
    _audio, comp = U.utterances(4000, 16)
    _load(eng, small_system, "OSI")
    try:
        eng.set_wb_universal(True)
        eng.set_wb_bpda(True)
        eng.set_companions(comp)                             # K = 17
        with pytest.raises(N.NativeError) as ex:
            eng.set_eot(2)
        assert ex.value.code == N.FB_E_ARG and eng.eot == 1
        eng.set_companions(None)
        eng.set_eot(2)
        assert eng._L.fb_set_companions(eng._h, N.ptr(comp), C.c_int(16), C.c_int64(4000)) == N.FB_E_ARG
        with pytest.raises(ValueError):
            eng.set_companions(comp)
    finally:
        _clear(eng)
    _same_attack(eng, nes_baseline)


# ------------------------------------------------------------------------------------- 6. AdaptivePGD and the driver
def test_adaptive_pgd_universal_returns_fakebobs_pair_checkpoint_and_per_utterance(small_system, tmp_path):
    from fakebob_amd import companions as CP
    from fakebob_amd.pgd import PGD, AdaptivePGD
    from fakebob_amd.systems import gmm_OSI
    ubm, spk = small_system
    ml = [["spk%d" % i, "utt%d" % i, g, -60.0 - i, 2.0 + i] for i, g in enumerate(spk)]
    model = gmm_OSI(str(tmp_path / "osi"), ml, ubm, pre_model_dir=str(tmp_path), threshold=0.0)
    try:
        audio, comp = U.utterances(4000, 2)
        with pytest.raises(TypeError):                                             # PGD itself takes none
            PGD("OSI", "targeted", model, max_iter=5, seed=11, verbose=False).attack(audio, None, threshold=1e3, target=1, companions=list(comp))
        with pytest.raises(ValueError, match="universal"):
            AdaptivePGD("OSI", "targeted", model, bpda=False, max_iter=5, seed=11, verbose=False).attack(audio, None, threshold=1e3, target=1,
                                                                                                     companions=list(comp))
        pgd = AdaptivePGD("OSI", "targeted", model, bpda=False, universal=True, max_iter=5, seed=11, verbose=False)
        assert model.engine.wb_universal and pgd.universal and not model.engine.wb_bpda
        cp = str(tmp_path / "pgd.cp")
        with pytest.raises(ValueError, match="lengths"):
            pgd.attack(audio, None, threshold=1e3, target=1, companions=[comp[0], comp[1][:-1]])
        res = pgd.attack(audio, cp, threshold=1e3, target=1, companions=list(comp))
        adv, flag = res
        assert model.engine.companions is None                                     # for that call only
        assert adv.dtype == np.int16 and adv.shape == (4000, 1) and flag == -1
        assert model.engine.debug_wb_universal_route() == 5
        with open(cp, "rb") as r:
            rows = pickle.load(r)
        assert len(rows) == 5 and rows[-1][1][0] < rows[0][1][0]                   # the mean loss went down
        for row in rows:
            assert len(row) == 4 and row[1].shape == (1,) and row[2].shape == (3,) and isinstance(row[3], float)
        assert np.array_equal(res.perturbation_i16, adv[:, 0].astype(np.int32) - CP.cast_i16(audio))
        per = res.per_utterance
        assert [d["utterance"] for d in per] == [0, 1, 2] and np.array_equal(per[0]["audio_i16"], adv[:, 0])
        moved = res.apply_perturbation(list(comp))
        for u in (1, 2):
            assert np.array_equal(per[u]["audio_i16"], moved[u - 1])
            assert np.array_equal(per[u]["audio_i16"], compose_row(adv[:, 0], CP.cast_i16(audio), comp)[u])
        assert all(d["success"] == (int(d["decision"]) == 1) for d in per)
        plain = pgd.attack(audio, None, threshold=1e3, target=1)                  # without companions: PGD's own attack
        assert plain.per_utterance is None and model.engine.debug_wb_universal_route() == 0
    finally:
        model.engine.close()


def test_ivector_pgd_universal_takes_companions_and_an_eot_size(eng, small_system):
    from fakebob_amd.pgd import IvectorPGD
    eng.load_ivector(synthetic_ivector_system(**dict(IV_SMALL, n_speakers=1)), "SV")
    audio, comp = U.utterances(4000, 1)

    class Model(object):      # the engine behind FakeBob's model interface, as systems.iv_SV presents it
        task, engine = "SV", eng

        def make_decisions(self, w, **kw):
            raw, _tv = eng.score_raw([np.asarray(w, np.int16)])
            return int(raw[0, 0] > 0), float(raw[0, 0])
    try:
        with pytest.raises(ValueError, match="universal"):
            IvectorPGD("SV", "targeted", Model(), bpda=True, eot_size=2, verbose=False)
        pgd = IvectorPGD("SV", "targeted", Model(), bpda=True, universal=True, eot_size=2, max_iter=3, max_lr=2.0 ** -15, momentum=0.0,
                         seed=11, verbose=False)
        assert eng.wb_universal and eng.wb_ivector and eng.wb_bpda and eng.eot == 2 and pgd.eot_size == 2
        res = pgd.attack_universal(audio, None, list(comp), threshold=1e3)
        adv, flag = res
        route, launches = eng.debug_wb_route(), eng.debug_wb_universal_route()
        assert adv.shape == (4000, 1) and flag == -1 and eng.companions is None
        assert launches == 3 and route["ctl_rep"] == route["iv_solve"] == route["backward"] == 12 and route["iv_ctl"] == 0
        assert [d["utterance"] for d in res.per_utterance] == [0, 1]
    finally:
        _clear(eng)
        _load(eng, small_system, "OSI")


def test_attack_main_pgd_wb_universal_on_the_synthetic_site(tmp_path, capsys):
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
                                "pgd", "--wb-universal", "--companions", "2", "--streams", "1", "--seed", "7"] + site
    np.random.seed(3)
    g, results, _thr = AM.main(argv)
    out = capsys.readouterr().out
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
        AM.main([a for a in argv if a != "--wb-universal"])      # without the flag --attack pgd --companions stays refused
    with pytest.raises(SystemExit):
        AM.main([("nes" if a == "pgd" else a) for a in argv])     # the flag belongs to --attack pgd
    capsys.readouterr()


# ------------------------------------------------------------------------------------- 7. what it is for
def test_the_universal_attack_beats_the_single_utterance_attack(eng, small_system):
    """tests/test_universal_vjp_host.py's comparison on the device: thirty plain sign steps of fb_attack_wb on the mean loss over
    K = 4 utterances, and the same thirty steps on utterance 0 alone; both perturbations scored as the mean loss over the four
    utterances (fb_get_grad_wb_from's forward with a_0 = the clean audio).  The three numbers are in DESIGN.md section 6."""
    audio, comp = U.utterances(ATTACK_N, ATTACK_K1)
    _load(eng, small_system, "SV")
    p = nes_params("SV", "untargeted", threshold=ATTACK_THRESHOLD, max_iter=ATTACK_STEPS, max_lr=ATTACK_LR, epsilon=ATTACK_EPS, momentum=0.0,
                   plateau_length=ATTACK_STEPS + 1)
    try:
        eng.set_wb_universal(True)
        _adv, _flag, single, trace1 = eng.attack_wb(p, audio)
        eng.set_companions(comp)
        _adv, _flag, universal, trace = eng.attack_wb(p, audio)
        launches = eng.debug_wb_universal_route()

        def mean_loss(a):
            return eng.get_grad_wb_from(p, a, audio, 0, want_grad=False)[1]
        clean, uni, one = mean_loss(audio), mean_loss(universal), mean_loss(single)
    finally:
        _clear(eng)
        _load(eng, small_system, "OSI")
    print("mean loss over K = %d utterances: clean %.9g, universal %.9g, utterance 0's steps %.9g" % (ATTACK_K1 + 1, clean, uni, one))
    assert launches == ATTACK_STEPS and trace.shape[0] == trace1.shape[0] == ATTACK_STEPS
    assert trace[0, 1] == clean
    assert np.isfinite([clean, uni, one]).all()
    assert uni < clean and uni < one
