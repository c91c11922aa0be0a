"""fb_attack_psy on the device (the "masking" section of include/fakebob_hip.h) against its host references (tests/psy_ref.py,
which tests/test_psy_host.py pins).

The loss kernel is an in-LDS radix-2 FFT; the reference is torch.fft.rfft with autograd.  The reference against itself (rfft
against an explicit DFT matrix, tests/test_psy_host.py, on the shapes used here) is SELF_GD = 6e-16 of max |gd|, SELF_D = 3e-16
relative, SELF_P = 1.5e-15 of max P; the kernel is given 64 times that, because an FFT of up to 2048 points rounds about log2 W
times where the DFT matrix rounds once:
  gd   max |gd - ref| / max |ref|       bar BAR_GD = 3.84e-14     measured worst MEASURED_GD
  D    |D - ref| / ref                  bar BAR_D  = 1.92e-14     measured worst MEASURED_D
  P    max |P - ref| / max ref          bar BAR_P  = 9.6e-14      measured worst MEASURED_P
n_over is exact, under the condition (asserted on the reference's own numbers) that no bin lies within 1e-9 relative of its
threshold.  The step kernel is compared with its numpy twin as CW2's is: m1, m2, mod, gate, take and the best slots bit for
bit, what has passed through tanh to CW2's bars.
"""
import ctypes as C
import os
import pickle

import numpy as np
import pytest

from fakebob_amd import _native as N
from fakebob_amd import masking as M
from fakebob_amd.engine import Engine, cw2_params, nes_params, psy_params
from fakebob_amd.models import synthetic_audio
from tests import cw2_ref as C2
from tests import psy_ref as PR
from tests import whitebox_ref as R
from tests.test_gpu_cw2 import BAR_L2, BAR_X, STATE_CASES, STEP_STATES, SV_LOOSE, _iv_system, _load, _switches

pytestmark = pytest.mark.gpu

SELF_GD, SELF_D, SELF_P = 6e-16, 3e-16, 1.5e-15          # tests/test_psy_host.py::test_the_reference_against_itself
BAR_GD, BAR_D, BAR_P = 64 * SELF_GD, 64 * SELF_D, 64 * SELF_P
MEASURED_GD, MEASURED_D, MEASURED_P = 7.49e-16, 1.84e-15, 1.03e-15    # the first run on an MI355X
FS = 16000


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


_thresholds = {}


def _theta(W, n, seed=0):
    """the threshold of synthetic_audio(seed, n) at window W: computed once"""
    if (W, n, seed) not in _thresholds:
        _thresholds[(W, n, seed)] = M.masking_threshold(synthetic_audio(seed, n), FS, W)
    return _thresholds[(W, n, seed)]


# ------------------------------------------------------------------------------------- 1. the loss kernel against the reference
LOSS_SHAPES = [(512, 512), (512, 513), (512, 4000), (1024, 1024 + 256 + 1), (2048, 2048), (2048, 2048 + 3 * 512 + 5)]


@pytest.mark.parametrize("amp", [1, 8, 64])
@pytest.mark.parametrize("W,n", LOSS_SHAPES)
def test_loss_kernel_against_the_reference(eng, W, n, amp):
    theta, psd_max = _theta(W, n)
    delta = np.random.default_rng(1).normal(0.0, amp / 32768.0, n)
    ref = PR.loss(delta, theta, psd_max, W)
    assert ref["margin"] > 1e-9, "a bin within 1e-9 of its threshold (%.3g): another seed, not another test" % ref["margin"]
    m = psy_params(theta, psd_max, W)
    got = eng.debug_psy_loss(m, delta, want_P=True)
    again = eng.debug_psy_loss(m, delta, want_P=True)
    gmax = np.abs(ref["gd"]).max()
    eg = float(np.abs(got["gd"] - ref["gd"]).max() / gmax) if gmax > 0 else float(np.abs(got["gd"]).max())
    eD = abs(got["D"] - ref["D"]) / ref["D"] if ref["D"] > 0 else abs(got["D"])
    eP = float(np.abs(got["P"] - ref["P"]).max() / ref["P"].max())
    print("loss kernel W=%d N=%d amp=%d: D %.6g n_over %d (ref %d) margin %.3g; error gd %.3g D %.3g P %.3g" %
          (W, n, amp, got["D"], got["n_over"], ref["n_over"], ref["margin"], eg, eD, eP))
    assert got["n_over"] == ref["n_over"]
    assert got["P"].shape == theta.shape and eP <= BAR_P
    if amp == 1:
        assert ref["D"] == 0.0 and ref["n_over"] == 0
        assert got["D"] == 0.0 and got["n_over"] == 0 and not got["gd"].any()
    assert eD <= BAR_D and eg <= BAR_GD
    assert got["D"] == again["D"] and got["n_over"] == again["n_over"]
    assert np.array_equal(_bits(got["gd"]), _bits(again["gd"])) and np.array_equal(_bits(got["P"]), _bits(again["P"]))


# ------------------------------------------------------------------------------------- 2. the step kernel against its twin
@pytest.mark.parametrize("l2_weight", [0.0, 0.5])
@pytest.mark.parametrize("state", sorted(STEP_STATES))
@pytest.mark.parametrize("n", [1, 255, 256, 257, 4000])
def test_step_kernel_against_the_twin(eng, n, state, l2_weight):
    al, gbest = STEP_STATES[state]
    t = 7
    rng = np.random.default_rng(1000 * n + 10 * t + len(state))
    a0 = rng.uniform(-0.95, 0.95, n)
    w0 = C2.w0_of(a0)
    mod = rng.normal(scale=0.25, size=n)        # (see the condition on N = 1 below)
    m1 = rng.normal(scale=1e-1, size=n)
    m2 = rng.uniform(1e-4, 1e-1, n)
    g = rng.normal(size=n)
    gd = rng.normal(scale=3.0, size=n)
    x = np.tanh(w0 + mod)
    q = cw2_params(abort_every=0)
    c, D, n_over = 0.375, 1.25, 17
    p1 = p2 = 1.0
    for _ in range(t + 1):
        p1 *= q.beta1
        p2 *= q.beta2
    got = eng.debug_psy_step(q, l2_weight, g, gd, x, a0, w0, mod, m1, m2, al, c, D, n_over, gbest, t, p1, p2)
    l2 = C2.l2_blocks(x, a0)
    d = PR.control(al, l2, D, l2_weight, c, gbest, t, float("inf"), 0)
    r_mod, r_m1, r_m2, r_x = PR.adam_step(g, gd, x, a0, w0, mod, m1, m2, c, d["gate"], l2_weight, p1, p2, q.lr, q.beta1, q.beta2,
                                          q.adam_eps)
    assert (got["gate"], got["take"]) == (d["gate"], d["take"]) == (1 if al > 0 else 0, 1 if state == "gate0_take1" else 0)
    assert got["l2"] == l2 and got["dist"] == d["dist"] == D + l2_weight * l2      # no tanh on this side of them: exact
    for name, ref in (("m1", r_m1), ("m2", r_m2), ("mod", r_mod)):
        assert np.array_equal(_bits(got[name]), _bits(ref)), name
    if d["take"]:
        assert np.array_equal(got["best_row"], C2.cast_i16(x)) and np.array_equal(_bits(got["best_x"]), _bits(x))
    else:
        assert np.array_equal(got["best_row"], C2.cast_i16(a0)) and np.array_equal(_bits(got["best_x"]), _bits(a0))
    ex = float(np.abs(got["x_next"] - r_x).max() / np.abs(r_x).max())
    r_l2 = C2.l2_blocks(r_x, a0)
    el = abs(got["l2_next"] - r_l2) / r_l2
    assert got["l2_next"] == C2.l2_blocks(got["x_next"], a0)
    if n == 1:
        # one sample has no averaging: l2 = d^2 moves by 2 ulp(x) / |d| when the device's tanh is one unit in the last place
        # from numpy's (which BAR_X allows).  With mod of size 1e-2, as CW2's test draws it, |d| is 5e-3 and that alone is
        # 5.6e-15, above BAR_L2 (first run on an MI355X); the condition, on the reference's own numbers: half the bar at most
        assert 2.0 * np.spacing(np.abs(r_x[0])) / abs(r_x[0] - a0[0]) <= BAR_L2 / 2, "ill-conditioned single sample: another seed"
    print("step kernel N=%d %s l2_weight=%g: x_next relative error %.3g, l2 relative error %.3g" % (n, state, l2_weight, ex, el))
    assert ex <= BAR_X and el <= BAR_L2


# ------------------------------------------------------------------------------------- 3. a whole attack is its replay
WHOLE = {
    "osi_targeted": ("OSI", dict(attack_type="targeted", target=1, threshold=0.0), None),
    "sv_untargeted": ("SV", dict(attack_type="untargeted", threshold=0.2), None),
    "ivector_osi": ("OSI", dict(attack_type="targeted", target=1, threshold=0.0), "iv"),
    "defended_eot2": ("OSI", dict(attack_type="targeted", target=1, threshold=0.0, seed=77, stream=3), "qt:512,noise:2"),
}
_replays = {}


def _setup(e, small_system, case):
    task, kw, extra = WHOLE[case]
    kw = dict(kw)
    p = nes_params(task, kw.pop("attack_type"), max_iter=8, samples_per_draw=0, **kw)
    if extra == "iv":
        e.load_ivector(_iv_system(), task)
        e.set_wb_ivector(True)
    else:
        _load(e, small_system, task)
    if extra not in (None, "iv"):
        e.set_input_transform(extra)
        e.set_wb_bpda(True)
        e.set_eot(2)
    return p


def _teardown(e):
    e.set_eot(1)
    e.set_wb_bpda(False)
    e.set_input_transform(None)
    e.set_wb_ivector(False)


@pytest.mark.parametrize("batch", ["1", "4"])
@pytest.mark.parametrize("case", sorted(WHOLE))
def test_a_whole_attack_is_its_replay(eng, small_system, monkeypatch, case, batch):
    q = cw2_params(search_steps=2, abort_every=4, initial_const=1.0)
    audio = R.test_audio(4000)
    theta, psd_max = _theta(512, 4000)
    m = psy_params(theta, psd_max, 512, 0.0)
    monkeypatch.setenv("FB_ATTACK_BATCH", batch)
    try:
        p = _setup(eng, small_system, case)
        it0 = eng.stats()["nes_iters"]
        got = eng.attack_psy(p, q, m, audio)
        assert eng.stats()["nes_iters"] - it0 == got["trace"].shape[0]
        secs = eng.attack_iter_seconds(got["trace"].shape[0])
        if case not in _replays:
            _replays[case] = (PR.replay(eng, p, q, m, audio), got)
        ref, first = _replays[case]
    finally:
        _teardown(eng)
    tr, rt = got["trace"], ref["trace"]
    print("%s batch %s: rows %s, flag %d, c %s, loss %s, dist %s, n_over %s, margin %.3g LSB, theta margin %.3g" %
          (case, batch, got["rows_per_step"], got["success"], tr[:, 4], tr[:, 3], tr[:, 0], tr[:, 2], ref["min_margin"],
           ref["min_theta_margin"]))
    assert ref["min_margin"] > 1e-6 and ref["min_theta_margin"] > 1e-9       # else: change the seed, not the test
    assert (secs > 0).all()
    assert np.array_equal(got["rows_per_step"], ref["rows_per_step"]) and tr.shape == rt.shape
    assert got["success"] == ref["success"] and np.array_equal(got["adv"], ref["adv"]) and got["const"] == ref["const"]
    assert np.array_equal(_bits(tr[:, 3:]), _bits(rt[:, 3:]))                   # adver_loss, c, score0: they depend on the int16 rows only
    assert np.array_equal(tr[:, 2], rt[:, 2]) and got["n_over"] == ref["n_over"]
    ed = [abs(tr[r, 0] - rt[r, 0]) / rt[r, 0] if rt[r, 0] > 0 else abs(tr[r, 0]) for r in range(tr.shape[0])]
    print("worst dist relative error %.3g" % max(ed))
    assert max(ed) <= BAR_D
    if ref["success"] == 1:
        assert abs(got["best_dist"] - ref["best_dist"]) <= BAR_D * ref["best_dist"]
    else:
        assert got["best_dist"] == ref["best_dist"] == float("inf")
    for k in got:                                                               # FB_ATTACK_BATCH does not show in a single bit
        assert np.array_equal(np.asarray(got[k]), np.asarray(first[k])) or (np.asarray(got[k]).dtype == np.float64 and
                                                                               np.array_equal(_bits(got[k]), _bits(first[k]))), k


# ------------------------------------------------------------------------------------- 3b. the abort rule
@pytest.mark.parametrize("l2_weight", [0.0, 0.5])
def test_abort_rule_ends_every_search_step_at_its_second_iteration(eng, small_system, l2_weight):
    """CW2's test of this name with the masking distortion.  Adam's normalised step moves each mod[n] by about lr = 1e-12, so
    L = c adver_loss + dist changes by far less than 0.01 % between t = 0 and t = 1, and prev is +inf at t = 0: every search
    step writes two rows and takes one step.  The threshold is out of reach, so nothing is ever taken."""
    _load(eng, small_system, "SV")
    audio = R.test_audio(4000)
    m = psy_params(*_theta(512, 4000), window=512, l2_weight=l2_weight)
    p = nes_params("SV", "untargeted", max_iter=6, samples_per_draw=0, threshold=1e3)
    got = eng.attack_psy(p, cw2_params(search_steps=3, lr=1e-12, abort_every=1), m, audio)
    assert list(got["rows_per_step"]) == [2, 2, 2] and got["trace"].shape[0] == 6
    assert list(got["trace"][:, 4]) == [1e-3, 1e-3, 1e-2, 1e-2, 1e-3 * 10.0 * 10.0, 1e-3 * 10.0 * 10.0]
    assert got["success"] == -1 and got["best_dist"] == float("inf") and got["n_over"] == 0
    assert np.array_equal(got["adv"], C2.cast_i16(audio)) and np.array_equal(_bits(got["adver_f64"]), _bits(audio))
    never = eng.attack_psy(p, cw2_params(search_steps=3, lr=1e-12, abort_every=0), m, audio)
    assert list(never["rows_per_step"]) == [6, 6, 6]


# ------------------------------------------------------------------------------------- 4. it does what it is for
def test_it_hides_under_the_threshold(eng, small_system):
    _load(eng, small_system, "SV")
    audio = R.test_audio(4000)
    theta, psd_max = _theta(512, 4000)
    m = psy_params(theta, psd_max, 512, 0.0)
    p = nes_params("SV", "untargeted", max_iter=30, samples_per_draw=0, **SV_LOOSE)
    q = cw2_params(search_steps=4, lr=2.0 ** -13)
    got = eng.attack_psy(p, q, m, audio)
    tr = got["trace"]
    print("rows %s, c %s, best_dist %.6g, n_over %d, best_l2 %.6g, const %.6g" %
          (got["rows_per_step"], sorted(set(tr[:, 4])), got["best_dist"], got["n_over"], got["best_l2"], got["const"]))
    print("adver_loss", tr[:, 3])
    print("dist", tr[:, 0])
    print("n_over", tr[:, 2])
    assert got["success"] == 1 and list(got["rows_per_step"]) == [30] * 4
    ok = tr[:, 3] < 0
    assert ok.any() and got["best_dist"] == tr[ok, 0].min()
    best = int(np.flatnonzero(ok & (tr[:, 0] == got["best_dist"]))[0])         # (the first such row: `take` needs strictly less)
    assert got["best_l2"] == tr[best, 1] and got["n_over"] == tr[best, 2]
    _fl, _g, al, sc = eng.get_grad(p, got["adv"].astype(np.float64) / 32768.0, want_grad=False)
    assert al == tr[best, 3] and np.array_equal(sc[:1], tr[best, 5:6])           # the returned row scores what the trace says
    assert np.array_equal(got["adv"], C2.cast_i16(got["adver_f64"]))
    ref = PR.loss(got["adver_f64"] - audio, theta, psd_max, 512)
    print("reference at the returned iterate: D %.6g n_over %d margin %.3g" % (ref["D"], ref["n_over"], ref["margin"]))
    assert ref["margin"] > 1e-9 and ref["n_over"] == got["n_over"]
    assert abs(ref["D"] - got["best_dist"]) <= BAR_D * ref["D"] if ref["D"] > 0 else got["best_dist"] == 0.0
    cw = eng.attack_cw2(p, q, audio)
    assert cw["success"] == 1
    rc = PR.loss(cw["adver_f64"] - audio, theta, psd_max, 512)
    F, K = theta.shape
    print("same budget: masking attack D %.6g n_over %d / %d, l2 %.6g; CW2's best iterate D %.6g n_over %d / %d, l2 %.6g" %
          (ref["D"], ref["n_over"], F * K, got["best_l2"], rc["D"], rc["n_over"], F * K, cw["best_l2"]))


# ------------------------------------------------------------------------------------- 5. refusals
NES_P = nes_params("OSI", "targeted", target=1, threshold=0.0, max_iter=3, samples_per_draw=6, seed=9)
PSY_P = nes_params("OSI", "targeted", target=1, threshold=0.0, max_iter=3, samples_per_draw=0)


@pytest.fixture(scope="module")
def nes_baseline(small_system):
    """an fb_attack on a fresh engine: what the same call must return after every refusal"""
    e = Engine(0)
    try:
        _load(e, small_system, "OSI")
        return e.attack(NES_P, R.test_audio(4000))
    finally:
        e.close()


def _same_attack(e, nes_baseline):
    got = e.attack(NES_P, R.test_audio(4000))
    for a, b in zip(got, nes_baseline):
        assert np.array_equal(a, b)


def _raw(theta, n_frames, window, psd_max, l2_weight=0.0):
    """fb_psy_params without psy_params' own shape check"""
    theta = np.ascontiguousarray(theta, np.float64)
    m = N.PsyParams()
    m._theta = theta
    m.theta = theta.ctypes.data
    m.n_frames, m.window, m.psd_max, m.l2_weight = int(n_frames), int(window), float(psd_max), float(l2_weight)
    return m


def _refused(e, code, audio, m, p=PSY_P, q=None):
    with pytest.raises(N.NativeError) as ex:
        e.attack_psy(p, q if q is not None else cw2_params(search_steps=2), m, audio)
    assert ex.value.code == code, str(ex.value)
    return str(ex.value)


@pytest.mark.parametrize("switches", [False, True], ids=["switches_off", "switches_on"])
@pytest.mark.parametrize("case", sorted(STATE_CASES))
def test_refused_victims(eng, small_system, nes_baseline, case, switches):
    on, off, word = STATE_CASES[case]
    _load(eng, small_system, "OSI")
    audio = R.test_audio(4000)
    theta, psd_max = _theta(512, 4000)
    on(eng)
    try:
        _switches(eng, switches)
        msg = _refused(eng, N.FB_E_STATE, audio, psy_params(theta, psd_max, 512))
    finally:
        _switches(eng, False)
        off(eng)
    assert word in msg and "CW2" in msg          # (the same checks as fb_attack_cw2, word for word)
    _same_attack(eng, nes_baseline)


def test_argument_refusals(eng, small_system, nes_baseline):
    _load(eng, small_system, "OSI")
    audio = R.test_audio(4000)
    theta, psd_max = _theta(512, 4000)
    F = theta.shape[0]
    good = psy_params(theta, psd_max, 512)
    bad = theta.copy()
    bad[3, 5] = -1.0
    nan = theta.copy()
    nan[F - 1, 256] = float("nan")
    inf = theta.copy()
    inf[0, 0] = float("inf")
    wide = np.ones((F, 129))
    for m, word in ((_raw(wide, F, 256, psd_max), "window"), (_raw(theta, F, 513, psd_max), "window"), (_raw(theta, F, 0, psd_max), "window"),
                    (_raw(theta, F - 1, 512, psd_max), "n_frames"), (_raw(np.ones((F + 1, 257)), F + 1, 512, psd_max), "n_frames"),
                    (_raw(bad, F, 512, psd_max), "theta"), (_raw(nan, F, 512, psd_max), "theta"), (_raw(inf, F, 512, psd_max), "theta"),
                    (_raw(theta, F, 512, 0.0), "psd_max"), (_raw(theta, F, 512, -1.0), "psd_max"), (_raw(theta, F, 512, float("nan")), "psd_max"),
                    (_raw(theta, F, 512, float("inf")), "psd_max"), (_raw(theta, F, 512, psd_max, -0.5), "l2_weight"),
                    (_raw(theta, F, 512, psd_max, float("inf")), "l2_weight"), (_raw(theta, F, 512, psd_max, float("nan")), "l2_weight")):
        msg = _refused(eng, N.FB_E_ARG, audio, m)
        assert word in msg and "masking" in msg, (word, msg)
    t2048 = np.ones((1, 1025))
    assert "fewer than the window" in _refused(eng, N.FB_E_ARG, audio[:2000], _raw(t2048, 1, 2048, psd_max))
    # CW2's own argument rules, by the same checks
    for kw, word in ((dict(search_steps=0), "search_steps"), (dict(initial_const=0.0), "initial_const"), (dict(lr=float("nan")), "lr"),
                     (dict(adam_eps=0.0), "adam_eps"), (dict(beta1=1.0), "beta"), (dict(abort_every=-1), "abort_every")):
        assert word in _refused(eng, N.FB_E_ARG, audio, good, q=cw2_params(**kw)), kw
    assert "max_iter" in _refused(eng, N.FB_E_ARG, audio, good, nes_params("OSI", "targeted", target=1, max_iter=0))
    assert "target" in _refused(eng, N.FB_E_ARG, audio, good, nes_params("OSI", "targeted", target=3, max_iter=3))
    # the hooks refuse the same parameters
    with pytest.raises(N.NativeError) as ex:
        eng.debug_psy_loss(_raw(theta, F - 1, 512, psd_max), audio)
    assert ex.value.code == N.FB_E_ARG
    L, h = eng._L, eng._h
    adv, per = np.empty(4000, np.int16), np.zeros(32, np.int32)
    flag, no, dist, l2, cc, q = C.c_int(), C.c_int(), C.c_double(), C.c_double(), C.c_double(), cw2_params(search_steps=2)
    full = [h, C.byref(PSY_P), C.byref(q), C.byref(good), N.ptr(audio), C.c_int64(4000), N.ptr(adv), None, None, None, N.ptr(per),
            C.byref(flag), C.byref(dist), C.byref(l2), C.byref(no), C.byref(cc)]
    for null in (0, 1, 2, 3, 4, 6, 10, 11, 12, 13, 14, 15):                     # adver_f64, trace and n_trace may be null
        args = list(full)
        args[null] = None
        assert L.fb_attack_psy(*args) == N.FB_E_ARG, null
    null_theta = _raw(theta, F, 512, psd_max)
    null_theta.theta = None
    assert "threshold" in _refused(eng, N.FB_E_ARG, audio, null_theta)
    assert L.fb_attack_psy(*full) == N.FB_OK and flag.value in (1, -1)
    _same_attack(eng, nes_baseline)


def test_victims_that_need_a_switch_are_refused_without_it(eng, small_system, nes_baseline):
    _load(eng, small_system, "OSI")
    audio = R.test_audio(4000)
    m = psy_params(*_theta(512, 4000), window=512)
    for on, off, word in ((lambda: eng.set_input_transform("qt:64"), lambda: eng.set_input_transform(None), "input-transform"),
                          (lambda: eng.set_codec("ulaw"), lambda: eng.set_codec(None), "codec"),
                          (lambda: eng.set_eot(2), lambda: eng.set_eot(1), "fb_set_eot")):
        on()
        try:
            assert word in _refused(eng, N.FB_E_STATE, audio, m)
        finally:
            off()
    eng.load_ivector(_iv_system(), "OSI")
    assert "i-vector" in _refused(eng, N.FB_E_STATE, audio, m)
    _load(eng, small_system, "OSI")
    _same_attack(eng, nes_baseline)


# ------------------------------------------------------------------------------------- 6. nothing else moved
def test_attack_cw2_does_not_notice(eng, small_system):
    _load(eng, small_system, "OSI")
    audio = R.test_audio(4000)
    p = nes_params("OSI", "targeted", target=1, threshold=0.0, max_iter=6, samples_per_draw=0)
    q = cw2_params(search_steps=2, initial_const=1.0)
    before = eng.attack_cw2(p, q, audio)
    m = psy_params(*_theta(512, 4000), window=512, l2_weight=0.5)
    eng.attack_psy(p, q, m, audio)
    psy_route = eng.debug_wb_route()
    after = eng.attack_cw2(p, q, audio)
    for k in before:
        a, b = np.asarray(before[k]), np.asarray(after[k])
        assert np.array_equal(_bits(a), _bits(b)) if a.dtype == np.float64 else np.array_equal(a, b), k
    assert psy_route == dict(ctl=12, ctl_rep=0, backward=12, chain_t=0)          # one control launch and one backward per iteration


# ------------------------------------------------------------------------------------- 7. the surface
def test_imperceptible_returns_the_pair_and_checkpoint(small_system, tmp_path):
    from fakebob_amd.cw2 import snr_db
    from fakebob_amd.psy import Imperceptible
    from fakebob_amd.systems import gmm_SV
    ubm, spk = small_system
    model = gmm_SV(str(tmp_path / "sv"), ["spk0", "utt0", spk[0], 0.0, 1.0], ubm, pre_model_dir=str(tmp_path), threshold=0.0)
    audio = R.test_audio(4000)
    at = Imperceptible("SV", "targeted", model, window=512, l2_weight=0.25, binary_search_steps=2, max_iter=10, lr=2.0 ** -13,
                       initial_const=1e-2, verbose=False)
    cp = str(tmp_path / "psy.cp")
    res = at.attack(audio, cp, threshold=0.2)
    adv, flag = res
    assert adv.dtype == np.int16 and adv.shape == (4000, 1) and flag in (1, -1)
    with open(cp, "rb") as r:
        rows = pickle.load(r)
    assert len(rows) == 20 == int(res.rows_per_step.sum())
    for row in rows:
        assert len(row) == 4 and isinstance(row[0], float) and row[1].shape == (1,) and np.ndim(row[2]) == 0 and row[3] > 0
    theta, psd_max = M.masking_threshold(audio, float(model.engine.cfg.sample_freq), 512)
    got = model.engine.attack_psy(at._params(), at._cw2_params(), psy_params(theta, psd_max, 512, 0.25), audio)
    assert np.array_equal(got["adv"], adv[:, 0]) and got["success"] == flag and got["best_dist"] == res.best_dist
    assert got["best_l2"] == res.best_l2 and got["n_over"] == res.n_over and got["const"] == res.const
    a0 = C2.cast_i16(audio)
    assert np.array_equal(res.perturbation_i16, adv[:, 0].astype(np.int32) - a0) and res.snr_db == snr_db(a0, res.perturbation_i16)
    with pytest.raises(ValueError):
        Imperceptible("SV", "targeted", model, window=256)
    with pytest.raises(ValueError):
        Imperceptible("SV", "targeted", model, l2_weight=-1.0)


def test_attack_main_psy_on_the_synthetic_site(tmp_path, capsys):
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
                                "psy", "--psy-window", "512", "--psy-l2-weight", "0.1", "--cw2-steps", "2", "--cw2-const", "0.01",
                                "--cw2-lr", "0.0005", "--streams", "1", "--seed", "7"] + site
    np.random.seed(3)
    g, results, _thr = AM.main(argv)
    out = capsys.readouterr().out
    assert "load data done, total num: 12" in out and "attack successful rate" in out
    assert out.count("psy ") == 12 and out.count(" dB, c ") == 12 and "dist " in out and "over " in out
    assert g[1] == 12 and len(results) == 12 and g[2] >= 12 * 8
    n = 0
    for root, _dirs, files in os.walk(str(tmp_path / "out" / "checkpoint" / "gmm-OSI-targeted")):
        for f in files:
            with open(os.path.join(root, f), "rb") as r:
                rows = pickle.load(r)
            assert len(rows) == 8 and len(rows[0]) == 4
            n += 1
    assert n == 12
    for extra in (["--companions", "1"], ["--air-channel", "t60:200-600"], ["--feco", "0.5"], ["--dither", "1.0"], ["--eot-size", "2"],
                  ["--input-transform", "ms:7"], ["--codec", "ulaw"], ["-archi", "iv"], ["--psy-window", "256"],
                  ["--psy-l2-weight", "-1"]):
        with pytest.raises(SystemExit):
            AM.main(argv + extra)
    capsys.readouterr()
