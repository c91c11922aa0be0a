"""White-box gradients through the over-the-air channel on the device (fb_set_wb_air; "The over-the-air channel" in
include/fakebob_hip.h) against tests/air_vjp_ref.py, which tests/test_air_vjp_host.py pins to the adjoint identity and to the
mask rule.

Exact: k_air_conv_t on integer cotangents (every product and partial sum an integer below 2^53, so any summation order gives
the int64 correlation's bits), the rows the front end reads, the forward (fb_get_grad's bit for bit), determinism between
engines, a whole attack against its host replay.  Real-valued cotangents are held to the float64 summation bound of the
L + 15 terms the kernel adds, against a long double reference.  Two comparisons carry a relative L2 bar,
||g - g_ref|| / ||g_ref||:
  fb_debug_defence_vjp with a channel against autograd through the restatement   measured worst MEASURED_VJP,  bar BAR_VJP
  fb_get_grad_wb_iter through a channel against the restatement's loss gradient  measured worst MEASURED_GRAD, bar BAR_GRAD
Each bar is four times the worst error measured over the listed cases on the first run on an MI355X, rounded up to one
digit; none may exceed 1e-2."""
import numpy as np
import pytest

from fakebob_amd import _native as N
from fakebob_amd import input_transform as IT
from fakebob_amd.engine import Engine, nes_params
from fakebob_amd.models import synthetic_ivector_system
from tests import air_channel_ref as A
from tests import air_vjp_ref as AV
from tests import bpda_ref as B
from tests import whitebox_iv_ref as V
from tests import whitebox_ref as R
from tests.test_gpu_whitebox import Z_MEAN, Z_STD, _load, quantize, rel_l2

pytestmark = pytest.mark.gpu

MEASURED_VJP, BAR_VJP = 2.07e-16, 9e-16     # worst: channel + at:20 and channel + ulaw at r = 3; float64 throughout
MEASURED_GRAD, BAR_GRAD = 1.19e-5, 5e-5     # worst: OSI targeted, r = 1, epoch 0 (the GMM backward's float32 products: 2.5e-5 undefended)

SEED, STREAM = 77, 3
ROOM = "t60:100-200,drr:6,taps:256,delay:8"
REFUSAL = "white-box gradients: an air channel is set (fb_set_air_channel: clear it)"


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


def _clear(e):
    e.set_air_channel(None)
    e.set_input_transform(None)
    e.set_codec(None)
    e.set_eot(1)
    e.set_wb_bpda(False)
    e.set_wb_ivector(False)
    e.set_wb_air(False)


def _chain(spec):
    return [tuple(s) for s in IT.parse(spec)]


def _normals(e, chain, n, it, replica):
    """the normals the noise stages of `chain` draw for (SEED, STREAM, epoch it, utterance 0, replica): the generator's own hook"""
    return {s: e.debug_tf_noise(SEED, STREAM, it, 0, replica, s, 0, n) for s, st in enumerate(chain) if st[0] == B.NOISE}


def _taps(e, it, r):
    """the responses the forward draws for (SEED, STREAM, epoch it, utterance row 0, replica j), j < r"""
    return [e.debug_air_taps(SEED, STREAM, it, 0, j)[0] for j in range(r)]


# ------------------------------------------------------------------------------------- 1. the kernel alone, exact
def _chunk(e):
    return e.debug_air_conv_t_chunk()


# (L, n); "c+1" / "c-1": around the kernel's own chunk size
KERNEL_SHAPES = [(2, 17), (255, 4000), (256, 100), (4096, 5000), (2048, 9001), (512, "c+1"), (512, "c-1")]


def _int_case(L, n, seed, B_=1):
    rng = np.random.default_rng(seed)
    taps = rng.integers(-32768, 32768, (B_, L)).astype(np.int16)
    cot = rng.integers(-2 ** 20, 2 ** 20 + 1, (B_, n))
    return taps, cot


@pytest.mark.parametrize("L,n", KERNEL_SHAPES, ids=["%d-%s" % s for s in KERNEL_SHAPES])
def test_kernel_on_integer_cotangents_is_the_int64_correlation(eng, L, n):
    c = _chunk(eng)
    n = c + 1 if n == "c+1" else c - 1 if n == "c-1" else n
    taps, cot = _int_case(L, n, L + n)
    dx = eng.debug_air_conv_t(taps, cot.astype(np.float64))
    assert eng.debug_wb_air_route() == 1
    want = AV.conv_t(taps[0], cot[0], None, np.int64)
    assert dx.shape == (1, n) and np.array_equal(dx[0].view(np.uint64), want.view(np.uint64))


def test_three_rows_with_their_own_taps_in_one_launch(eng):
    c = _chunk(eng)
    taps, cot = _int_case(300, c + 37, 5, 3)
    dx = eng.debug_air_conv_t(taps, cot.astype(np.float64))
    assert eng.debug_wb_air_route() == 1
    for b in range(3):
        assert np.array_equal(dx[b], AV.conv_t(taps[b], cot[b], None, np.int64)), b
    assert not np.array_equal(dx[0], dx[1])


def test_a_unit_response_returns_the_cotangent(eng):
    """amp = 0: only t[0] = 16384"""
    taps = np.zeros((1, 256), np.int16)
    taps[0, 0] = 16384
    cot = np.random.default_rng(3).normal(size=(1, 4001))
    assert np.array_equal(eng.debug_air_conv_t(taps, cot), cot)


def test_masked_positions_contribute_exactly_nothing(eng):
    n = 4000
    t, x = AV.full_range_case(n)
    sat = AV.sat_mask(x, t)
    assert 0 < sat.sum() < n / 4                       # (on the twin, before the device is asked)
    _taps1, cot = _int_case(2, n, 9)
    dx = eng.debug_air_conv_t(t, cot.astype(np.float64), sat)
    assert np.array_equal(dx[0], AV.conv_t(t, cot[0], sat, np.int64))
    assert not np.array_equal(dx[0], AV.conv_t(t, cot[0], None, np.int64))
    other = cot.astype(np.float64)
    other[0, sat.astype(bool)] = 1e300                 # whatever stands at a masked position
    assert np.array_equal(eng.debug_air_conv_t(t, other, sat).view(np.uint64), dx.view(np.uint64))
    # the forward writes the same bytes: an all-ones cotangent through debug_defence_vjp counts the unsaturated neighbours
    try:
        eng.set_wb_air(True)
        eng.set_air_channel((2, 1, 0.0, 0.5, 0.5), validate=False)      # amp = 0: the unit response; the mask is all zero ...
        dwav, out = eng.debug_defence_vjp(x, np.ones((1, n)))
        assert np.array_equal(out[0], x) and np.array_equal(dwav[0], np.ones(n))   # ... 32767 is a legitimate unsaturated value
    finally:
        _clear(eng)


# ------------------------------------------------------------------------------------- 2. real-valued cotangents
@pytest.mark.parametrize("L,n", [(255, 4000), (4096, 5000), (2048, 9001)])
def test_kernel_on_real_cotangents_within_the_summation_bound(eng, L, n):
    rng = np.random.default_rng(L)
    taps = rng.integers(-32768, 32768, (1, L)).astype(np.int16)
    cot = rng.normal(size=(1, n)) * np.exp(rng.normal(size=(1, n)) * 3.0)       # several decades of magnitude
    dx = eng.debug_air_conv_t(taps, cot)[0]
    ref = AV.conv_t(taps[0], cot[0], None, np.longdouble)
    err = np.abs(dx.astype(np.longdouble) - ref).astype(np.float64)
    bound = AV.bound(taps[0], cot[0])
    print("L=%d n=%d: worst error / bound %.3g" % (L, n, float((err / np.maximum(bound, 1e-300)).max())))
    assert (err <= bound).all()


# ------------------------------------------------------------------------------------- 3. the hook through the channel
HOOK_SETTINGS = [("channel", None, None), ("channel+ms7-qt512", "ms:7,qt:512", None), ("channel+at20", "at:20", None),
                 ("channel+ulaw", None, "ulaw")]


@pytest.mark.parametrize("r", [1, 3])
@pytest.mark.parametrize("name,spec,codec", HOOK_SETTINGS, ids=[s[0] for s in HOOK_SETTINGS])
def test_defence_vjp_hook_through_the_channel(eng, name, spec, codec, r):
    n, it = 4000, 5
    wav = quantize(R.test_audio(n))
    chain = _chain(spec)
    cot = np.random.default_rng(n + len(name) + r).normal(size=(r, n))
    try:
        eng.set_air_channel(ROOM)
        eng.set_input_transform(spec)
        eng.set_codec(codec)
        eng.set_eot(r)
        with pytest.raises(N.NativeError) as ex:             # off: refused as documented
            eng.debug_defence_vjp(wav, cot, SEED, STREAM, it)
        assert ex.value.code == N.FB_E_STATE and REFUSAL in str(ex.value)
        eng.set_wb_air(True)
        dwav, out = eng.debug_defence_vjp(wav, cot, SEED, STREAM, it)
        launches, route = eng.debug_wb_air_route(), eng.debug_wb_route()
        taps = _taps(eng, it, r)
        worst = 0.0
        for j in range(r):
            want, ref_out = AV.defence_vjp(wav, taps[j], chain, codec, _normals(eng, chain, n, it, j), cot[j])
            assert np.array_equal(out[j], ref_out), "replica %d: the row the front end would read is not the twins'" % j
            assert np.isfinite(dwav[j]).all()
            worst = max(worst, rel_l2(dwav[j], want))
        eng.set_air_channel(None)
        eng.debug_defence_vjp(wav, cot, SEED, STREAM, it)
        without = eng.debug_wb_air_route()
    finally:
        _clear(eng)
    print("defence vjp %s r=%d: relative L2 error %.3g" % (name, r, worst))
    assert launches == 1 and without == 0
    assert route == dict(ctl=0, ctl_rep=0, backward=0, chain_t=r if chain else 0)
    if r > 1:
        assert not np.array_equal(out[0], out[1])
    assert worst < BAR_VJP


def test_defence_vjp_hook_with_saturated_outputs(eng):
    """full-range input: the forward's own saturation bytes, not the rails of its output, decide what passes"""
    n, it = 4000, 2
    _t, wav = AV.full_range_case(n)
    cot = np.random.default_rng(12).normal(size=(1, n))
    try:
        eng.set_air_channel(ROOM)
        eng.set_codec("ulaw")                                # wav_air is overwritten in place before the backward runs
        eng.set_wb_air(True)
        dwav, out = eng.debug_defence_vjp(wav, cot, SEED, STREAM, it)
        taps = _taps(eng, it, 1)[0]
    finally:
        _clear(eng)
    sat = AV.sat_mask(wav, taps)
    at_rail = np.abs(A.convolve(wav, taps).astype(np.int32)) >= 32767
    print("full range through the room: %d of %d outputs saturated, %d at a rail" % (int(sat.sum()), n, int(at_rail.sum())))
    assert 0 < sat.sum() < n
    want, ref_out = AV.defence_vjp(wav, taps, [], "ulaw", None, cot[0])
    assert np.array_equal(out[0], ref_out)
    assert rel_l2(dwav[0], want) < BAR_VJP
    assert rel_l2(dwav[0], AV.conv_t(taps, cot[0], None)) > 1e-3          # the mask mattered


# ------------------------------------------------------------------------------------- 4. the full gradient
BRANCHES = [("osi_targeted", "OSI", "targeted", dict(target=1, threshold=-10.0)),
            ("csi_untargeted", "CSI", "untargeted", dict(true=0))]


def _p(task, attack, kw, **more):
    return nes_params(task, attack, samples_per_draw=0, seed=SEED, stream=STREAM, **dict(kw, **more))


@pytest.mark.parametrize("it", [0, 5])
@pytest.mark.parametrize("r", [1, 3])
@pytest.mark.parametrize("bname,task,attack,kw", BRANCHES, ids=[b[0] for b in BRANCHES])
def test_get_grad_wb_through_the_channel(eng, small_system, bname, task, attack, kw, r, it):
    audio = R.test_audio(4000)
    models = _load(eng, small_system, task)
    zk = {} if task != "CSI" else dict(z_mean=Z_MEAN[:models[0].shape[0]], z_std=Z_STD[:models[0].shape[0]])
    p = _p(task, attack, kw)
    try:
        eng.set_air_channel(ROOM)
        eng.set_eot(r)
        eng.set_wb_bpda(r > 1)                               # the channel alone needs no other switch
        eng.set_wb_air(True)
        grad, al, sc = eng.get_grad_wb_iter(p, audio, it)
        launches, route = eng.debug_wb_air_route(), eng.debug_wb_route()
        _fl, _gg, al0, sc0 = eng.get_grad(p, audio, it=it, want_grad=False)
        ref = AV.loss_and_grad(eng.cfg, models, task, attack, audio, _taps(eng, it, r), **dict(kw, **zk))
    finally:
        _clear(eng)
    err = rel_l2(grad, ref.grad)
    print("%s r=%d it=%d: loss %.9g (restatement %.9g; per replica %s), min |c0 - thr| %.3g, relative L2 error %.3g"
          % (bname, r, it, al, ref.loss, ref.losses, ref.margin, err))
    assert al == al0 and np.array_equal(sc, sc0)                # the forward is fb_get_grad's, bit for bit
    assert launches == 1 and route == dict(ctl=1 if r == 1 else 0, ctl_rep=r if r > 1 else 0, backward=r, chain_t=0)
    assert ref.margin > 1e-3
    assert abs(al - ref.loss) < 1e-3 and np.abs(sc - ref.scores).max() < 1e-3
    assert np.isfinite(grad).all() and grad.any()
    assert err < BAR_GRAD


def test_get_grad_wb_through_channel_and_chain(eng, small_system):
    """channel, at:20 (the SNR power of replica j's own row) and mu-law behind it, r = 3"""
    audio, r, it, spec, codec = R.test_audio(4000), 3, 5, "at:20", "ulaw"
    models = _load(eng, small_system, "OSI")
    kw = dict(target=1, threshold=-10.0)
    chain = _chain(spec)
    try:
        eng.set_air_channel(ROOM)
        eng.set_input_transform(spec)
        eng.set_codec(codec)
        eng.set_eot(r)
        eng.set_wb_bpda(True)
        eng.set_wb_air(True)
        grad, al, sc = eng.get_grad_wb_iter(_p("OSI", "targeted", kw), audio, it)
        launches, route = eng.debug_wb_air_route(), eng.debug_wb_route()
        _fl, _gg, al0, sc0 = eng.get_grad(_p("OSI", "targeted", kw), audio, it=it, want_grad=False)
        nz = [_normals(eng, chain, audio.size, it, j) for j in range(r)]
        ref = AV.loss_and_grad(eng.cfg, models, "OSI", "targeted", audio, _taps(eng, it, r), chain, codec, nz, **kw)
    finally:
        _clear(eng)
    err = rel_l2(grad, ref.grad)
    print("channel + at:20 + ulaw r=3: loss %.9g (restatement %.9g), relative L2 error %.3g" % (al, ref.loss, err))
    assert al == al0 and np.array_equal(sc, sc0)
    assert launches == 1 and route == dict(ctl=0, ctl_rep=r, backward=r, chain_t=r)
    assert ref.margin > 1e-3 and abs(al - ref.loss) < 1e-3
    assert err < BAR_GRAD


def test_get_grad_wb_through_the_channel_on_an_ivector_system(eng):
    from tests.test_gpu_whitebox_iv import VAD_MARGIN, _assert_margins
    sy = synthetic_ivector_system(C=64, D=72, R=32, L=16, n_speakers=2, seed=4)
    tab = V.IvTables(sy)
    eng.load_ivector(sy, "OSI")
    audio, it = R.test_audio(4000), 5
    kw = dict(target=1, threshold=-10.0)
    p = _p("OSI", "targeted", kw)
    try:
        eng.set_air_channel(ROOM)
        eng.set_wb_ivector(True)
        eng.set_wb_air(True)
        grad, al, sc = eng.get_grad_wb_iter(p, audio, it)
        sel, _info = eng.debug_iv_gselect()
        launches, route = eng.debug_wb_air_route(), eng.debug_wb_route()
        _fl, _gg, al0, sc0 = eng.get_grad(p, audio, it=it, want_grad=False)
        taps = _taps(eng, it, 1)[0]
    finally:
        _clear(eng)
    assert al == al0 and np.array_equal(sc, sc0)
    assert launches == 1 and route["iv_post_t"] == 1 and route["chain_t"] == 0 and route["backward"] == 1
    wav = quantize(audio)
    out = A.convolve(wav, taps)
    r = V.loss_and_grad_iv(eng.cfg, tab, "OSI", "targeted", out.astype(np.float64) / 32768.0, sel=sel, **kw)
    _assert_margins(r, sel, "channel")
    assert r.margin > VAD_MARGIN
    want = AV.conv_t(taps, r.grad / 32768.0, AV.sat_mask(wav, taps)) * 32768.0     # the cotangent on the row the front end read
    err = rel_l2(grad, want)
    print("i-vector through the channel: loss %.9g (restatement %.9g), relative L2 error %.3g" % (al, r.loss, err))
    assert abs(al - r.loss) < 1e-3
    assert err < BAR_GRAD


def test_two_fresh_engines_give_equal_bits(small_system):
    audio = R.test_audio(4000)
    p = _p("OSI", "targeted", dict(target=1, threshold=-10.0))
    got = []
    for _ in range(2):
        e = Engine(0)
        try:
            _load(e, small_system, "OSI")
            e.set_air_channel(ROOM)
            e.set_input_transform("noise:40")
            e.set_eot(3)
            e.set_wb_bpda(True)
            e.set_wb_air(True)
            got.append(e.get_grad_wb_iter(p, audio, 2))
        finally:
            e.close()
    a, b = got
    assert np.array_equal(a[0].view(np.uint64), b[0].view(np.uint64)) and a[1] == b[1] and np.array_equal(a[2], b[2])


def test_the_draws_differ_between_epochs(eng, small_system):
    audio = R.test_audio(4000)
    _load(eng, small_system, "OSI")
    p = _p("OSI", "targeted", dict(target=1, threshold=-10.0))
    try:
        eng.set_air_channel(ROOM)
        eng.set_wb_air(True)
        g0, al0, _ = eng.get_grad_wb(p, audio)
        g0b, al0b, _ = eng.get_grad_wb_iter(p, audio, 0)
        g5, al5, _ = eng.get_grad_wb_iter(p, audio, 5)
    finally:
        _clear(eng)
    assert np.array_equal(g0, g0b) and al0 == al0b                    # fb_get_grad_wb is iter = 0
    assert al0 != al5 and not np.array_equal(g0, g5)


# ------------------------------------------------------------------------------------- 5. the switch
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
    assert eng.wb_air is False
    eng.set_wb_air(True)
    try:
        for bad in (2, -1):
            with pytest.raises(N.NativeError) as ex:
                eng.set_wb_air(bad)
            assert ex.value.code == N.FB_E_ARG and eng.wb_air is True     # the setting stays
    finally:
        eng.set_wb_air(False)


@pytest.mark.parametrize("other", ["none", "bpda", "ivector"])
def test_switch_off_refuses_as_before(eng, small_system, nes_baseline, other):
    """the very messages tests/test_gpu_bpda.py and tests/test_gpu_whitebox_iv.py assert, with their switches on"""
    if other == "ivector":
        eng.load_ivector(synthetic_ivector_system(C=64, D=72, R=32, L=16, n_speakers=2, seed=4), "OSI")
    else:
        _load(eng, small_system, "OSI")
    try:
        eng.set_wb_bpda(other == "bpda")
        eng.set_wb_ivector(other == "ivector")
        eng.set_air_channel(ROOM)
        msg = _refused(eng, R.test_audio(4000))
    finally:
        _clear(eng)
    assert "air channel" in msg and REFUSAL in msg
    _load(eng, small_system, "OSI")
    _same_attack(eng, nes_baseline)                     # off, an NES attack equals its baseline ...
    eng.set_wb_air(True)
    try:
        _same_attack(eng, nes_baseline)                 # ... and on as well: the switch is the white-box calls' alone
    finally:
        _clear(eng)


def test_on_without_a_channel_queues_the_same_launches(eng, small_system):
    audio = R.test_audio(4000)
    _load(eng, small_system, "OSI")
    p = nes_params("OSI", "targeted", target=1, threshold=0.0, max_iter=4)
    off = eng.get_grad_wb(p, audio)
    off_route, off_nes, off_air = eng.debug_wb_route(), eng.debug_nes_route(), eng.debug_wb_air_route()
    off_attack = eng.attack_wb(p, audio)
    off_attack_route = eng.debug_wb_route()
    try:
        eng.set_wb_air(True)
        on = eng.get_grad_wb(p, audio)
        on_route, on_nes, on_air = eng.debug_wb_route(), eng.debug_nes_route(), eng.debug_wb_air_route()
        on_attack = eng.attack_wb(p, audio)
        on_attack_route = eng.debug_wb_route()
    finally:
        _clear(eng)
    assert np.array_equal(off[0].view(np.uint64), on[0].view(np.uint64)) and off[1] == on[1] and np.array_equal(off[2], on[2])
    assert off_route == on_route == dict(ctl=1, ctl_rep=0, backward=1, chain_t=0) and off_nes == on_nes and off_air == on_air == 0
    assert off_attack_route == on_attack_route
    for x, y in zip(off_attack, on_attack):
        assert np.array_equal(x, y)


ON_CASES = {
    "companions": (lambda e: e.set_companions([R.test_audio(4000)]), lambda e: e.set_companions(None), "companions"),
    "feature_compression": (lambda e: e.set_feature_compression(0.5, 2), lambda e: e.set_feature_compression(None), "feature compression"),
    "dither": (lambda e: e.set_frontend(dither=1.0), lambda e: e.set_frontend(dither=0.0), "dither"),
    "eot_without_bpda": (lambda e: e.set_eot(2), lambda e: e.set_eot(1), "fb_set_eot"),
    "chain_without_bpda": (lambda e: e.set_input_transform("qt:64"), lambda e: e.set_input_transform(None), "input-transform"),
    "codec_without_bpda": (lambda e: e.set_codec("ulaw"), lambda e: e.set_codec(None), "codec"),
}


@pytest.mark.parametrize("case", sorted(ON_CASES))
def test_still_refused_with_the_switch_on(eng, small_system, case):
    on, off, word = ON_CASES[case]
    _load(eng, small_system, "OSI")
    try:
        eng.set_air_channel(ROOM)
        eng.set_wb_air(True)
        eng.set_wb_bpda(not case.endswith("without_bpda"))
        on(eng)
        assert word in _refused(eng, R.test_audio(4000))
    finally:
        off(eng)
        _clear(eng)


def test_an_ivector_system_under_eot_is_still_refused(eng, small_system):
    eng.load_ivector(synthetic_ivector_system(C=64, D=72, R=32, L=16, n_speakers=2, seed=4), "OSI")
    try:
        eng.set_air_channel(ROOM)
        eng.set_wb_air(True)
        msg = _refused(eng, R.test_audio(4000))                  # without fb_set_wb_ivector: an i-vector system
        assert "i-vector" in msg
        eng.set_wb_ivector(True)
        eng.set_wb_bpda(True)
        eng.set_eot(2)
        msg = _refused(eng, R.test_audio(4000))
        assert "i-vector" in msg and "fb_set_eot" in msg
    finally:
        _clear(eng)
        _load(eng, small_system, "OSI")


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
    # (adver_thresh keeps the mean loss above zero, so that all four iterations run)
    p = nes_params("OSI", "targeted", target=1, threshold=0.0, adver_thresh=50.0, max_iter=4, plateau_length=2, seed=SEED, stream=STREAM)
    monkeypatch.setenv("FB_ATTACK_BATCH", batch)
    try:
        eng.set_air_channel(ROOM)
        eng.set_eot(2)
        eng.set_wb_bpda(True)
        eng.set_wb_air(True)
        adv, flag, adv_f, trace = eng.attack_wb(p, audio)
        launches, route = eng.debug_wb_air_route(), eng.debug_wb_route()
        r_adv, r_flag, r_adv_f, r_trace = replay(eng, p, audio)
    finally:
        _clear(eng)
    print("batch %s: %d rows, flag %d, loss %s, lr %s" % (batch, trace.shape[0], flag, trace[:, 1], trace[:, 2]))
    assert launches == 4 and route == dict(ctl=0, ctl_rep=8, backward=8, chain_t=0)
    assert trace.shape == r_trace.shape == (4, 6) and np.array_equal(trace.view(np.uint64), r_trace.view(np.uint64))
    assert flag == r_flag and np.array_equal(adv_f.view(np.uint64), r_adv_f.view(np.uint64)) and np.array_equal(adv, r_adv)
    assert len(set(trace[:, 1])) == 4


# ------------------------------------------------------------------------------------- 7. it does what it is for
def test_the_adaptive_attack_wins_in_held_out_rooms(eng, small_system):
    """Thirty AdaptivePGD steps with air=True, eot_size=8 (epochs 0 .. 29 of the channel) against the same thirty steps on the
    no-channel gradient; both results scored through 16 held-out epochs of the channel (100 .. 115).  Both runs are
    deterministic; the two mean loss drops are in DESIGN.md section 6 and the README."""
    from fakebob_amd.pgd import AdaptivePGD
    _load(eng, small_system, "SV")
    audio = R.test_audio(4000)
    model = type("M", (), dict(task="SV", engine=eng))()
    score = nes_params("SV", "untargeted", threshold=1e3, samples_per_draw=0, seed=SEED, stream=STREAM)
    hp = dict(max_iter=30, seed=SEED, verbose=False)          # (threshold=1e3: never stops early)

    def held_out(a):
        return float(np.mean([eng.get_grad(score, a, it=it, want_grad=False)[2] for it in range(100, 116)]))
    try:
        plain_adv, _flag = AdaptivePGD("SV", "untargeted", model, bpda=False, **hp).attack(audio, None, threshold=1e3)
        eng.set_air_channel(ROOM)
        adaptive_adv, _flag = AdaptivePGD("SV", "untargeted", model, bpda=True, eot_size=8, air=True, **hp).attack(audio, None, threshold=1e3)
        launches = eng.debug_wb_air_route()
        eng.set_eot(1)
        clean = held_out(audio)
        plain = held_out(plain_adv[:, 0].astype(np.float64) / 32768.0)
        adaptive = held_out(adaptive_adv[:, 0].astype(np.float64) / 32768.0)
    finally:
        _clear(eng)
    print("held-out rooms, mean adver_loss: clean %.9g, after the no-channel attack %.9g (drop %.9g), after the adaptive attack %.9g "
          "(drop %.9g)" % (clean, plain, clean - plain, adaptive, clean - adaptive))
    assert launches == 30
    assert clean - adaptive > clean - plain
