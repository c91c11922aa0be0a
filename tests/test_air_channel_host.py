"""The over-the-air channel without a GPU: the numpy restatement of its contract (tests/air_channel_ref.py) against
np.convolve and against its own definitions, the spec parser with every refusal, the T60 / DRR conversions, the system
classes' keyword / FB_AIR_CHANNEL, --air-channel reaching make_model, and the library's new symbols."""
import inspect
import math

import numpy as np
import pytest

from fakebob_amd import _native, air_channel as A, systems
from tests import air_channel_ref as R


def _rng(seed):
    return np.random.default_rng(seed)


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("n,L", [(1, 2), (5, 17), (300, 64), (1000, 511), (700, 4096), (5000, 1000)])
def test_convolution_equals_numpy_convolve(n, L):
    g = _rng(n * 7 + L)
    x = g.integers(-32768, 32768, n).astype(np.int16)
    t = g.integers(-32767, 32768, L).astype(np.int16)
    t[0] = 16384
    full = np.convolve(x.astype(np.int64), t.astype(np.int64))[:n]          # truncated: the recording stops with the utterance
    assert full.dtype == np.int64 and np.array_equal(R.conv_sums(x, t), full)
    want = np.clip((full + 8192) >> 14, -32768, 32767).astype(np.int16)
    got = R.convolve(x, t)
    assert got.dtype == np.int16 and got.shape == x.shape and np.array_equal(got, want)


def test_the_shift_is_a_floor_and_the_clip_is_int16s():
    one = np.array([1], np.int16)
    for tap, want in ((8191, 0), (8192, 1), (-8192, 0), (-8193, -1), (-24577, -2), (24575, 1)):   # (y + 8192) >> 14
        assert R.convolve(one, np.array([tap, 0], np.int16))[0] == want, tap
    x = np.full(4, 32767, np.int16)
    assert np.array_equal(R.convolve(x, np.array([32767, 32767], np.int16)), [32767] * 4)
    assert np.array_equal(R.convolve(x, np.array([-32767, -32767], np.int16)), [-32768] * 4)


@pytest.mark.parametrize("rho", [1.0, 0.9999, 0.99928, 0.99, 0.5, 1e-3])
def test_envelope_is_its_definition_and_close_to_the_power(rho):
    e = R.envelope(rho, 4096)
    r = np.float64(rho)
    Q = [np.float64(1.0)]
    for _ in range(63):
        Q.append(Q[-1] * r)
    S = Q[63] * r
    P = [np.float64(1.0)]
    for _ in range(63):
        P.append(P[-1] * S)
    for m in range(4096):
        assert e[m] == P[m >> 6] * Q[m & 63], m
    exact = [math.exp(m * math.log(rho)) if rho < 1 else 1.0 for m in range(4096)]
    big = [m for m in range(4096) if exact[m] > 1e-300]                     # (below that the power itself is subnormal)
    rel = max(abs(float(e[m]) - exact[m]) / exact[m] for m in big)
    assert rel <= 1e-12, rel
    if rho == 1.0:
        assert np.all(e == 1.0)


def test_decay_stays_in_its_range():
    for w in (0, 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF):
        assert R.decay(w, 0.9991, 0.9991) == np.float64(0.9991)
        v = R.decay(w, 0.99, 0.9999)
        assert 0.99 <= v <= 0.9999
    assert R.decay(0, 0.5, 1.0) < R.decay(0xFFFFFFFF, 0.5, 1.0) <= 1.0
    U = (0x80000000 + 0.5) * 2.0 ** -32
    assert R.decay(0x80000000, 0.25, 0.75) == 0.25 + U * 0.5


def test_taps_layout():
    z = _rng(3).standard_normal(64).astype(np.float32)
    t = R.taps(64, 9, 2000.0, 0.97, 0.99, z, 12345)
    assert t.dtype == np.int16 and t[0] == 16384 and not t[1:9].any() and t[9:].any()
    e = R.envelope(R.decay(12345, 0.97, 0.99), 55)
    want = np.rint((np.float64(2000.0) * z[9:64].astype(np.float64)) * e)
    assert np.array_equal(t[9:], want.astype(np.int16))
    big = R.taps(64, 1, 16384.0, 1.0, 1.0, np.full(64, 5.0, np.float32), 0)
    small = R.taps(64, 1, 16384.0, 1.0, 1.0, np.full(64, -5.0, np.float32), 0)
    assert np.all(big[1:] == 32767) and np.all(small[1:] == -32767)          # the clip is symmetric: never -32768


def test_amp_zero_is_the_identity_for_full_scale_input():
    g = _rng(5)
    x = g.choice(np.array([-32768, 32767, 0, 1, -1], np.int16), 3000).astype(np.int16)
    z = g.standard_normal(2048).astype(np.float32)
    t = R.taps(2048, 32, 0.0, 0.999, 0.9995, z, 99)
    assert t[0] == 16384 and not t[1:].any()
    assert np.array_equal(R.convolve(x, t), x)
    assert np.array_equal(R.channel(np.zeros(100, np.int16), 2048, 32, 9000.0, 0.999, 0.9995, z, 99), np.zeros(100, np.int16))


def test_worst_case_stays_below_2_42():
    L = 4096
    x = np.full(2 * L, -32768, np.int16)
    for t in (np.full(L, 32767, np.int16), np.full(L, -32767, np.int16)):
        y = R.conv_sums(x, t)
        assert np.abs(y).max() == L * 32767 * 32768 < 2 ** 42
        assert np.array_equal(y.astype(np.float64).astype(np.int64), y)     # ... so float64 holds every partial sum exactly
    assert np.all(R.convolve(x, np.full(L, 32767, np.int16)) == -32768)
    assert np.all(R.convolve(x, np.full(L, -32767, np.int16)) == 32767)


def test_key_and_counter():
    assert R.AIRC == int.from_bytes(b"AIRC", "big")
    assert R.air_key(0x1122334455667788, 7) == (0x55667788 ^ R.AIRC, 0x11223344 ^ 7)
    assert R.air_counter(R.DECAY_C0, 5, 2, 9) == (0xFFFFFFFF, 5, 2, 9)
    assert R.air_counter(4095 >> 2, 0, 1, 3) == (1023, 0, 1, 3)


# ------------------------------------------------------------------------------------------- parser and conversions
def test_conversions():
    rho = A.rho_from_t60(300.0)
    assert rho == 10.0 ** (-3.0 / (300.0 * 16000 / 1000.0))
    assert abs(20.0 * math.log10(rho) * 4800 + 60.0) < 1e-9                  # 60 dB over 300 ms of samples
    assert A.rho_from_t60(300.0, fs=8000) == 10.0 ** (-3.0 / 2400.0)
    lo, hi = A.rho_from_t60(200.0), A.rho_from_t60(600.0)
    rm = 0.5 * (lo + hi)
    assert A.amp_from_drr(6.0, lo, hi) == 16384.0 * math.sqrt((1.0 - rm * rm) * 10.0 ** -0.6)
    assert A.amp_from_drr(-80.0, lo, hi) == 16384.0                          # the cap
    a = A.amp_from_drr(0.0, lo, lo)
    assert abs(a * a / (1.0 - lo * lo) - 16384.0 ** 2) < 1e-3 * 16384.0 ** 2  # the tail's energy equals the direct path's


def test_parser():
    ch = A.parse("t60:200-600,drr:6,taps:2048,delay:32")
    assert (ch.taps, ch.predelay) == (2048, 32)
    assert (ch.rho_lo, ch.rho_hi) == (A.rho_from_t60(200.0), A.rho_from_t60(600.0))
    assert ch.amp == A.amp_from_drr(6.0, ch.rho_lo, ch.rho_hi)
    assert A.parse("t60:300") == A.parse(" T60:300-300 , drr:6 , taps:2048, delay:32 ") == A.from_room(300.0)
    one = A.parse("t60:250,drr:-3.5,taps:4096,delay:4095")
    assert one.rho_lo == one.rho_hi and (one.taps, one.predelay) == (4096, 4095)
    assert A.parse("t60:1,taps:2,delay:1").taps == 2
    for none in (None, "", "none", "NONE", " off "):
        assert A.parse(none) is None
    assert A.parse(ch) is ch
    assert "taps=2048" in repr(ch) and ch != one


@pytest.mark.parametrize("bad", [
    "drr:6", "t60", "t60:", "t60:abc", "t60:0", "t60:-5", "t60:600-200", "t60:inf", "t60:nan", "t60:200-600-700",
    "t60:300,drr:nan", "t60:300,drr:inf", "t60:300,taps:1", "t60:300,taps:4097", "t60:300,taps:2.5", "t60:300,delay:0",
    "t60:300,taps:64,delay:64", "t60:300,delay:-1", "t60:300,t60:400", "t60:300,room:big", "t60:300;drr:6", "ms:7", 7, 3.5,
    ["t60:300"],
])
def test_parser_refusals(bad):
    with pytest.raises(ValueError):
        A.parse(bad)


@pytest.mark.parametrize("args", [
    (1, 1, 0.0, 0.5, 0.5), (4097, 1, 0.0, 0.5, 0.5), (8, 0, 0.0, 0.5, 0.5), (8, 8, 0.0, 0.5, 0.5), (8, 1, -1.0, 0.5, 0.5),
    (8, 1, 16384.5, 0.5, 0.5), (8, 1, float("nan"), 0.5, 0.5), (8, 1, float("inf"), 0.5, 0.5), (8, 1, 1.0, 0.0, 0.5),
    (8, 1, 1.0, -0.1, 0.5), (8, 1, 1.0, 0.6, 0.5), (8, 1, 1.0, 0.5, 1.5), (8, 1, 1.0, float("nan"), 0.5),
    (8, 1, 1.0, 0.5, float("nan")), (8, 1, 1.0, 0.5, float("inf")), (8.5, 1, 1.0, 0.5, 0.5),
    (float("inf"), 1, 1.0, 0.5, 0.5), (8, float("-inf"), 1.0, 0.5, 0.5), (float("nan"), 1, 1.0, 0.5, 0.5), ("8", 1, 1.0, 0.5, 0.5),
])
def test_object_refusals(args):
    with pytest.raises(ValueError):
        A.AirChannel(*args)


def test_object_limits_are_inclusive():
    A.AirChannel(2, 1, 0.0, 1.0, 1.0)
    A.AirChannel(4096, 4095, 16384.0, 1e-300, 1.0)


# ------------------------------------------------------------------------------------------------------ the surface
def test_system_keyword_and_environment(monkeypatch):
    class FakeEngine(object):
        got = "untouched"

        def set_air_channel(self, spec):
            self.got = A.parse(spec)
    monkeypatch.delenv("FB_AIR_CHANNEL", raising=False)
    e = FakeEngine()
    systems._apply_air_channel(e, None)
    assert e.got == "untouched"                                    # nobody asked: the engine keeps its setting
    systems._apply_air_channel(e, "t60:300")
    assert e.got == A.from_room(300.0)
    monkeypatch.setenv("FB_AIR_CHANNEL", "t60:200-400,taps:512")
    systems._apply_air_channel(e, None)
    assert e.got.taps == 512
    systems._apply_air_channel(e, "none")                          # the keyword wins over the environment
    assert e.got is None
    monkeypatch.setenv("FB_AIR_CHANNEL", "junk")
    with pytest.raises(ValueError):
        systems._apply_air_channel(e, None)
    for cls in (systems.gmm_OSI, systems.gmm_CSI, systems.gmm_SV, systems.iv_OSI, systems.iv_CSI, systems.iv_SV):
        assert "air_channel" in inspect.signature(cls.__init__).parameters, cls.__name__


def test_dropin_classes_inherit_the_keyword():
    from fakebob_amd.dropin import gmm_ubm_OSI, ivector_PLDA_SV
    assert "air_channel" in inspect.signature(gmm_ubm_OSI.gmm_OSI.__init__).parameters
    assert "air_channel" in inspect.signature(ivector_PLDA_SV.iv_SV.__init__).parameters


def test_air_channel_option_reaches_make_model(monkeypatch, tmp_path):
    from fakebob_amd import attack_main

    class Reached(Exception):
        pass
    seen = {}

    def fake_make_model(architecture, task, model_list, pre_model_dir, threshold, group_id, **kw):
        seen.update(kw)
        raise Reached()
    assert "air_channel" in inspect.signature(attack_main.make_model).parameters
    monkeypatch.setattr(attack_main, "make_model", fake_make_model)
    monkeypatch.setattr(attack_main, "load_spk_models", lambda *a, **k: [])
    with pytest.raises(Reached):
        attack_main.main(["-spk_id", "a", "--air-channel", "t60:200-600,drr:6", "--out_dir", str(tmp_path)])
    assert seen == {"air_channel": "t60:200-600,drr:6"}
    seen.clear()
    with pytest.raises(Reached):
        attack_main.main(["-spk_id", "a", "--out_dir", str(tmp_path)])
    assert "air_channel" not in seen                               # not named: make_model's own default


def test_library_symbols():
    for name in ("fb_set_air_channel", "fb_debug_air_taps", "fb_debug_air_convolve"):
        assert name in _native.EXPORTS
    assert [f[0] for f in _native.AirParams._fields_] == ["taps", "predelay", "amp", "rho_lo", "rho_hi"]
