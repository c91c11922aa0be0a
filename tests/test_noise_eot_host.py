"""The randomised stage and the EOT option on the host: builders, spec strings, the refusals that mirror the library's,
and the numpy restatement (tests/input_transform_noise_ref.py) against a direct Python loop."""
import math

import numpy as np
import pytest

from fakebob_amd import _native, input_transform as T
from fakebob_amd.systems import eot_option
from tests.input_transform_noise_ref import eot_mean, noise_scale, power, ref_noise_stage, ref_noisy


def test_abi_lists_the_new_entry_points():
    for name in ("fb_set_eot", "fb_debug_tf_noise", "fb_debug_input_transform_eot"):
        assert name in _native.EXPORTS
    assert _native.FB_TF_NOISE == T.NOISE == 4


def test_builders_and_spec_strings():
    (s,) = T.parse("at:20")
    assert (s.kind, s.k) == (T.NOISE, T.NOISE_SNR) and s.taps.dtype == np.float64 and s.taps[0] == 100.0
    assert T.at(13.0).taps[0] == 10.0 ** (13.0 / 10)
    (s,) = T.parse("noise:12.5")
    assert (s.kind, s.k, s.taps[0]) == (T.NOISE, T.NOISE_ABS, 12.5)
    assert T.radius(s) == 0
    chain = T.parse("ms:3,noise:4,as:5,qt:4")
    assert [c.kind for c in chain] == [T.MEDIAN, T.NOISE, T.FIR, T.QUANT]
    assert T.noise(0).taps[0] == 0.0 and T.noise(32768).taps[0] == 32768.0
    arr, keep = T.c_stages(T.parse("at:20"))
    assert (arr[0].kind, arr[0].k, arr[0].taps[0]) == (4, 1, 100.0)
    del keep


@pytest.mark.parametrize("bad", ["noise:-1", "noise:32769", "noise:nan", "at:inf", "at:nan", "at", "noise:1:2", "at:-inf"])
def test_host_refusals_of_spec_strings(bad):
    with pytest.raises(ValueError):
        T.parse(bad)


def test_host_refusals_of_hand_made_stages():
    for bad in (T.Stage(T.NOISE, 2, np.array([1.0])), T.Stage(T.NOISE, -1, np.array([1.0])), T.Stage(T.NOISE, 0, None),
                T.Stage(T.NOISE, 0, np.array([-0.5])), T.Stage(T.NOISE, 0, np.array([np.nan])),
                T.Stage(T.NOISE, 1, np.array([0.0])), T.Stage(T.NOISE, 1, np.array([np.inf])),
                T.Stage(T.NOISE, 1, np.array([-3.0])), T.Stage(T.NOISE, 0, np.array([1.0, 2.0]))):
        with pytest.raises(ValueError):
            T.validate([bad])
    assert len(T.validate([T.noise(3.0)] * 8)) == 8
    with pytest.raises(ValueError):
        T.validate([T.noise(3.0)] * 9)


def test_eot_option(monkeypatch):
    monkeypatch.delenv("FB_EOT_SIZE", raising=False)
    assert eot_option(None) is None and eot_option(4) == 4 and eot_option("1") == 1
    monkeypatch.setenv("FB_EOT_SIZE", "8")
    assert eot_option(None) == 8 and eot_option(2) == 2
    for bad in (0, 33, -1):
        with pytest.raises(ValueError):
            eot_option(bad)


def _loop(x, s, z):
    """y[i] = clip(rint(x[i] + s * z[i])) sample by sample in Python floats (IEEE double, round() ties to even)"""
    out = []
    for xi, zi in zip(x.tolist(), z.tolist()):
        v = float(xi) + float(s) * float(zi)
        out.append(max(-32768, min(32767, round(v))))
    return np.array(out, np.int16)


def test_restatement_against_a_python_loop():
    rng = np.random.default_rng(3)
    x = rng.integers(-2000, 2000, 50).astype(np.int16)
    z = rng.normal(size=50).astype(np.float32)
    # ties: s * z exactly k + 0.5 -> rint goes to the even neighbour, up and down
    x[:6] = [0, 1, 2, -1, -2, 7]
    z[:6] = [0.5, 0.5, 1.5, -0.5, -1.5, 2.5]
    # the clip at both ends of the scale
    x[6:10] = [32767, -32768, 32000, -32000]
    z[6:10] = [3.0, -3.0, 4000.0, -4000.0]
    y = ref_noise_stage(x, 0, 1.0, z, power(x))
    assert np.array_equal(y, _loop(x, 1.0, z))
    assert y[:6].tolist() == [0, 2, 4, -2, -4, 10]            # 0.5 -> 0, 1.5 -> 2, 3.5 -> 4, ..., 9.5 -> 10
    assert y[6:10].tolist() == [32767, -32768, 32767, -32768]
    s = 7.3
    assert np.array_equal(ref_noise_stage(x, 0, s, z, 0), _loop(x, s, z))
    # SNR mode: s from the exact power
    E = sum(int(v) ** 2 for v in x.tolist())
    assert power(x) == E
    rho = 10.0 ** (20 / 10)
    s_snr = math.sqrt(float(E) / 50.0 / rho)
    assert noise_scale(1, rho, E, 50) == s_snr
    assert np.array_equal(ref_noise_stage(x, 1, rho, z, E), _loop(x, s_snr, z))
    # a silent utterance: s = 0 and the output is the input
    zero = np.zeros(50, np.int16)
    assert np.array_equal(ref_noise_stage(zero, 1, rho, z, 0), zero)
    # in a chain E is the power of the CHAIN's input, not of the stage's
    chain = [T.quant(512), T.at(20)]
    got = ref_noisy(x, chain, {1: z})
    from tests.input_transform_ref import ref
    assert np.array_equal(got, _loop(ref(x, chain[:1]), s_snr, z))


def test_eot_mean_order():
    v = np.array([[0.1, 0.2, 0.3], [1e16, 1.0, -1e16]])
    assert eot_mean(v)[0] == ((0.1 + 0.2) + 0.3) / 3.0
    assert eot_mean(v)[1] == ((1e16 + 1.0) + -1e16) / 3.0
    assert np.array_equal(eot_mean(np.full((5, 4), 0.3)), np.full(5, 0.3))     # r = 4 of equal values: exact
