"""Companion utterances without a GPU: the numpy restatement against hand-worked cases (both rails), the Python argument
handling (unequal lengths refused, None clears), apply_perturbation, the driver's crop rule and choice of companions, and
the presence of the new symbols."""
import os
import re

import numpy as np
import pytest

from fakebob_amd import _native, companions as CP
from tests import companions_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def i16(*v):
    return np.array(v, np.int16)


# ------------------------------------------------------------------------------------------------ the restatement
def test_composition_by_hand():
    q = i16(110, -32768, 5, 32767, -3)
    a0 = i16(100, -32760, 5, 32760, 0)          # the difference: +10, -8, 0, +7, -3
    comp = np.stack([i16(32767, -32768, -7, 32761, 2), i16(0, 0, 0, 0, 0)])
    w = R.compose_row(q, a0, comp)
    assert w.shape == (3, 5)
    assert np.array_equal(w[0], q)                                         # utterance 0 is q itself
    assert np.array_equal(w[1], i16(32767, -32768, -7, 32767, -1))        # 32777 -> 32767, -32776 -> -32768, 32768 -> 32767
    assert np.array_equal(w[2], i16(10, -8, 0, 7, -3))                    # on silence: the perturbation itself


def test_the_difference_is_int32_not_int16():
    """q - a0 spans [-65535, 65535]: a 16-bit difference would wrap"""
    w = R.compose_row(i16(32767, -32768), i16(-32768, 32767), np.stack([i16(-32768, 32767), i16(0, 0)]))
    assert np.array_equal(w[1], i16(32767, -32768))      # -32768 + 65535 = 32767; 32767 - 65535 = -32768: exact, no clip
    assert np.array_equal(w[2], i16(32767, -32768))      # 65535 -> 32767, -65535 -> -32768


def test_row_order_and_the_chain():
    """[b][u][j] of the restatement: the chain acts on the composed, clipped samples (qt:4 after the clip)"""
    q = np.stack([i16(10, 20, 30), i16(11, 19, 32760)])
    a0 = i16(10, 20, 30)
    comp = np.stack([i16(100, 200, 300)])
    out = R.compose(q, a0, comp, [(0, 4, None)], 2)
    assert out.shape == (2, 2, 2, 3)
    assert np.array_equal(out[0, 0, 0], i16(12, 20, 32)) and np.array_equal(out[0, 0, 1], out[0, 0, 0])
    assert np.array_equal(out[0, 1, 0], i16(100, 200, 300))
    assert np.array_equal(out[1, 1, 1], i16(100, 200, 32767))      # 301, 199, 33030 -> clip 32767 -> qt:4 -> 32768 -> clip
    flat = out.reshape(-1, 3)
    assert np.array_equal(flat[1 * 4 + 1 * 2 + 0], out[1, 1, 0])   # row b * K * r + u * r + j


def test_noise_draws_by_replica_and_scales_by_the_composed_row():
    seen = []

    def normals(b, rho, s):
        seen.append((b, rho, s))
        return np.full(4, 1.0, np.float32)
    q = np.stack([i16(100, 100, 100, 100)])
    comp = np.stack([i16(300, 300, 300, 300)])
    out = R.compose(q, i16(100, 100, 100, 100), comp, [(4, 1, np.array([1.0]))], 2, normals)   # SNR 0 dB: s = rms of the row
    assert seen == [(0, 0, 0), (0, 1, 0), (0, 2, 0), (0, 3, 0)]
    assert np.array_equal(out[0, 0, 0], i16(200, 200, 200, 200)) and np.array_equal(out[0, 1, 1], i16(600, 600, 600, 600))


def test_the_mean_of_two_equal_values_is_exact_and_three_are_not_always():
    v = np.array([0.1, 0.1])
    assert R.mean_over_replicas(v) == 0.1
    acc = (np.float64(0.1) + np.float64(0.1) + np.float64(0.1)) / np.float64(3.0)
    assert R.mean_over_replicas(np.array([0.1, 0.1, 0.1])) == acc
    m = R.mean_over_replicas(np.array([[1.0, 2.0, 4.0], [1e16, 1.0, -1e16]]))
    assert np.array_equal(m, [7.0 / 3.0, 0.0])                     # rho ascending: 1e16 + 1 rounds the 1 away


# ------------------------------------------------------------------------------------------------ the host helpers
def test_cast_rule():
    x = np.array([0.0, 0.5, -0.5, 1.0, -1.0, 0.99999, -3.05e-5, 3.05e-5, 1.5])
    want = (x * 32768.0).astype(np.int64).astype(np.int16)         # truncation, then the low 16 bits
    assert np.array_equal(CP.cast_i16(x), want)
    assert CP.cast_i16(np.array([1.0]))[0] == -32768
    assert np.array_equal(CP.cast_i16(np.array([0.5, -0.26]), 8), i16(64, -33))
    k = i16(1, -2, 3)
    assert np.array_equal(CP.cast_i16(k), k)


def test_argument_handling():
    assert CP.as_companions(None) is None and CP.as_companions([]) is None
    a = CP.as_companions([np.zeros(7), i16(1, 2, 3, 4, 5, 6, 7)], 7)
    assert a.dtype == np.int16 and a.shape == (2, 7) and a.flags.c_contiguous
    assert CP.as_companions(i16(1, 2, 3)).shape == (1, 3)
    with pytest.raises(ValueError, match="lengths"):
        CP.as_companions([np.zeros(7), np.zeros(8)])
    with pytest.raises(ValueError, match="7 samples"):            # equal among themselves, not to the attacked utterance
        CP.as_companions([np.zeros(8), np.zeros(8)], 7)
    with pytest.raises(ValueError, match="at most 31"):
        CP.as_companions([np.zeros(4)] * 32)
    with pytest.raises(ValueError):
        CP.as_companions([np.zeros(0)])


def test_apply_perturbation_is_the_contracts_clip_add():
    d = np.array([10, -8, 0, 65535, -65535], np.int32)
    out = CP.apply_perturbation(d, [i16(32767, -32768, -7, -32768, 32767), np.array([0.0, 0.0, 0.5, 0.0, 0.0])])
    assert [o.dtype for o in out] == [np.int16, np.int16]
    assert np.array_equal(out[0], i16(32767, -32768, -7, 32767, -32768))
    assert np.array_equal(out[1], i16(10, -8, 16384, 32767, -32768))
    q, a0 = i16(110, -32768, 5), i16(100, -32760, 5)
    comp = np.stack([i16(32767, -32768, -7)])
    assert np.array_equal(CP.apply_perturbation(q.astype(np.int32) - a0, list(comp))[0], R.compose_row(q, a0, comp)[1])
    assert np.array_equal(CP.compose(q, a0, comp[0]), R.compose_row(q, a0, comp)[1])
    with pytest.raises(ValueError):
        CP.apply_perturbation(d, [i16(1, 2)])


def test_attack_result_unpacks_as_the_references_pair():
    adv = i16(1, 2, 3).reshape(-1, 1)
    res = CP.AttackResult(adv, -1, np.array([1, 0, -1], np.int32))
    a, flag = res
    assert a is adv and flag == -1 and len(res) == 2 and res.per_utterance is None
    assert np.array_equal(res.apply_perturbation(i16(32767, 0, -32768))[0], i16(32767, 0, -32768))


def test_success_rule():
    assert CP.succeeded("OSI", "targeted", 2, target=2) and not CP.succeeded("OSI", "targeted", -1, target=2)
    assert CP.succeeded("OSI", "untargeted", 0) and not CP.succeeded("OSI", "untargeted", -1)
    assert CP.succeeded("CSI", "untargeted", 1, true=0) and not CP.succeeded("CSI", "untargeted", 0, true=0)
    assert CP.succeeded("SV", "targeted", 1) and not CP.succeeded("SV", "targeted", -1)


# ------------------------------------------------------------------------------------------------ the driver
def _items():
    mk = lambda spk, name, n: dict(spk=spk, name=name, audio=np.full(n, 0.25))   # noqa: E731
    return [mk("a", "a1.wav", 9), mk("a", "a1.wav", 9), mk("a", "a2.wav", 7), mk("b", "b1.wav", 5), mk("a", "a3.wav", 8)]


def test_the_driver_picks_the_next_utterances_of_the_speaker():
    it = _items()
    assert CP.pick_companions(it, 0, 2) == [2, 4]          # the duplicate of a targeted job and speaker b are skipped
    assert CP.pick_companions(it, 4, 2) == [0, 2]          # wrapping around
    assert CP.pick_companions(it, 2, 5) == [4, 0]          # fewer than asked for: what there is
    assert CP.pick_companions(it, 3, 2) == []


def test_the_drivers_crop_rule_is_printed(capsys):
    from fakebob_amd.attack_main import with_companions
    audio, comp = with_companions(_items(), 0, 2)
    assert audio.size == 7 and [c.size for c in comp] == [7, 7]
    msg = capsys.readouterr().out
    assert "7 samples each" in msg and "a1.wav cropped from 9" in msg and "a3.wav cropped from 8" in msg and "a2.wav cropped" not in msg
    wavs, n = CP.crop_to_shortest([np.arange(5), np.arange(3), np.arange(4)])
    assert n == 3 and all(np.array_equal(w, np.arange(3)) for w in wavs)      # the FIRST n samples


# ------------------------------------------------------------------------------------------------ the symbols
def test_new_symbols_are_declared_and_bound():
    pub = open(os.path.join(ROOT, "include", "fakebob_hip.h")).read()
    tst = open(os.path.join(ROOT, "include", "fakebob_hip_test.h")).read()
    assert re.search(r"int fb_set_companions\(fb_engine \*e, const int16_t \*wav, int K1, int64_t N\);", pub)
    assert re.search(r"int fb_debug_compose\(fb_engine \*e, const int16_t \*q, int B, int64_t N,", tst)
    assert "MEAN, NOT A MAXIMUM" in pub
    assert "fb_set_companions" in _native.EXPORTS and "fb_debug_compose" in _native.EXPORTS
    src = open(os.path.join(ROOT, "fakebob_amd", "csrc", "input_transform_kernel.hip")).read()
    assert "k_input_transform_cmp" in src and "k_tf_power_cmp" in src
    from fakebob_amd.engine import Engine
    from fakebob_amd.attack import FakeBob
    import inspect
    assert callable(Engine.set_companions) and callable(Engine.debug_compose)
    assert "companions" in inspect.signature(FakeBob.attack).parameters
    from fakebob_amd import systems
    for cls in ("gmm_OSI", "gmm_CSI", "gmm_SV", "iv_OSI", "iv_CSI", "iv_SV"):
        assert "companions" in inspect.signature(getattr(systems, cls).__init__).parameters, cls
