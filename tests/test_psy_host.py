"""The host side of the masking attack (include/fakebob_hip.h, "masking"): fakebob_amd/masking.py against its independent
restatement (tests/psy_ref.py), the properties of the threshold, the framing, and the PyTorch reference of the loss against
itself and against central differences.  No GPU.

Bars, each from the references' own error:
  theta, masking.py against the restatement            measured worst 3.2e-13 relative, bar BAR_THETA = 2e-12.  Both are float64;
      they differ in the transform (numpy's rfft against an explicit DFT matrix), which leaves the weakest bin of p known to
      1.5e-13 relative (measured, SELF_P_BIN), and a masker spreads upwards as p^(1 + 0.37 dz): over the upper Bark range that
      is about the tenth power, so ten times the transform's error, rounded up.
  the loss reference, torch.fft.rfft against the explicit DFT, on the shapes of tests/test_gpu_psy.py
      gd: worst 5.6e-16 of max |gd| (SELF_GD = 6e-16); D: 2.7e-16 relative (SELF_D = 3e-16); P: 1.5e-15 of max P (SELF_P = 1.5e-15).
      The device is given 64 times these in tests/test_gpu_psy.py; here they are pinned.
"""
import numpy as np
import pytest

from fakebob_amd import masking as M
from fakebob_amd.models import synthetic_audio
from tests import psy_ref as PR

BAR_THETA = 2e-12
SELF_GD, SELF_D, SELF_P = 6e-16, 3e-16, 1.5e-15
GPU_SHAPES = [(512, 512), (512, 513), (512, 4000), (1024, 1024 + 256 + 1), (2048, 2048), (2048, 2048 + 3 * 512 + 5)]
FS = 16000


def noise(n, amp_lsb):
    return np.random.default_rng(1).normal(0.0, amp_lsb / 32768.0, n)


@pytest.mark.parametrize("W,N", [(512, 4000), (1024, 1024 + 256 + 1), (2048, 2048 + 3 * 512 + 5)])
def test_masking_equals_its_restatement(W, N):
    a0 = synthetic_audio(0, N)
    theta, psd_max = M.masking_threshold(a0, FS, W)
    ref, ref_max, maskers = PR.threshold_ref(a0, FS, W)
    err = float(np.max(np.abs(theta - ref) / ref))
    print("W=%d N=%d: theta relative error %.3g, psd_max %.3g, maskers per frame %d .. %d, theta %.3g .. %.3g" %
          (W, N, err, abs(psd_max - ref_max) / ref_max, min(map(len, maskers)), max(map(len, maskers)), theta.min(), theta.max()))
    assert theta.shape == ref.shape == (M.n_frames(N, W), W // 2 + 1) and theta.dtype == np.float64
    assert abs(psd_max - ref_max) <= 4e-16 * ref_max * np.log2(W)
    assert err <= BAR_THETA
    # the maskers themselves: the same bins, frame by frame
    p = M.frame_power(a0, W)
    psd = 96.0 + 10.0 * np.log10(p / psd_max + 1e-20)
    ath, z = M.threshold_in_quiet(FS, W)
    for f in range(p.shape[0]):
        bins, _levels = M.frame_maskers(psd[f], ath, z)
        assert list(bins) == [k for k, _l in maskers[f]], f


def test_theta_is_at_least_the_threshold_in_quiet():
    for W in M.WINDOWS:
        a0 = synthetic_audio(0, W + 700)
        theta, _pm = M.masking_threshold(a0, FS, W)
        ath, z = M.threshold_in_quiet(FS, W)
        quiet = 10.0 ** (ath / 10.0)
        assert (quiet[z <= 1.0] == 0.0).all() and np.isfinite(theta).all() and (theta > 0.0).all()
        assert (theta >= quiet[None, :]).all()


@pytest.mark.parametrize("W", [512, 2048])
def test_a_tone_has_one_masker_at_its_bin(W):
    """A 1 kHz tone on a bin centre: above 1 Bark every frame keeps one masker, the tone's.  Below 1 Bark the contract has no
    threshold in quiet (ATH = -inf), so step 3 drops nothing there, and the strict-maximum test of step 1 finds peaks in the
    rounding noise of the transform on the 1e-20 floor of the PSD (-104 dB): frames whose tone is not cut by the zero extension
    keep one or two of them at L = -99.2 dB, 197 dB under the tone.  They are the contract's, not an error of either
    implementation (both find the same ones); what they add to theta is asserted to be nothing."""
    hop = W // 4
    N = W + 5 * hop + 7
    tone = 0.5 * np.sin(2.0 * np.pi * 1000.0 * np.arange(N) / FS)
    kt = 1000 * W // FS
    theta, psd_max = M.masking_threshold(tone, FS, W)
    p = M.frame_power(tone, W)
    psd = 96.0 + 10.0 * np.log10(p / psd_max + 1e-20)
    ath, z = M.threshold_in_quiet(FS, W)
    _t, _m, maskers = PR.threshold_ref(tone, FS, W)
    for f in range(p.shape[0]):
        bins, levels = M.frame_maskers(psd[f], ath, z)
        assert list(bins) == [k for k, _l in maskers[f]]
        above = [(int(k), float(l)) for k, l in zip(bins, levels) if z[k] > 1.0]
        assert len(above) == 1 and above[0][0] == kt and above[0][1] > 90.0, (f, above)
        floor = [(int(k), float(l)) for k, l in zip(bins, levels) if z[k] <= 1.0]
        assert all(l < -99.0 for _k, l in floor), (f, floor)
        only = M.spread(np.array([kt]), np.array([above[0][1]]), z) + 10.0 ** (ath / 10.0)
        # (a floor masker's own power is 10^((-99.2 - 6.025) / 10) = 3e-11 at its bin and less elsewhere; at most two are kept)
        assert len(floor) <= 2 and (np.abs(theta[f] - only) <= 2 * 10.0 ** -10.5 + 1e-14 * only).all()


def test_theta_does_not_depend_on_the_level():
    a0 = synthetic_audio(0, 4000)
    theta, pm = M.masking_threshold(a0, FS, 512)
    half, pm_half = M.masking_threshold(0.5 * a0, FS, 512)       # a power of two: every p scales exactly
    assert np.array_equal(half, theta) and pm_half == 0.25 * pm
    third, pm_third = M.masking_threshold(0.3 * a0, FS, 512)
    assert np.max(np.abs(third - theta) / theta) <= BAR_THETA and abs(pm_third - 0.09 * pm) <= 1e-14 * pm


def test_frame_counts_and_refusals():
    for W in M.WINDOWS:
        hop = W // 4
        assert [M.n_frames(n, W) for n in (W, W + 1, W + hop, W + hop + 1)] == [1, 2, 2, 3]
        assert [PR.frames_of(n, W) for n in (W, W + 1, W + hop, W + hop + 1)] == [1, 2, 2, 3]
        for n in (W, W + 1, W + hop, W + hop + 1):
            assert M.frame_power(np.ones(n), W).shape == (M.n_frames(n, W), W // 2 + 1)
            assert (M.n_frames(n, W) - 1) * hop + W >= n > (M.n_frames(n, W) - 2) * hop + W or n == W
        with pytest.raises(ValueError):
            M.n_frames(W - 1, W)
    with pytest.raises(ValueError):
        M.n_frames(4000, 256)
    with pytest.raises(ValueError):
        M.masking_threshold(np.zeros(4000), FS, 512)


def test_host_loss_is_the_reference():
    a0 = synthetic_audio(0, 4000)
    theta, pm = M.masking_threshold(a0, FS, 512)
    d = noise(4000, 64)
    ref = PR.loss(d, theta, pm, 512)
    D, n_over, P = M.masking_loss(d, theta, pm, 512)
    assert n_over == ref["n_over"] > 0 and abs(D - ref["D"]) <= 64 * SELF_D * ref["D"]
    assert np.abs(P - ref["P"]).max() <= 64 * SELF_P * ref["P"].max()


@pytest.mark.parametrize("W,N", GPU_SHAPES)
def test_the_reference_against_itself(W, N):
    """torch.fft.rfft against the explicit DFT matrix: the reference's own error, and the margin condition of the GPU test"""
    a0 = synthetic_audio(0, N)
    theta, pm = M.masking_threshold(a0, FS, W)
    for amp in (1, 8, 64):
        d = noise(N, amp)
        a, b = PR.loss(d, theta, pm, W), PR.loss(d, theta, pm, W, dft=True)
        eg = float(np.abs(a["gd"] - b["gd"]).max() / max(np.abs(a["gd"]).max(), 1e-300))
        eD = abs(a["D"] - b["D"]) / max(a["D"], 1e-300)
        eP = float(np.abs(a["P"] - b["P"]).max() / a["P"].max())
        print("W=%d N=%d amp=%d: D %.6g n_over %d margin %.3g; self error gd %.3g D %.3g P %.3g" %
              (W, N, amp, a["D"], a["n_over"], a["margin"], eg, eD, eP))
        assert a["margin"] > 1e-9 and a["n_over"] == b["n_over"]
        assert eg <= SELF_GD and eD <= SELF_D and eP <= SELF_P
        if amp == 1:
            assert a["D"] == 0.0 and a["n_over"] == 0 and not a["gd"].any()


def test_autograd_agrees_with_central_differences():
    """D is piecewise quadratic in delta: away from a kink the central difference is exact up to the rounding of D itself,
    about sqrt(F K) eps D in each of the two evaluations, divided by 2h: the bar is 32 eps D / h (F K = 1028 here)."""
    W, N, h = 512, 1000, 1e-6
    a0 = synthetic_audio(0, N)
    theta, pm = M.masking_threshold(a0, FS, W)
    d = noise(N, 64)
    ref = PR.loss(d, theta, pm, W)
    assert ref["D"] > 0.0
    bar = 32.0 * np.finfo(np.float64).eps * ref["D"] / h
    worst = 0.0
    for i in np.random.default_rng(2).integers(0, N, 12):
        e = np.zeros(N)
        e[i] = h
        up, dn = PR.loss(d + e, theta, pm, W), PR.loss(d - e, theta, pm, W)
        assert up["n_over"] == dn["n_over"] == ref["n_over"]       # no bin crosses its threshold between the two
        worst = max(worst, abs((up["D"] - dn["D"]) / (2.0 * h) - ref["gd"][i]))
    print("central differences: worst %.3g, bar %.3g, max |gd| %.3g" % (worst, bar, np.abs(ref["gd"]).max()))
    assert worst <= bar and bar < 1e-8 * np.abs(ref["gd"]).max()
