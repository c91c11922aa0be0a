"""k_update_perturb / k_update_perturb_x with 256 and with 512 threads per workgroup of 256 samples (FB_UP_THREADS; on a GPU
shared by three or more attacks the engine chooses 256, a lone attack 512): the same arithmetic in the same order, so the
trace, the float64 adversarial audio and the int16 audio of an attack are equal bit for bit.

System: a tiny GMM (C = 64, D = 72, UBM + 2 speakers); six iterations with the early stop out of reach (adver_thresh = 1e3),
on the unfused chain (fb_set_fused_chain(e, 0)).  Cases:
  - N = 4000 (a partial last workgroup), 4095, 4096 (a full one), 4097 (a workgroup that holds one sample), 16001; 4095, 4097
    and 16001 are no multiple of 4 (scalar stores of the columns);
  - samples_per_draw = 2 (half = 1), 10 (64 * 5 items do not divide over 256 or 512 threads evenly), 50 (the recipe), 80
    (FB_FUSE_MAX_HALF);
  - bits_per_sample = 8 next to the default 16;
  - a float32 and a float64 model on the same GPU (fb_attack_dev, k_update_perturb_x; tests/foreign_models.py);
  - the 256-thread run against the fused chain (fb_set_fused_chain(e, 1), k_gmm_finalize_loss_update).
Every case asserts the shape it ran (Engine.debug_launch_shape()["up_threads"]) and the route (Engine.debug_nes_route)."""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")   # ahead of the library: the model on the GPU and the engine share one HIP runtime

from fakebob_amd.engine import Engine, nes_params  # noqa: E402
from fakebob_amd.models import synthetic_audio, synthetic_gmm_system  # noqa: E402
from tests.foreign_models import FrameModel  # noqa: E402

pytestmark = pytest.mark.gpu
ITERS = 6
KW = dict(epsilon=0.002, sigma=0.001, max_lr=0.001, min_lr=1e-6, momentum=0.9, plateau_length=2, plateau_drop=2.0,
          adver_thresh=1e3, target=0, threshold=0.2277)


@pytest.fixture(autouse=True)
def _clean_knobs(monkeypatch):
    for k in ("FB_UP_THREADS", "FB_FUSE_PARTS", "FB_NO_FUSE", "FB_FUSE_UPD", "FB_GMM_SUB", "FB_MFCC_CUS"):
        monkeypatch.delenv(k, raising=False)


@pytest.fixture(scope="module")
def engine():
    ubm, spk = synthetic_gmm_system(n_speakers=2, C=64, D=72)
    e = Engine(0)
    e.load_gmm([ubm] + spk)
    e.set_system("OSI")
    yield e
    e.close()


def _run(e, n, spd, threads, fused=False, bits=16):
    """One attack -> (int16 adv, flag, float64 adv, trace), the launch shape and the route it reports."""
    if threads is None:
        os.environ.pop("FB_UP_THREADS", None)
    else:
        os.environ["FB_UP_THREADS"] = str(threads)
    try:
        e.set_fused_chain(fused)
        p = nes_params("OSI", "targeted", samples_per_draw=spd, max_iter=ITERS, seed=42, stream=1, bits_per_sample=bits, **KW)
        res = e.attack(p, synthetic_audio(3, n))
        return res, e.debug_launch_shape(), e.debug_nes_route()
    finally:
        os.environ.pop("FB_UP_THREADS", None)


def _assert_same(a, b, label):
    (adv_a, flag_a, advf_a, tr_a), (adv_b, flag_b, advf_b, tr_b) = a, b
    assert flag_a == flag_b, label
    assert tr_a.shape == tr_b.shape and tr_a.shape[0] == ITERS, (label, tr_a.shape, tr_b.shape)
    assert np.array_equal(tr_a.view(np.uint64), tr_b.view(np.uint64)), label
    assert np.array_equal(advf_a.view(np.uint64), advf_b.view(np.uint64)), label
    assert np.array_equal(adv_a, adv_b), label


def _both(e, n, spd, bits=16):
    out = {}
    for t in (256, 512):
        res, sh, route = _run(e, n, spd, t, bits=bits)
        assert sh["up_threads"] == t, (t, sh)
        # the batch of iteration it + 1 rides in the update launch of iteration it: one k_update_perturb per iteration
        assert route["k_update_perturb"] == ITERS and route["k_loss"] == ITERS and route["fin_loss_update"] == 0, route
        out[t] = res
    _assert_same(out[256], out[512], (n, spd, bits))
    moved = np.abs(out[256][2] - synthetic_audio(3, n)).max()
    assert 0.0 < moved <= KW["epsilon"] + 1e-12, moved   # the attack did step, inside its ball
    return out[256]


@pytest.mark.parametrize("n", [4000, 4095, 4096, 4097, 16001])
def test_thread_counts_agree_over_sample_counts(engine, n):
    _both(engine, n, 50)


@pytest.mark.parametrize("spd", [2, 10, 80])
def test_thread_counts_agree_over_samples_per_draw(engine, spd):
    _both(engine, 4097, spd)


def test_thread_counts_agree_at_eight_bits(engine):
    r8 = _both(engine, 4097, 50, bits=8)
    r16 = _both(engine, 4097, 50, bits=16)
    assert not np.array_equal(r8[0], r16[0])   # the narrower cast is a different attack


def test_shared_chain_chooses_256_and_equals_the_fused_chain(engine):
    """Without the override the unfused chain launches 256 threads, and its attack is the fused chain's bit for bit (there the
    update rides in k_gmm_finalize_loss_update's 512-thread workgroups)."""
    for n, spd in ((4097, 50), (16001, 10)):
        shared, sh, route = _run(engine, n, spd, None, fused=False)
        assert sh["up_threads"] == 256 and route["k_update_perturb"] == ITERS, (sh, route)
        forced, sh, _ = _run(engine, n, spd, 256, fused=False)
        assert sh["up_threads"] == 256, sh
        fused, sh, route = _run(engine, n, spd, None, fused=True)
        assert sh["up_threads"] == 512, sh
        assert route["fin_loss_update"] == ITERS and route["k_update_perturb"] == 0, route
        _assert_same(shared, fused, (n, spd, "fused"))
        _assert_same(shared, forced, (n, spd, "forced"))


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_thread_counts_agree_for_a_model_on_the_gpu(dtype):
    """fb_attack_dev: k_update_perturb_x writes the next batch into the model's float32 / float64 buffer."""
    dt = getattr(torch, dtype)
    n, spd, S = 4097, 10, 4
    m = FrameModel("OSI", S, "cuda:0", seed=2, device_dtype=dt)
    audio = synthetic_audio(3, n)
    out = {}
    for t in (256, 512, None):
        e = Engine(0)
        try:
            if t is not None:
                os.environ["FB_UP_THREADS"] = str(t)
            p = nes_params("OSI", "targeted", samples_per_draw=spd, max_iter=ITERS, seed=4, stream=1,
                           **dict(KW, target=1, threshold=0.5))
            x = torch.empty((spd + 1, n), dtype=dt, device="cuda:0")
            sc = torch.empty((spd + 1, S), dtype=torch.float32, device="cuda:0")
            out[t] = e.attack_dev(p, S, m.score_device, x, sc, audio, look_every=2)
            assert e.debug_foreign_path()["x_dtype"] == dtype
            assert e.debug_launch_shape()["up_threads"] == (t or 512)   # (a lone model's attack: 512 unless forced)
            assert e.debug_nes_route()["k_update_perturb"] == ITERS
        finally:
            os.environ.pop("FB_UP_THREADS", None)
            e.close()
    _assert_same(out[256], out[512], dtype)
    _assert_same(out[256], out[None], dtype)
