"""Every batch row and every kept normal of every NES launch route, element by element, against the oracle's generator.

fb_noise4 inlines fb_box_muller's quadrant chain into each kernel that draws during an attack, and that chain has been
compiled wrongly twice, each time in one kernel only (csrc/fb_device.h above fb_box_muller_sel; DESIGN.md, the HopSkipJump
section).  The rest of the suite compares those kernels with each other and with a replay of k_noise's normals, and reads
only trajectories: a launch that draws a wrong normal in a few lanes writes the same value into the batch row and into zbuf
and stays self-consistent.  Here the rows themselves are read -- a host callback's batch, a device model's x, the engine's
own int16 batch and the kept normals through fb_debug_nes_batch -- and compared bit for bit with tests/nes_batch_ref.py on
oracle.noise, at the lane patterns where the chain has gone wrong: single active lanes, partly filled waves, many grid rows
over a tiny N.

  a. k_noise                                          debug_noise
  b. k_perturb_f64                                    attack_ext / get_grad_ext, a recording callback
  c. k_perturb_x<float | double>                      get_grad_dev, x aligned and one element off
  d. k_update_perturb_x<float | double, 256 | 512>    attack_dev: x holds the batch the last update launch wrote
  e. k_perturb                                        get_grad on a tiny GMM system, 16 and 8 bits per sample
  f. k_update_perturb<256 | 512>, k_gmm_finalize_loss_update   attack / bench_nes on it, over the launch chains

Seed 77, stream 3, sigma 0.001, the stop out of reach.  Every case asserts the route it ran.  That each (route, N) group
draws every quadrant in the last, partly filled Philox counter of a row is a property of the reference:
tests/test_nes_batch_ref_host.py."""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")   # ahead of the library: the model on the GPU and the engine share one HIP runtime

from fakebob_amd import _native as N  # noqa: E402
from fakebob_amd.engine import Engine, nes_params  # noqa: E402
from fakebob_amd.models import synthetic_audio, synthetic_gmm_system  # noqa: E402
from tests import nes_batch_ref as R  # noqa: E402
from tests.foreign_models import FrameModel  # noqa: E402
from tests.golden.synth_model import synth_audio  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
S = 4
KW = dict(epsilon=0.002, sigma=R.SIGMA, max_lr=0.001, min_lr=1e-6, momentum=0.9, plateau_length=2, plateau_drop=2.0,
          adver_thresh=1e3, seed=R.SEED, stream=R.STREAM)
KNOBS = ("FB_UP_THREADS", "FB_FUSE_PARTS", "FB_NO_FUSE", "FB_FUSE_UPD", "FB_GMM_SUB", "FB_MFCC_CUS", "FB_FIN_COUNTER",
         "FB_FIN_TICKET", "FB_ATTACK_BATCH", "FB_LOOK_AHEAD")


@pytest.fixture(autouse=True)
def _clean_knobs(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


@pytest.fixture(scope="module")
def feng():
    """An engine without a model of its own: the NES kernels around a foreign model."""
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def geng():
    """The tiny GMM system of tests/test_gpu_update_shapes.py: C = 64, D = 72, UBM + 2 speakers."""
    ubm, spk = synthetic_gmm_system(n_speakers=2, C=64, D=72)
    e = Engine(0)
    e.load_gmm([ubm] + spk)
    e.set_system("OSI")
    yield e
    e.close()


def _same(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.dtype, want.shape)
    bad = np.argwhere(R.bits_of(got) != R.bits_of(want))
    assert bad.shape[0] == 0, (what, "%d elements differ" % bad.shape[0], "first (row, sample)", bad[0].tolist(),
                               got[tuple(bad[0])], want[tuple(bad[0])])


def _launches(eng):
    return {k: v for k, v in eng.debug_nes_route().items() if v}


def _foreign_params(half, max_iter=3):
    return nes_params("OSI", "targeted", samples_per_draw=2 * half, max_iter=max_iter, threshold=0.5, target=1, **KW)


def _halves(n):
    # half = 63 at N = 2: the shape of the HopSkipJump finding, 63 grid rows over one active lane
    return R.PERTURB_HALVES + ((63,) if n == 2 else ())


def _kept_normals(eng, oracle, n, half, it, what):
    """fb_debug_nes_batch after a foreign-model call: the normals the launch kept are the oracle's for iteration `it`."""
    q, z, got_it = eng.debug_nes_batch(n, half, want_q=False)
    assert q is None and got_it == it, (what, got_it, it)
    _same(z, oracle.noise(R.SEED, it, R.STREAM, n, half), (what, "zbuf"))


# ------------------------------------------------------------------ a. k_noise
@pytest.mark.parametrize("n", R.TINY_N)
def test_k_noise(feng, oracle, n):
    for half in (1, 16, 63):
        for it in (0, 7):
            _same(feng.debug_noise(R.SEED, it, R.STREAM, n, half), oracle.noise(R.SEED, it, R.STREAM, n, half), (n, half, it))


# ------------------------------------------------------------------ b. k_perturb_f64
class _Recorder(object):
    """A host scorer that keeps every batch it is handed -- a copy, or with copy=False the array itself, which the model
    owns (Engine._score_cb) and the engine must not write again.  score((N, B) float64) -> (B, S)."""

    def __init__(self, n, copy=True):
        self.W = np.random.RandomState(3).normal(size=(n, S)) / max(n, 1) ** 0.5
        self.copy = copy
        self.batches = []

    def score(self, a):
        self.batches.append(np.array(a.T, order="C") if self.copy else a.T)
        return a.T @ self.W


@pytest.mark.parametrize("n", R.TINY_N)
def test_k_perturb_f64_through_the_host_plugin_path(feng, oracle, n):
    audio = synth_audio(n, 5)
    for half in _halves(n):
        p = _foreign_params(half)
        m = _Recorder(n)
        adv, flag, advf, tr = feng.attack_ext(p, S, m.score, audio)
        assert flag == -1 and tr.shape[0] == 3 and len(m.batches) == 3, (n, half, flag, tr.shape)
        route = feng.debug_foreign_path()
        assert route["path"] == "host" and route["launches_per_iter"] == 3 and route["model_calls"] == 3
        assert _launches(feng) == dict(k_loss=3, k_grad_update=3)
        _same(m.batches[0][0], audio, (n, half, "iteration 0 starts at the audio"))
        assert np.any(R.bits_of(m.batches[2][0]) != R.bits_of(audio))          # (the attack did step)
        for it, x in enumerate(m.batches):
            _same(x, R.rows(x[0], oracle.noise(R.SEED, it, R.STREAM, n, half), "float64"), (n, half, "attack_ext", it))
        _kept_normals(feng, oracle, n, half, 2, (n, half, "attack_ext"))       # k_perturb_f64: the last batch scored
        for it in (0, 2):
            m = _Recorder(n, copy=False)
            feng.get_grad_ext(p, S, m.score, audio, it=it)
            assert len(m.batches) == 1 and _launches(feng) == dict(k_loss=1, k_grad_update=1)
            _same(m.batches[0], R.rows(audio, oracle.noise(R.SEED, it, R.STREAM, n, half), "float64"), (n, half, "get_grad_ext", it))
            _kept_normals(feng, oracle, n, half, it, (n, half, "get_grad_ext"))


def test_the_hook_refuses_what_the_last_call_did_not_leave(feng, oracle):
    n, half = 5, 7
    audio = synth_audio(n, 5)
    p = _foreign_params(half)
    feng.get_grad_ext(p, S, _Recorder(n).score, audio, it=1)
    with pytest.raises(N.NativeError) as ex:                                   # a foreign model's batch is not the engine's
        feng.debug_nes_batch(n, half)
    assert ex.value.code == N.FB_E_STATE
    for bad_n, bad_half in ((n + 1, half), (n, half + 1)):
        with pytest.raises(N.NativeError) as ex:
            feng.debug_nes_batch(bad_n, bad_half, want_q=False)
        assert ex.value.code == N.FB_E_ARG
    _kept_normals(feng, oracle, n, half, 1, "after the refusals")              # (read only: still there)
    z = oracle.noise(R.SEED, 1, R.STREAM, n, half).astype(np.float64).T.copy()
    feng.get_grad_ext(p, S, _Recorder(n).score, audio, it=1, noise_pos=z)
    with pytest.raises(N.NativeError) as ex:                                   # injected normals: none kept
        feng.debug_nes_batch(n, half, want_q=False)
    assert ex.value.code == N.FB_E_STATE
    e = Engine(0)
    try:
        with pytest.raises(N.NativeError) as ex:                               # before the first call
            e.debug_nes_batch(n, half, want_q=False)
        assert ex.value.code == N.FB_E_STATE
    finally:
        e.close()


# ------------------------------------------------------------------ c. k_perturb_x
def _frame_model(n, dtype):
    """FrameModel with a frame short enough for n samples."""
    frame = min(n, 64)
    return FrameModel("OSI", S, DEV, seed=11, frame=frame, hop=max(frame // 2, 1), device_dtype=dtype)


GUARD = 12345.0


def _batch_buffer(n, B, dtype, aligned):
    """-> (x [B, n], the allocation it lives in): 16-byte aligned, or a contiguous view one element into a larger
    allocation, which makes the kernels take the scalar stores (x_vec = 0)."""
    if aligned:
        x = torch.full((B, n), GUARD, dtype=dtype, device=DEV)
        assert x.data_ptr() % 16 == 0
        return x, None
    big = torch.full((B * n + 2,), GUARD, dtype=dtype, device=DEV)
    x = big[1:1 + B * n].view(B, n)
    assert x.is_contiguous() and big.data_ptr() % 16 == 0 and x.data_ptr() % 16 != 0
    return x, big


def _guards_untouched(big):
    return big is None or (float(big[0]) == GUARD and float(big[-1]) == GUARD)


@pytest.mark.parametrize("n", R.TINY_N)
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_k_perturb_x(feng, oracle, dtype, n):
    dt = getattr(torch, dtype)
    audio = synth_audio(n, 5)
    m = _frame_model(n, dt)
    for half in _halves(n):
        B = 2 * half + 1
        p = _foreign_params(half)
        sc = torch.empty((B, S), dtype=torch.float64, device=DEV)
        for aligned in (True, False):
            x, big = _batch_buffer(n, B, dt, aligned)
            for it in (0, 1, 2):
                what = (dtype, n, half, "aligned" if aligned else "one element off", it)
                feng.get_grad_dev(p, S, m.score_device, x, sc, audio, it=it)
                route = feng.debug_foreign_path()
                assert route["path"] == "device" and route["x_dtype"] == dtype and route["launches_per_iter"] == 3, what
                assert _launches(feng) == dict(k_loss=1, k_grad_update=1), what
                _same(x.cpu().numpy(), R.rows(audio, oracle.noise(R.SEED, it, R.STREAM, n, half), dtype), what)
                assert _guards_untouched(big), what
                _kept_normals(feng, oracle, n, half, it, what)


# ------------------------------------------------------------------ d. k_update_perturb_x
@pytest.mark.parametrize("n", R.UPD_N)
@pytest.mark.parametrize("threads", [256, 512])
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_k_update_perturb_x(feng, oracle, _clean_knobs, dtype, threads, n):
    """attack_dev to max_iter: x holds the batch the last update launch wrote for iteration max_iter, built from the returned
    float64 adversarial audio and never scored."""
    dt = getattr(torch, dtype)
    _clean_knobs.setenv("FB_UP_THREADS", str(threads))
    audio = synth_audio(n, 5)
    m = _frame_model(n, dt)
    for half in R.UPD_HALVES:
        B = 2 * half + 1
        sc = torch.empty((B, S), dtype=torch.float64, device=DEV)
        for aligned in (True, False):
            x, big = _batch_buffer(n, B, dt, aligned)
            for k in (1, 2, 3):
                what = (dtype, threads, n, half, "aligned" if aligned else "one element off", k)
                adv, flag, advf, tr = feng.attack_dev(_foreign_params(half, k), S, m.score_device, x, sc, audio)
                assert flag == -1 and tr.shape[0] == k, what
                route = feng.debug_foreign_path()
                assert route["path"] == "device" and route["x_dtype"] == dtype and route["launches_per_iter"] == 2, what
                assert _launches(feng) == dict(k_loss=k, k_update_perturb=k), what
                assert feng.debug_launch_shape()["up_threads"] == threads, what
                assert np.any(R.bits_of(advf) != R.bits_of(audio)), what
                _same(x.cpu().numpy(), R.rows(advf, oracle.noise(R.SEED, k, R.STREAM, n, half), dtype), what)
                assert _guards_untouched(big), what
                _kept_normals(feng, oracle, n, half, k, what)


# ------------------------------------------------------------------ e. k_perturb
def _gmm_params(half, max_iter=3, bits=16):
    return nes_params("OSI", "targeted", samples_per_draw=2 * half, max_iter=max_iter, target=0, threshold=0.2277,
                      bits_per_sample=bits, **KW)


@pytest.mark.parametrize("n", R.GMM_N)
@pytest.mark.parametrize("bits", [16, 8])
def test_k_perturb(geng, oracle, bits, n):
    audio = synthetic_audio(3, n)
    geng.set_fused_chain(None)
    for half in R.GMM_PERTURB_HALVES:
        p = _gmm_params(half, bits=bits)
        for it in (0, 1, 2):
            what = (bits, n, half, it)
            geng.get_grad(p, audio, it=it)
            assert _launches(geng) == dict(k_loss=1, k_grad_update=1), what
            q, z, got_it = geng.debug_nes_batch(n, half)
            assert got_it == it, what
            zo = oracle.noise(R.SEED, it, R.STREAM, n, half)
            _same(z, zo, (what, "zbuf"))
            _same(q, R.rows(audio, zo, "int16", bits=bits), (what, "batch"))


# ------------------------------------------------------------------ f. k_update_perturb, k_gmm_finalize_loss_update
# name: (set_fused_chain, the environment, the kinds of launch an iteration queues, threads of the update workgroups)
CHAINS = {
    "fused": (True, {}, ("fin_loss_update",), 512),
    "FB_FUSE_UPD=0": (True, {"FB_FUSE_UPD": "0"}, ("fin_loss", "k_update_perturb"), 512),
    "shared 256": (False, {"FB_UP_THREADS": "256"}, ("k_loss", "k_update_perturb"), 256),
    "shared 512": (False, {"FB_UP_THREADS": "512"}, ("k_loss", "k_update_perturb"), 512),
}


def _resident_batch(geng, oracle, n, half, it, a, what, row0=None):
    """The engine's resident batch is iteration `it`'s, built from the float64 iterate `a`."""
    q, z, got_it = geng.debug_nes_batch(n, half)
    assert got_it == it, (what, got_it, it)
    zo = oracle.noise(R.SEED, it, R.STREAM, n, half)
    _same(z, zo, (what, "zbuf"))
    want = R.rows(a, zo, "int16")
    if row0 is not None:
        want[0] = row0
    _same(q, want, (what, "batch"))


@pytest.mark.parametrize("n", R.GMM_N)
@pytest.mark.parametrize("chain", sorted(CHAINS))
def test_update_launches_of_the_gmm_chains(geng, oracle, _clean_knobs, chain, n):
    """attack to max_iter: the resident batch is iteration max_iter's, built from the returned float64 adversarial audio.
    half = 4 has the empty split-sum loop, 33 is the first with a fifth draw-ahead trip, which 64 threads take."""
    fused, env, kinds, threads = CHAINS[chain]
    for k, v in env.items():
        _clean_knobs.setenv(k, v)
    audio = synthetic_audio(3, n)
    geng.set_fused_chain(fused)
    try:
        for half in R.UPD_HALVES:
            for k in (1, 2, 3):
                what = (chain, n, half, k)
                adv, flag, advf, tr = geng.attack(_gmm_params(half, k), audio)
                assert flag == -1 and tr.shape[0] == k, what
                assert _launches(geng) == {kind: k for kind in kinds}, (what, _launches(geng))
                assert geng.debug_launch_shape()["up_threads"] == threads, what
                assert np.any(R.bits_of(advf) != R.bits_of(audio)), what
                _resident_batch(geng, oracle, n, half, k, advf, what)
                assert np.array_equal(geng.debug_nes_batch(n, half, want_z=False)[0][0], adv), what   # row 0: the returned int16 audio
    finally:
        geng.set_fused_chain(None)


def test_bench_nes_leaves_the_batch_of_its_next_iteration(geng, oracle):
    n, half = 4101, 7
    audio = synthetic_audio(3, n)
    geng.set_fused_chain(True)
    try:
        p = _gmm_params(half, 1000)
        before = geng.debug_nes_route()                                        # (bench_nes adds to the last call's counts)
        geng.bench_nes(p, audio, 0, 3)
        assert geng.debug_nes_route() == dict(before, fin_loss_update=before["fin_loss_update"] + 3)
        assert geng.debug_launch_shape()["up_threads"] == 512
        a = geng.bench_nes_state(p, n)["adver"]
        assert np.any(R.bits_of(a) != R.bits_of(audio))
        _resident_batch(geng, oracle, n, half, 3, a, "bench_nes")
        geng.bench_nes(p, audio, -1, 2)                                        # ... and continued: iterations 3 and 4
        _resident_batch(geng, oracle, n, half, 5, geng.bench_nes_state(p, n)["adver"], "bench_nes continued")
    finally:
        geng.set_fused_chain(None)


def test_every_launch_on_its_own_leaves_the_last_batch_it_scored(geng, oracle, _clean_knobs):
    """FB_NO_FUSE=1 is k_perturb (covered by e): after max_iter = 1 the resident batch is iteration 0's, built from the audio;
    the attack's epilogue has put the returned int16 audio into row 0."""
    n, half = 4099, 7
    audio = synthetic_audio(3, n)
    _clean_knobs.setenv("FB_NO_FUSE", "1")
    geng.set_fused_chain(None)
    adv, flag, advf, tr = geng.attack(_gmm_params(half, 1), audio)
    assert flag == -1 and tr.shape[0] == 1
    assert _launches(geng) == dict(k_loss=1, k_grad_update=1)
    assert geng.debug_launch_shape()["up_threads"] == 0
    assert np.any(R.bits_of(advf) != R.bits_of(audio))
    _resident_batch(geng, oracle, n, half, 0, audio, "FB_NO_FUSE=1", row0=adv)
    assert np.array_equal(adv, R.rows(advf, np.empty((0, n), np.float32), "int16")[0])


def test_an_attack_that_stops_leaves_the_stopping_iterations_batch(geng, oracle):
    """adver_thresh far below every loss: iteration 0 stops the attack, the launches queued behind it return on the flag, and
    the resident batch is iteration 0's, built from the audio."""
    n, half = 4097, 7
    audio = synthetic_audio(3, n)
    geng.set_fused_chain(True)
    try:
        p = nes_params("OSI", "targeted", samples_per_draw=2 * half, max_iter=3, target=0, threshold=0.2277,
                       **dict(KW, adver_thresh=-1e4))
        adv, flag, advf, tr = geng.attack(p, audio)
        assert flag == 1 and tr.shape[0] == 1
        _same(advf, audio, "no step was taken")
        _resident_batch(geng, oracle, n, half, 0, audio, "stopped at iteration 0")
    finally:
        geng.set_fused_chain(None)
