"""The NES step (perturbed batch, loss_fn, np.mean(loss * noise) / sigma, momentum sign step, clip, plateau and stop
rules) at the parameter values where it switches kernels, templates or launch paths -- samples_per_draw 8 .. 1030, 3 ..
62 speakers, plateau windows of 1 .. 12 losses, utterances of 3 .. 9001 samples, an unaligned batch buffer -- away from
the recipe's values the rest of the suite runs at.  Everything compares bits, except the one comparison with the oracle's
GMM scores at the bar tests/test_gpu_configs.py uses for it.

a. g11 (tests/golden/make_golden_nes_edges.py: the reference's own FAKEBOB.py at these values) through the host plugin
   path and the device path, as test_gpu_plugin_api.py / test_gpu_foreign_device.py do for g2 / g3.
b. Philox replay: the fused and LDS-staged paths run only without injected noise, so g11 cannot reach them.  An attack on
   the device's Philox stream must equal the same attack fed those normals as noise_all -- the path (a) pins to g11.
c. The device path equals the host path, with the model's batch buffer 16-byte aligned and one element off.
d. The engine's own GMM system: the four launch chains are bit-identical and equal their Philox replay.
e. The i-vector system's solve-kernel tail against k_loss.
Every case asserts the route it ran: launches_per_iter for a foreign model, and for every scorer the launches of each kind
the call queued (fb_debug_nes_route: the loss in the i-vector solve kernel's tail, in the GMM finalising launch with or
without the update, or in k_loss; the momentum step in k_update_perturb or k_grad_update)."""
import pickle

import numpy as np
import pytest

import torch

from fakebob_amd.attack import FakeBob  # noqa: E402
from fakebob_amd.engine import Engine, nes_params  # noqa: E402
from fakebob_amd.models import (stack_models, synthetic_audio, synthetic_gmm_system,  # noqa: E402
                                synthetic_ivector_system)
from tests import nes_edges_ref as R  # noqa: E402
from tests.foreign_models import FrameModel, ScoreOnly, TorchSynthModel  # noqa: E402
from tests.golden.synth_model import SynthModel, synth_audio  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FUSE_MAX_HALF = 40          # fb_kernels.h: FB_FUSE_MAX_HALF
CHAIN_ENV = ("FB_NO_FUSE", "FB_FUSE_UPD", "FB_FUSE_PARTS", "FB_FIN_COUNTER", "FB_FIN_TICKET", "FB_ATTACK_BATCH",
             "FB_IV_TAIL", "FB_IV_SOLVE", "FB_VAD_WHOLE")


@pytest.fixture(scope="module")
def g11():
    return R.load()


@pytest.fixture(scope="module")
def feng():
    """An engine without a model of its own: the NES kernels around a foreign model."""
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture
def clean_env(monkeypatch):
    for k in CHAIN_ENV:
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def _launches(eng):
    """fb_debug_nes_route of the last call, the kinds that ran only: {kind: launches}."""
    return {k: v for k, v in eng.debug_nes_route().items() if v}


def _assert_same_attack(a, b, what):
    """(int16 adv, flag, float64 adv, trace) twice: the same bits."""
    assert a[1] == b[1], what
    assert np.array_equal(a[0], b[0]), what
    assert np.array_equal(_bits(a[2]), _bits(b[2])), what
    assert a[3].shape == b[3].shape and np.array_equal(_bits(a[3]), _bits(b[3])), what


# ------------------------------------------------------------------ a. g11 through both foreign paths
def _fakebob_grad(c, model):
    fb = FakeBob(c["task"], c["attack"], model, adver_thresh=c["kappa"], samples_per_draw=c["spd"], sigma=0.001, seed=1,
                 verbose=False)
    fb.threshold, fb.target, fb.true = c["thr"], c["target"], c["true"]
    return fb


def _assert_grad_case(z, i, c, got):
    fl, grad, al, sc = got
    assert fl == float(z["final_loss_%d" % i]), c
    assert al.shape == (1,) and al[0] == float(z["adver_loss_%d" % i].reshape(-1)[0]), c
    assert np.array_equal(np.asarray(sc).reshape(-1), z["score_%d" % i].reshape(-1)), c
    assert grad.shape == (c["N"], 1) and np.array_equal(grad[:, 0], z["grad_%d" % i].reshape(-1)), c


def test_g11_get_grad_through_the_plugin_api(g11):
    """k_perturb_f64, k_loss<SMALL> at 128 against 130 and with B > 1024 (losses read back from memory), k_grad_update on
    injected normals in one block of NumPy's sum and in its recursion, three 256-sample blocks, the last of 3 samples."""
    z, meta = g11
    for i, c in enumerate(meta["get_grad"]):
        model = SynthModel(c["task"], c["n_spk"], c["N"], seed=c["model_seed"])
        audio = synth_audio(c["N"], c["audio_seed"])
        half = c["spd"] // 2
        fb = _fakebob_grad(c, model)
        _assert_grad_case(z, i, c, fb.get_grad(audio, noise_pos=R.noise_stream(c["noise_seed"], c["N"], half, 1)[0]))
        assert model.n_calls == 1 and model.n_scored == 2 * half + 1
        r = fb._engine().debug_foreign_path()
        assert r["path"] == "host" and r["launches_per_iter"] == 3


def test_g11_get_grad_through_the_device_path(g11):
    z, meta = g11
    for i, c in enumerate(meta["get_grad"]):
        model = TorchSynthModel(c["task"], c["n_spk"], c["N"], seed=c["model_seed"], device=DEV)
        audio = synth_audio(c["N"], c["audio_seed"])
        half = c["spd"] // 2
        fb = _fakebob_grad(c, model)
        _assert_grad_case(z, i, c, fb.get_grad(audio, noise_pos=R.noise_stream(c["noise_seed"], c["N"], half, 1)[0]))
        assert model.n_dev_calls == 1 and model.n_dev_scored == 2 * half + 1 and model.n_calls == 0
        r = fb._engine().debug_foreign_path()
        assert r["path"] == "device" and r["x_dtype"] == "float64" and r["launches_per_iter"] == 3
        assert r["batch_bytes_d2h"] == 0 and r["score_bytes_h2d"] == 0


def _assert_attack_case(z, i, c, audio, adv, flag, cp):
    want = z["trace_%d" % i]
    assert flag == c["flag"], c["name"]
    assert adv.dtype == np.int16 and adv.shape == tuple(c["adv_shape"])
    assert np.array_equal(adv.reshape(-1), R.adv_i16(z, i, audio)), c["name"]
    with open(cp, "rb") as r:
        rows = pickle.load(r)                       # [distance, adver_loss (1,), score, used_time] per iteration
    assert len(rows) == c["n_rows"] == want.shape[0]
    assert [row[0] for row in rows] == list(want[:, 0]), c["name"]
    assert [float(row[1][0]) for row in rows] == list(want[:, 1]), c["name"]
    got_sc = np.array([np.asarray(row[2]).reshape(-1) for row in rows])
    assert np.array_equal(got_sc, want[:, 2:]), c["name"]
    assert (rows[-1][3] == 0.0) == bool(c["last_time_is_zero"])


def test_g11_attack_trajectories_through_the_plugin_api(g11, tmp_path):
    """Plateau windows of 1, 8 (the last kept in registers), 9 and 12 losses (kept in memory); 7, 8, 9 and 62 speakers (the
    eight-scores-in-registers switch of the loss row; B S on both sides of 2048 at samples_per_draw = 130); utterances
    of 3, 255 and 257 samples."""
    z, meta = g11
    for i, c in enumerate(meta["attack"]):
        model = SynthModel(c["task"], c["n_spk"], c["N"], seed=c["model_seed"])
        audio, noise = R.attack_inputs(c)
        fb = FakeBob(c["task"], c["attack"], model, seed=1, verbose=False, **c["fbkw"])
        cp = str(tmp_path / ("cp_%d" % i))
        adv, flag = fb.attack(audio, cp, noise_all=noise, **c["atkw"])
        _assert_attack_case(z, i, c, audio, adv, flag, cp)
        assert model.n_calls == c["n_get_grad"], c["name"]
        r = fb._engine().debug_foreign_path()
        assert r["path"] == "host" and r["launches_per_iter"] == 3


@pytest.mark.parametrize("look_every", [1, 4])
def test_g11_attack_trajectories_through_the_device_path(g11, tmp_path, look_every):
    """... with the plateau and stop rules run by k_loss between the host's looks."""
    z, meta = g11
    for i, c in enumerate(meta["attack"]):
        model = TorchSynthModel(c["task"], c["n_spk"], c["N"], seed=c["model_seed"], device=DEV, look_every=look_every)
        audio, noise = R.attack_inputs(c)
        fb = FakeBob(c["task"], c["attack"], model, seed=1, verbose=False, **c["fbkw"])
        cp = str(tmp_path / ("cp_%d_%d" % (i, look_every)))
        adv, flag = fb.attack(audio, cp, noise_all=noise, **c["atkw"])
        _assert_attack_case(z, i, c, audio, adv, flag, cp)
        assert c["n_get_grad"] <= model.n_dev_calls <= c["n_get_grad"] + look_every - 1, c["name"]
        r = fb._engine().debug_foreign_path()
        assert r["path"] == "device" and r["launches_per_iter"] == 3   # noise replay: unfused
        assert r["batch_bytes_d2h"] == 0 and r["score_bytes_h2d"] == 0


def test_g11_step_sizes_on_the_device(g11, feng):
    """The trace's step-size column (not in the checkpoint FakeBob writes) against the rates the reference printed, for
    the plateau cases: the window of 9 and 12 losses lives in memory (c.ls), 1 and 8 in registers."""
    z, meta = g11
    seen = 0
    for i, c in enumerate(meta["attack"]):
        if not c["name"].startswith("plateau"):
            continue
        fbkw, at = c["fbkw"], c["atkw"]
        model = TorchSynthModel(c["task"], c["n_spk"], c["N"], seed=c["model_seed"], device=DEV)
        audio, noise = R.attack_inputs(c)
        p = nes_params(c["task"], c["attack"], threshold=at["threshold"], seed=1, **fbkw)
        B = 2 * (fbkw["samples_per_draw"] // 2) + 1
        x = torch.empty((B, c["N"]), dtype=torch.float64, device=DEV)
        sc = torch.empty((B, model.S), dtype=torch.float64, device=DEV)
        adv, flag, _advf, tr = feng.attack_dev(p, model.S, model.score_device, x, sc, audio, noise_all=noise, look_every=3)
        lrs = z["lrs_%d" % i]                                          # printed with %f
        assert tr.shape[0] == lrs.shape[0] == c["n_rows"]
        assert np.abs(tr[:, 2] - lrs).max() <= 5.1e-7, c["name"]
        # exactly: max_lr halved each time, floored at min_lr
        allowed = [fbkw["max_lr"] / 2 ** k for k in range(3)] + [fbkw["min_lr"]]
        assert all(v in allowed for v in tr[:, 2]), c["name"]
        assert np.array_equal(adv, R.adv_i16(z, i, audio)) and flag == c["flag"]
        seen += 1
    assert seen == 4


# ------------------------------------------------------------------ b. Philox replay
def _foreign_params(spd, max_iter, seed, stream):
    # adver_thresh = 50: the loss stays positive, the attack runs its max_iter iterations
    return nes_params("OSI", "targeted", samples_per_draw=spd, max_iter=max_iter, threshold=0.5, target=2, adver_thresh=50.0,
                      epsilon=0.01, max_lr=0.003, seed=seed, stream=stream)


def _dev_attack(eng, model, p, n, audio, dtype, noise_all=None, look_every=0, x=None):
    B = 2 * (p.samples_per_draw // 2) + 1
    if x is None:
        x = torch.empty((B, n), dtype=dtype, device=DEV)
    sc = torch.empty((B, model.S), dtype=torch.float64, device=DEV)
    r = eng.attack_dev(p, model.S, model.score_device, x, sc, audio, noise_all=noise_all, look_every=look_every)
    return r, eng.debug_foreign_path()


@pytest.mark.parametrize("spd", [8, 14, 66, 72, 78, 80, 82])
@pytest.mark.parametrize("kind", ["synth_f64", "frame_f32"])
def test_device_path_on_philox_equals_its_replay(feng, kind, spd):
    """k_update_perturb_x (fb_update_perturb_body without the wait, 512 threads; the normals are drawn inside the phase-2
    loop): a fifth trip of that loop from half = 33 on (idx >= 2048) -- for 64 threads only at 33 --, a second trip of the
    staging loop (half 256 > 8192), half = 40 the last fused and 41 the first that is not; N = 1600 takes the vector stores,
    1601 the scalar ones and a last block of one sample.  (The five register sets of normals drawn ahead belong to the
    waiting form: test_gmm_launch_chains... below.)"""
    half = spd // 2
    for n in (1600, 1601):
        if kind == "synth_f64":
            model, dtype = TorchSynthModel("OSI", 4, n, seed=5, device=DEV), torch.float64
        else:
            model, dtype = FrameModel("OSI", 4, DEV, seed=11), torch.float32
        audio = synth_audio(n, 6)
        p = _foreign_params(spd, 4, seed=77, stream=3)
        got, route = _dev_attack(feng, model, p, n, audio, dtype)
        assert route["path"] == "device" and route["launches_per_iter"] == (2 if half <= FUSE_MAX_HALF else 3), (spd, n)
        assert route["x_dtype"] == ("float64" if dtype is torch.float64 else "float32")
        assert _launches(feng) == (dict(k_loss=4, k_update_perturb=4) if half <= FUSE_MAX_HALF else dict(k_loss=4, k_grad_update=4))
        noise = R.replay_noise(feng, 77, 3, n, half, 4)
        rep, route_r = _dev_attack(feng, model, p, n, audio, dtype, noise_all=noise)
        assert route_r["launches_per_iter"] == 3                      # k_perturb_x, k_loss, k_grad_update
        assert _launches(feng) == dict(k_loss=4, k_grad_update=4)
        assert got[3].shape[0] == 4 and got[1] == -1
        assert np.any(got[0] != (audio * 32768.0).astype(np.int16))   # (the attack moved the audio)
        _assert_same_attack(got, rep, (kind, spd, n))


@pytest.mark.parametrize("spd", [122, 124, 126, 128, 130, 300, 302])
def test_host_path_on_philox_equals_its_replay(feng, spd):
    """k_perturb_f64 + k_grad_update on the normals it staged in LDS: trips of 16 pairs with half % 16 != 0, more than 64 KB
    of LDS from half = 64 on (8 spd + 1024 half > 65536), half = 150 the last staged and 151 read from memory; SMALL at 128
    against 130.  N = 515: three blocks, the last of 3 samples."""
    n, half = 515, spd // 2
    model = SynthModel("OSI", 4, n, seed=5)
    audio = synth_audio(n, 6)
    p = _foreign_params(spd, 3, seed=78, stream=1)
    got = feng.attack_ext(p, 4, model.score, audio)
    route = feng.debug_foreign_path()
    assert route["path"] == "host" and route["launches_per_iter"] == 3 and route["model_calls"] == 3
    assert _launches(feng) == dict(k_loss=3, k_grad_update=3)
    g_got = feng.get_grad_ext(p, 4, model.score, audio, it=2)
    noise = R.replay_noise(feng, 78, 1, n, half, 3)
    rep = feng.attack_ext(p, 4, model.score, audio, noise_all=noise)
    g_rep = feng.get_grad_ext(p, 4, model.score, audio, it=2, noise_pos=noise[2])
    assert got[3].shape[0] == 3 and got[1] == -1
    assert np.any(got[0] != (audio * 32768.0).astype(np.int16))
    _assert_same_attack(got, rep, spd)
    assert g_got[0] == g_rep[0] and g_got[2] == g_rep[2]
    assert np.array_equal(_bits(g_got[1]), _bits(g_rep[1])) and np.array_equal(_bits(g_got[3]), _bits(g_rep[3]))


# ------------------------------------------------------------------ c. device path == host path, aligned or not
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["float32", "float64"])
@pytest.mark.parametrize("spd,n", [(66, 1600), (66, 1601), (80, 1600), (80, 1601)])
def test_device_path_equals_host_path_with_an_unaligned_batch(feng, spd, n, dtype):
    """The same FrameModel through score_device and through the host plugin API; then with x a contiguous view that
    starts one element into a larger allocation: not 16-byte aligned, so k_perturb_x and k_update_perturb_x take the scalar
    stores (x_vec = 0).  Same bits, and the elements in front of and behind the view stay as they were."""
    half, B = spd // 2, 2 * (spd // 2) + 1
    audio = synth_audio(n, 5)
    p = _foreign_params(spd, 4, seed=9, stream=2)
    dm = FrameModel("OSI", 4, DEV, seed=11, device_dtype=dtype)
    hm = ScoreOnly(FrameModel("OSI", 4, DEV, seed=11, device_dtype=dtype))
    host = feng.attack_ext(p, 4, hm.score, audio)
    route_h = feng.debug_foreign_path()
    assert route_h["path"] == "host" and route_h["launches_per_iter"] == 3

    aligned, route_a = _dev_attack(feng, dm, p, n, audio, dtype)
    assert route_a["path"] == "device" and route_a["launches_per_iter"] == 2 and half <= FUSE_MAX_HALF
    assert _launches(feng) == dict(k_loss=4, k_update_perturb=4)
    _assert_same_attack(aligned, host, (spd, n, "device == host"))
    assert aligned[3].shape[0] == 4

    guard = 12345.0
    big = torch.full((B * n + 2,), guard, dtype=dtype, device=DEV)
    x = big[1:1 + B * n].view(B, n)
    assert x.is_contiguous() and big.data_ptr() % 16 == 0 and x.data_ptr() % 16 != 0     # what makes x_vec = 0
    off, route_u = _dev_attack(feng, dm, p, n, audio, dtype, x=x)
    assert route_u["path"] == "device" and route_u["launches_per_iter"] == 2
    assert _launches(feng) == dict(k_loss=4, k_update_perturb=4)
    _assert_same_attack(off, aligned, (spd, n, "unaligned == aligned"))
    assert float(big[0]) == guard and float(big[-1]) == guard
    # ... and get_grad's k_perturb_x on its own
    sc = torch.empty((B, 4), dtype=torch.float64, device=DEV)
    g_u = feng.get_grad_dev(p, 4, dm.score_device, x, sc, audio, it=1)
    x_u = x.clone()
    xa = torch.empty((B, n), dtype=dtype, device=DEV)
    g_a = feng.get_grad_dev(p, 4, dm.score_device, xa, sc, audio, it=1)
    assert torch.equal(x_u, xa) and float(big[0]) == guard and float(big[-1]) == guard
    assert g_u[0] == g_a[0] and np.array_equal(_bits(g_u[1]), _bits(g_a[1]))


# ------------------------------------------------------------------ d. the engine's own GMM system
GMM_CASES = [(66, 9000, 3), (80, 9000, 3), (80, 9001, 3), (80, 9000, 12), (8, 9000, 3), (14, 9000, 3)]


@pytest.mark.parametrize("spd,n,n_spk", GMM_CASES)
def test_gmm_launch_chains_are_identical_and_equal_the_philox_replay(oracle, clean_env, spd, n, n_spk):
    """The update workgroups of k_gmm_finalize_loss_update (fb_update_perturb_body<WAIT>): the normals drawn ahead kept in
    five register sets from half = 33 on, the split block sum with an empty loop (samples_per_draw = 8) and tails of 6
    (14), 2 (66) and 0 (80); 12 speakers: 13 models, B S = 972 > 768 scores in memory and B M = 1053 > 512 finalising
    workgroups on the arrival counter.  The routes (fb_engine.hip: loop_knobs, attack_loop):
      fused          set_fused_chain(True): k_gmm_finalize_loss_update -- half <= FB_FUSE_MAX_HALF, Philox, 36 <= 192 blocks
      FB_FUSE_UPD=0  ... k_gmm_finalize_loss, then k_update_perturb
      shared         set_fused_chain(False): k_gmm_finalize, k_loss, k_update_perturb
      FB_NO_FUSE=1   every launch on its own: k_perturb, ..., k_loss, k_grad_update
      replay         noise_all: k_perturb, k_gmm_finalize_loss and k_grad_update on the injected normals.
    fb_debug_nes_route counts the launches of each kind a call queued: 6 for the attack that runs to max_iter, and for the
    one that stops the rows rounded up to the four iterations queued per look."""
    half = spd // 2
    assert 0 < half <= FUSE_MAX_HALF and (n + 255) // 256 <= 192
    ubm, spk = synthetic_gmm_system(n_speakers=n_spk, C=128, D=72)
    models = [ubm] + spk
    audio = synthetic_audio(6, n)
    e = Engine(0)
    try:
        e.load_gmm(models)
        e.set_system("OSI")
        raw, _ = e.score_raw([(audio * 32768.0).astype(np.int16)])
        sc = raw[0, 1:] - raw[0, 0]
        tgt = int(np.argmax(sc))
        kw_full = dict(samples_per_draw=spd, max_iter=6, target=tgt, threshold=float(sc.max()) + 50.0)
        p_full = nes_params("OSI", "targeted", seed=5, stream=0, **kw_full)
        p_stop = nes_params("OSI", "targeted", samples_per_draw=spd, max_iter=40, target=tgt, threshold=float(sc[tgt]) + 0.01,
                            epsilon=0.004, max_lr=0.002, seed=11, stream=2)

        routes = {"fused": ("fin_loss_update",), "FB_FUSE_UPD=0": ("fin_loss", "k_update_perturb"),
                  "shared": ("k_loss", "k_update_perturb"), "FB_NO_FUSE=1": ("k_loss", "k_grad_update")}

        def run(name):
            full = e.attack(p_full, audio)
            assert _launches(e) == {k: 6 for k in routes[name]}, (name, _launches(e))
            stop = e.attack(p_stop, audio)
            queued = 4 * ((stop[3].shape[0] + 3) // 4)
            assert _launches(e) == {k: queued for k in routes[name]}, (name, _launches(e))
            return [full, stop]
        got = {}
        for name, fused, env in (("fused", True, {}), ("FB_FUSE_UPD=0", True, {"FB_FUSE_UPD": "0"}), ("shared", False, {}),
                                 ("FB_NO_FUSE=1", None, {"FB_NO_FUSE": "1"})):
            for k, v in env.items():
                clean_env.setenv(k, v)
            e.set_fused_chain(fused)
            got[name] = run(name)
            chain = e.debug_frontend_route()["chain"]
            assert (chain in ("split", "whole")) == (name != "FB_NO_FUSE=1"), (name, chain)
            for k in env:
                clean_env.delenv(k, raising=False)
        e.set_fused_chain(True)
        noise = R.replay_noise(e, 5, 0, n, half, 6, oracle=oracle)
        rep = e.attack(p_full, audio, noise_all=noise)
        assert _launches(e) == dict(fin_loss=6, k_grad_update=6)
        grad0 = e.get_grad(p_full, audio, it=0)
        assert _launches(e) == dict(k_loss=1, k_grad_update=1)
    finally:
        e.close()
    ref = got["fused"]
    print("spd %d n %d speakers %d: %d rows to max_iter, %d rows to the stop (flag %d)"
          % (spd, n, n_spk, ref[0][3].shape[0], ref[1][3].shape[0], ref[1][1]))
    assert ref[0][3].shape[0] == 6 and ref[0][1] == -1
    assert 1 <= ref[1][3].shape[0] < 40 and ref[1][1] == 1              # the other one stops early
    assert np.any(ref[0][0] != (audio * 32768.0).astype(np.int16))
    for name, other in got.items():
        for a, b in zip(ref, other):
            _assert_same_attack(a, b, (spd, n, n_spk, name))
    _assert_same_attack(ref[0], rep, (spd, n, n_spk, "replay"))
    if n_spk == 12:
        # iteration 0 against the oracle, at the bar of test_attack_on_a_site_with_more_than_ten_models_equals_the_oracle
        gc, miv, iv = stack_models(models)
        ctx = oracle.GmmSystemCtx(oracle.default_cfg(), "OSI", gc, miv, iv, nthreads=8)
        po = oracle.nes_params("OSI", "targeted", ctx.S, **kw_full)
        flo, _go, alo, sco = oracle.get_grad(po, ctx.fn, ctx.ctx, audio, seed=5, it=0, stream=0)
        row0 = ref[0][3][0]                                             # [distance, adver_loss, lr, scores]
        assert sco.shape == (12,) and row0[3:].shape == (12,)
        assert np.abs(row0[3:] - sco).max() <= 2e-5 and abs(row0[1] - alo) <= 2e-5
        flg, _gg, alg, scg = grad0
        assert np.abs(scg[:12] - sco).max() <= 2e-5 and abs(flg - flo) <= 2e-5 and abs(alg - alo) <= 2e-5


# ------------------------------------------------------------------ e. the i-vector tail
@pytest.mark.parametrize("spd", [128, 130])
def test_ivector_tail_loss_equals_k_loss_and_the_philox_replay(clean_env, spd):
    """An i-vector system's loss body rides in the tail of the solve kernel while samples_per_draw <= 128
    (fb_iv_tail_takes_loss: B - 1 <= 128, with FB_IV_TAIL unset); at 130 the tail hands it back to k_loss<false>.  Either
    way the fused chain equals every launch on its own (FB_NO_FUSE=1), the separate back-end and k_loss launches
    (FB_IV_TAIL=split) and its own Philox replay.  half = 64 / 65 > FB_FUSE_MAX_HALF: the update is k_grad_update on the
    staged normals everywhere.  The tail does not depend on the chain: FB_NO_FUSE=1 changes the front end's launches
    (asserted through fb_debug_frontend_route) and keeps the tail; fb_debug_nes_route tells where the loss ran."""
    n, half = 8000, spd // 2
    sy = synthetic_ivector_system(C=96, D=72, R=48, L=24, n_speakers=2)
    audio = synthetic_audio(6, n)
    e = Engine(0)
    try:
        e.load_ivector(sy, "OSI")
        s0 = e.system_scores(e.score_raw([(audio * 32768.0).astype(np.int16)])[0])[0]
        p = nes_params("OSI", "targeted", samples_per_draw=spd, max_iter=3, target=int(np.argmin(s0)),
                       threshold=float(s0.max()) + 50.0, seed=7, stream=1)
        got = {}
        for name, fused, env in (("fused", True, {}), ("FB_NO_FUSE=1", None, {"FB_NO_FUSE": "1"}),
                                 ("FB_IV_TAIL=split", True, {"FB_IV_TAIL": "split"})):
            for k, v in env.items():
                clean_env.setenv(k, v)
            e.set_fused_chain(fused)
            got[name] = e.attack(p, audio)
            in_tail = spd <= 128 and name != "FB_IV_TAIL=split"
            assert _launches(e) == {"iv_tail" if in_tail else "k_loss": 3, "k_grad_update": 3}, (name, _launches(e))
            chain = e.debug_frontend_route()["chain"]
            assert (chain in ("split", "whole")) == (name != "FB_NO_FUSE=1"), (name, chain)
            for k in env:
                clean_env.delenv(k, raising=False)
        e.set_fused_chain(True)
        rep = e.attack(p, audio, noise_all=R.replay_noise(e, 7, 1, n, half, 3))
        assert _launches(e) == {"iv_tail" if spd <= 128 else "k_loss": 3, "k_grad_update": 3}
    finally:
        e.close()
    ref = got["fused"]
    assert ref[3].shape == (3, 3 + 2) and ref[1] == -1
    assert np.any(ref[0] != (audio * 32768.0).astype(np.int16))
    for name, other in got.items():
        _assert_same_attack(ref, other, (spd, name))
    _assert_same_attack(ref, rep, (spd, "replay"))
