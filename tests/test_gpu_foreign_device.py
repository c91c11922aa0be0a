"""The plugin API with the model on the same GPU (fb_attack_dev / fb_get_grad_dev; FakeBob's score_device).

1. The reference-captured goldens g2 / g3 / g4 (tests/golden/make_golden.py) through the device path: TorchSynthModel
   restates SynthModel in torch, so with a float64 batch the bar is bit-exact equality, as in test_gpu_plugin_api.py.
2. Device path == host path for a float32 model (FrameModel): the same model driven through score_device and through
   a score-only wrapper gives identical bits -- trace, int16 and float64 audio, flag, get_grad outputs.
3. The route: fb_debug_foreign_path reports what the last foreign call ran.
4. Refusals, a raising model, and recovery on the same engine.
5. One HIP runtime in the process."""
import json
import os
import pickle

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from fakebob_amd import _native as N  # noqa: E402
from fakebob_amd.attack import FakeBob  # noqa: E402
from fakebob_amd.engine import Engine, nes_params  # noqa: E402
from tests.foreign_models import FrameModel, ScoreOnly, TorchSynthModel  # noqa: E402
from tests.golden.synth_model import synth_audio  # noqa: E402

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DEV = "cuda:0"


@pytest.fixture(scope="module")
def meta():
    with open(os.path.join(G, "golden_meta.json")) as r:
        return json.load(r)


def _noise_stream(seed, N_, half, count):
    rs = np.random.RandomState(seed)
    return [rs.normal(size=(N_, half)) for _ in range(count)]


def _route(fb):
    return fb._engine().debug_foreign_path()


# ------------------------------------------------------------------ 1. goldens
def test_g2_get_grad_through_the_device_path(meta):
    z = np.load(os.path.join(G, "g2_get_grad.npz"))
    for i, c in enumerate(meta["g2"]):
        model = TorchSynthModel(c["task"], 5, c["N"], seed=c["model_seed"], device=DEV)
        audio = synth_audio(c["N"], c["audio_seed"])
        half = c["spd"] // 2
        noise = _noise_stream(c["noise_seed"], c["N"], half, 1)[0]
        fb = FakeBob(c["task"], c["attack"], model, adver_thresh=c["kappa"], samples_per_draw=c["spd"],
                     sigma=0.001, seed=1, verbose=False)
        fb.threshold, fb.target, fb.true = c["thr"], c["target"], c["true"]
        fl, grad, al, sc = fb.get_grad(audio, noise_pos=noise)
        assert fl == float(z["final_loss_%d" % i]), i
        assert al.shape == (1,) and al[0] == float(z["adver_loss_%d" % i].reshape(-1)[0])
        assert np.array_equal(np.asarray(sc).reshape(-1), z["score_%d" % i].reshape(-1))
        assert grad.shape == (c["N"], 1) and np.array_equal(grad[:, 0], z["grad_%d" % i].reshape(-1)), i
        assert model.n_dev_calls == 1 and model.n_dev_scored == 2 * half + 1 and model.n_calls == 0
        r = _route(fb)
        assert r["path"] == "device" and r["x_dtype"] == "float64" and r["model_calls"] == 1
        assert r["batch_bytes_d2h"] == 0 and r["score_bytes_h2d"] == 0


@pytest.mark.parametrize("look_every", [1, 4])
def test_g3_attack_trajectories_through_the_device_path(meta, tmp_path, look_every):
    z = np.load(os.path.join(G, "g3_attack.npz"))
    for i, c in enumerate(meta["g3"]):
        fbkw, at = c["fbkw"], c["atkw"]
        model = TorchSynthModel(c["task"], 5, c["N"], seed=c["model_seed"], device=DEV, look_every=look_every)
        audio = z["audio_%d" % i] if c["custom_audio"] else synth_audio(c["N"], c["audio_seed"])
        half = fbkw["samples_per_draw"] // 2
        noise = np.stack(_noise_stream(c["noise_seed"], c["N"], half, fbkw["max_iter"]))
        fb = FakeBob(c["task"], c["attack"], model, seed=1, verbose=False, **fbkw)
        cp = str(tmp_path / ("cp_%d_%d" % (i, look_every)))
        adv, flag = fb.attack(audio, cp, noise_all=noise, **at)
        want = z["trace_%d" % i]
        assert flag == c["flag"], c["name"]
        assert adv.dtype == np.int16 and adv.shape == tuple(c["adv_shape"])
        assert np.array_equal(adv, z["adv_%d" % i].reshape(adv.shape)), c["name"]
        if look_every == 1:
            assert model.n_dev_calls == c["n_get_grad"], c["name"]
        else:
            assert c["n_get_grad"] <= model.n_dev_calls <= c["n_get_grad"] + look_every - 1, c["name"]
        with open(cp, "rb") as r:
            rows = pickle.load(r)
        assert len(rows) == c["n_rows"] == want.shape[0]
        assert [row[0] for row in rows] == list(want[:, 0]), c["name"]
        assert [float(row[1][0]) for row in rows] == list(want[:, 1]), c["name"]
        got_sc = np.array([np.asarray(row[2]).reshape(-1) for row in rows])
        assert np.array_equal(got_sc, want[:, 2:]), c["name"]
        assert (rows[-1][3] == 0.0) == bool(c["last_time_is_zero"])
        r = _route(fb)
        assert r["path"] == "device" and r["launches_per_iter"] == 3   # noise replay: unfused
        assert r["batch_bytes_d2h"] == 0 and r["score_bytes_h2d"] == 0


def test_g4_estimate_threshold_through_the_device_path(meta):
    for c in meta["g4"]:
        fbkw = c["fbkw"]
        model = TorchSynthModel(c["task"], 5, c["N"], seed=c["model_seed"], threshold=c["model_threshold"], device=DEV)
        audio = synth_audio(c["N"], c["audio_seed"])
        half = fbkw["samples_per_draw"] // 2
        noise = np.stack(_noise_stream(c["noise_seed"], c["N"], half, max(c["n_get_grad"], 1)))
        fb = FakeBob(c["task"], "targeted", model, seed=1, verbose=False, **fbkw)
        score, n_iters, _secs = fb.estimate_threshold(audio, noise_all=noise)
        assert n_iters == c["n_iters"] and score == c["score"] and fb.threshold == c["final_threshold"]
        assert fb.attack_type == c["attack_type_after"]
        assert model.n_dev_calls == c["n_get_grad"]


# ------------------------------------------------------- 2. device == host path
def _pair(task, n_spk, look_every=1, device_dtype=torch.float32, seed=11):
    return (FrameModel(task, n_spk, DEV, seed=seed, look_every=look_every, device_dtype=device_dtype),
            ScoreOnly(FrameModel(task, n_spk, DEV, seed=seed, device_dtype=device_dtype)))


def _attack_both(task, attack_type, n, spd, max_iter=8, look_every=1, device_dtype=torch.float32, noise=False,
                 fbkw=None, atkw=None):
    dm, hm = _pair(task, 4, look_every, device_dtype)
    audio = synth_audio(n, 5)
    na = np.stack(_noise_stream(3, n, spd // 2, max_iter)) if noise else None
    out = []
    for m in (dm, hm):
        fb = FakeBob(task, attack_type, m, samples_per_draw=spd, max_iter=max_iter, seed=9, verbose=False,
                     epsilon=0.01, max_lr=0.003, **(fbkw or {}))
        eng = fb._engine()
        kw = dict(atkw or {})
        fb.threshold, fb.target, fb.true = kw.get("threshold", 0.), kw.get("target"), kw.get("true")
        p = fb._params()
        S = fb._speakers(audio[:, None])
        if m is dm:
            x, sc = fb._device_buffers(n, S)
            r = eng.attack_dev(p, S, m.score_device, x, sc, audio, noise_all=na, look_every=look_every)
        else:
            r = eng.attack_ext(p, S, fb._score_fn(16000, 16, 1, False), audio, noise_all=na)
        route = eng.debug_foreign_path()
        calls = m.n_calls
        g = fb._grad_foreign(eng, p, S, audio, 16000, 16, 1, False, 3, None if na is None else na[0])
        out.append((r, g, route, calls))
    return out


def _assert_same(d, h, calls_equal):
    (ra, ga, route_d, calls_d), (rb, gb, route_h, calls_h) = d, h
    adv_a, flag_a, advf_a, tr_a = ra
    adv_b, flag_b, advf_b, tr_b = rb
    assert flag_a == flag_b
    assert np.array_equal(adv_a, adv_b)
    assert np.array_equal(advf_a.view(np.uint64), advf_b.view(np.uint64))
    assert tr_a.shape == tr_b.shape and np.array_equal(tr_a.view(np.uint64), tr_b.view(np.uint64))
    assert ga[0] == gb[0] and ga[2] == gb[2]
    assert np.array_equal(ga[1].view(np.uint64), gb[1].view(np.uint64))
    assert np.array_equal(np.asarray(ga[3]), np.asarray(gb[3]))
    assert route_d["path"] == "device" and route_h["path"] == "host"
    if calls_equal:
        assert calls_d == calls_h
    return tr_a.shape[0]


@pytest.mark.parametrize("case", [
    dict(task="OSI", attack_type="targeted", n=16000, spd=50, atkw=dict(threshold=0.5, target=2)),
    dict(task="CSI", attack_type="untargeted", n=16000, spd=50, atkw=dict(true=1)),
    dict(task="SV", attack_type="targeted", n=16000, spd=50, atkw=dict(threshold=0.3)),
    dict(task="OSI", attack_type="targeted", n=12003, spd=100, atkw=dict(threshold=0.5, target=1)),   # unfused
    dict(task="CSI", attack_type="targeted", n=8002, spd=2, atkw=dict(target=3)),
    dict(task="OSI", attack_type="untargeted", n=9001, spd=20, noise=True, atkw=dict(threshold=0.5)),  # replay
    dict(task="SV", attack_type="targeted", n=16000, spd=50, device_dtype=torch.float64, atkw=dict(threshold=0.3)),
    dict(task="OSI", attack_type="untargeted", n=8000, spd=10, fbkw=dict(adver_thresh=-1e4),
         atkw=dict(threshold=0.5)),   # stops at once
])
@pytest.mark.parametrize("look_every", [1, 4])
def test_device_path_equals_host_path(case, look_every):
    case = dict(case)
    d, h = _attack_both(look_every=look_every, **case)
    _assert_same(d, h, calls_equal=look_every == 1)
    fused = not case.get("noise") and 0 < case["spd"] // 2 <= 40
    assert d[2]["launches_per_iter"] == (2 if fused else 3)
    assert d[2]["x_dtype"] == ("float64" if case.get("device_dtype") is torch.float64 else "float32")
    assert d[2]["batch_bytes_d2h"] == 0 and d[2]["score_bytes_h2d"] == 0
    B = 2 * (case["spd"] // 2) + 1
    assert h[2]["launches_per_iter"] == 3 and h[2]["batch_bytes_d2h"] == 8 * B * case["n"] * h[2]["model_calls"]
    assert h[2]["score_bytes_h2d"] == 8 * B * (1 if case["task"] == "SV" else 4) * h[2]["model_calls"]


def test_float32_scores_buffer_equals_float64():
    """fb_dev_model.score_dtype = FB_DT_F32: the loss reads the model's float32 scores and widens them exactly."""
    m = FrameModel("OSI", 4, DEV, seed=2)
    audio = synth_audio(16000, 2)
    res = []
    for sdt in (torch.float32, torch.float64):
        e = Engine(0)
        p = nes_params("OSI", "targeted", samples_per_draw=50, max_iter=6, threshold=0.5, target=1, seed=4, stream=1)
        x = torch.empty((51, 16000), dtype=torch.float32, device=DEV)
        sc = torch.empty((51, 4), dtype=sdt, device=DEV)
        res.append(e.attack_dev(p, 4, m.score_device, x, sc, audio, look_every=2))
        assert e.debug_foreign_path()["score_dtype"] == ("float32" if sdt is torch.float32 else "float64")
        e.close()
    assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][3], res[1][3])


# ------------------------------------------------------------- 4. refusals, errors
def test_refusals_and_recovery():
    e = Engine(0)
    n, spd = 4000, 10
    B = spd + 1
    p = nes_params("OSI", "targeted", samples_per_draw=spd, max_iter=4, threshold=0.5, target=1, seed=4)
    m = FrameModel("OSI", 4, DEV, seed=2)
    audio = synth_audio(n, 3)
    x = torch.empty((B, n), dtype=torch.float32, device=DEV)
    sc = torch.empty((B, 4), dtype=torch.float64, device=DEV)
    with pytest.raises(ValueError, match="is on cpu"):
        e.attack_dev(p, 4, m.score_device, x.cpu(), sc, audio)
    with pytest.raises(ValueError, match="dtype torch.float16"):
        e.attack_dev(p, 4, m.score_device, x.half(), sc, audio)

    def raw(xp, xdt, spd_=None, S=4, params=p):
        dm = N.DevModel()
        dm.x_dtype, dm.x, dm.score_dtype, dm.scores, dm.look_every = xdt, xp, N.FB_DT_F64, sc.data_ptr(), 1
        cb = N.SCORE_DEV_CB(lambda *a: 0)
        import ctypes as C
        adv = np.empty(n, np.int16)
        flag = C.c_int()
        rc = e._L.fb_attack_dev(e._h, C.byref(params), C.c_int(S), C.byref(dm), cb, None, N.ptr(audio), C.c_int64(n),
                                None, N.ptr(adv), None, None, None, C.byref(flag))
        return rc, e._L.fb_last_error().decode()
    host = np.zeros((B, n), np.float32)
    rc, msg = raw(host.ctypes.data, N.FB_DT_F32)
    assert rc == N.FB_E_ARG and "x is not device memory" in msg
    rc, msg = raw(x.data_ptr(), 7)
    assert rc == N.FB_E_ARG and "x_dtype 7" in msg
    rc, msg = raw(x.data_ptr(), N.FB_DT_F32, S=0)
    assert rc == N.FB_E_ARG and "[1, 62] (got 0)" in msg
    rc, msg = raw(x.data_ptr(), N.FB_DT_F32, S=63)
    assert rc == N.FB_E_ARG and "[1, 62] (got 63)" in msg
    psv = nes_params("SV", "targeted", samples_per_draw=spd, max_iter=4, threshold=0.5, seed=4)
    rc, msg = raw(x.data_ptr(), N.FB_DT_F32, S=2, params=psv)
    assert rc == N.FB_E_ARG and "SV scores one speaker (got S = 2)" in msg

    class Boom(Exception):
        pass

    def bad(xx):
        if bad.n == 2:
            raise Boom("model exploded")
        bad.n += 1
        return m.score_device(xx)
    bad.n = 0
    with pytest.raises(Boom):
        e.attack_dev(p, 4, bad, x, sc, audio, look_every=1)
    after = e.attack_dev(p, 4, m.score_device, x, sc, audio, look_every=1)
    e.close()
    f = Engine(0)
    fresh = f.attack_dev(p, 4, m.score_device, x, sc, audio, look_every=1)
    f.close()
    for a, b in zip(after, fresh):
        assert np.array_equal(np.asarray(a), np.asarray(b))


# --------------------------------------------------------------- 5. one runtime
def test_one_hip_runtime():
    m = TorchSynthModel("OSI", 3, 3000, seed=1, device=DEV)
    fb = FakeBob("OSI", "targeted", m, samples_per_draw=6, max_iter=3, verbose=False)
    fb.attack(synth_audio(3000, 1), None, threshold=0.1, target=1)
    assert len(N.hip_runtimes()) == 1, N.hip_runtimes()
