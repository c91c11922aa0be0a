"""The device path of the plugin API without a GPU: the torch restatement of SynthModel against SynthModel itself, the
routing of FakeBob (score_device -> fb_attack_dev / fb_get_grad_dev, score -> the _ext pair, a native system -> its
engine), and the ABI (ctypes prototypes, header declarations)."""
import os
import re

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from fakebob_amd import _native as N  # noqa: E402
from fakebob_amd.attack import FakeBob  # noqa: E402
from tests.foreign_models import TorchSynthModel, int16_cast  # noqa: E402
from tests.golden.synth_model import SynthModel, synth_audio  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")


def _same(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


@pytest.mark.parametrize("task", ["OSI", "CSI", "SV"])
def test_torch_synth_model_equals_synth_model_bit_for_bit(task):
    N_ = 1601
    ref = SynthModel(task, 5, N_, seed=3)
    tm = TorchSynthModel(task, 5, N_, seed=3)
    rs = np.random.RandomState(7)
    cols = [synth_audio(N_, s) for s in range(4)]
    cols.append(np.clip(synth_audio(N_, 9) + 1e-3 * rs.normal(size=N_), -1, 1))   # values between the int16 steps
    edge = np.zeros(N_)
    edge[:8] = [1.0, -1.0, 1 + 2 ** -15, -1 - 2 ** -15, 3.0, -3.0, 2.0, 98304 / 32768.]   # +-1, past int16, wrap
    cols.append(edge)
    audios = np.stack(cols, axis=1)                           # (N, B), as FAKEBOB.py:250 hands them to score
    want = np.asarray(ref.score(audios)).reshape(len(cols), -1)
    got = tm.score_device(torch.from_numpy(np.ascontiguousarray(audios.T))).numpy().reshape(len(cols), -1)
    assert _same(got, want)
    assert tm.n_dev_calls == 1 and tm.n_dev_scored == len(cols)


def test_torch_synth_model_on_the_golden_inputs():
    import json
    with open(os.path.join(G, "golden_meta.json")) as r:
        meta = json.load(r)
    z = np.load(os.path.join(G, "g3_attack.npz"))
    cases = [(c["task"], c["N"], c["model_seed"], synth_audio(c["N"], c["audio_seed"])) for c in meta["g2"]]
    cases += [(c["task"], c["N"], c["model_seed"],
               z["audio_%d" % i] if c["custom_audio"] else synth_audio(c["N"], c["audio_seed"]))
              for i, c in enumerate(meta["g3"])]
    for task, n, seed, audio in cases:
        ref = SynthModel(task, 5, n, seed=seed)
        tm = TorchSynthModel(task, 5, n, seed=seed)
        noise = np.random.RandomState(seed).normal(size=(n, 4)) * 1e-3
        batch = np.concatenate([audio.reshape(-1, 1), audio.reshape(-1, 1) + noise], axis=1)
        want = np.asarray(ref.score(batch)).reshape(batch.shape[1], -1)
        got = tm.score_device(torch.from_numpy(np.ascontiguousarray(batch.T))).numpy().reshape(batch.shape[1], -1)
        assert _same(got, want), (task, n)


def test_int16_cast_wraps_like_numpy():
    v = np.array([0.0, 1.0, -1.0, 1 + 2 ** -15, -1 - 2 ** -15, 0.99999, -0.99999, 2.0, 3.0, -3.0, 98304 / 32768.,
                  65536 / 32768., -65537 / 32768., 1.5, -1.5, 3.2e-5, -3.2e-5])
    want = (v * 32768).astype(np.int16).astype(np.int64)
    assert np.array_equal(int16_cast(torch.from_numpy(v)).numpy(), want)
    assert int16_cast(torch.tensor([98304 / 32768.])).item() == -32768
    assert int16_cast(torch.tensor([65536 / 32768.], dtype=torch.float64)).item() == 0
    for bits in (8, 12):
        want = (v * 2 ** (bits - 1)).astype(np.int16).astype(np.int64)
        assert np.array_equal(int16_cast(torch.from_numpy(v), bits).numpy(), want)


# ---- routing with a stub engine
class _StubEngine(object):
    device = 0
    n_speakers = 3

    def __init__(self):
        self.calls = []

    def _ret_attack(self, n):
        return np.zeros(n, np.int16), -1, np.zeros(n), np.zeros((1, 6))

    def attack(self, p, audio, noise_all=None):
        self.calls.append("attack")
        return self._ret_attack(audio.size)

    def attack_ext(self, p, S, fn, audio, noise_all=None):
        self.calls.append("attack_ext")
        return self._ret_attack(audio.size)

    def attack_dev(self, p, S, fn, x, sc, audio, noise_all=None, look_every=0):
        self.calls.append(("attack_dev", tuple(x.shape), x.dtype, sc.dtype, look_every))
        return self._ret_attack(audio.size)

    def get_grad(self, p, audio, it=0, noise_pos=None):
        self.calls.append("get_grad")
        return 0.5, np.zeros(audio.size), 0.25, np.zeros(3)

    def get_grad_ext(self, p, S, fn, audio, it=0, noise_pos=None):
        self.calls.append("get_grad_ext")
        return 0.5, np.zeros(audio.size), 0.25, np.zeros(S)

    def get_grad_dev(self, p, S, fn, x, sc, audio, it=0, noise_pos=None):
        self.calls.append(("get_grad_dev", tuple(x.shape), x.dtype))
        return 0.5, np.zeros(audio.size), 0.25, np.zeros(S)

    def attack_iter_seconds(self, n):
        return np.zeros(n)


class _HostOnly(object):
    spk_ids = ["a", "b", "c"]

    def score(self, audios, **kw):
        return np.zeros(3)


class _DeviceModel(_HostOnly):
    look_every = 2

    def score_device(self, x):
        return x[:, :3]


class _Native(object):
    task = "OSI"
    threshold = 0.0

    def __init__(self):
        self.engine = _StubEngine()


def _routed(model, monkeypatch, stub=None):
    stub = stub or _StubEngine()
    fb = FakeBob("OSI", "targeted", model, samples_per_draw=4, max_iter=3, verbose=False)
    if not hasattr(model, "engine"):
        fb._own_engine = stub
    # the device buffers live on the engine's GPU; without one, CPU tensors of the same shape stand in
    monkeypatch.setattr(FakeBob, "_cuda", lambda self: torch.device("cpu"))
    audio = synth_audio(800, 1)
    fb.attack(audio, None, target=1)
    fb.get_grad(audio)
    return stub.calls


def test_a_model_with_score_device_takes_the_device_path(monkeypatch):
    calls = _routed(_DeviceModel(), monkeypatch)
    assert calls[0] == ("attack_dev", (5, 800), torch.float32, torch.float64, 2)
    assert calls[1] == ("get_grad_dev", (5, 800), torch.float32)

    class F64(_DeviceModel):
        device_dtype = torch.float64
    calls = _routed(F64(), monkeypatch)
    assert calls[0][2] == torch.float64 and calls[1][2] == torch.float64


def test_a_model_without_score_device_takes_the_host_path(monkeypatch):
    assert _routed(_HostOnly(), monkeypatch) == ["attack_ext", "get_grad_ext"]


def test_a_native_system_still_takes_its_own_engine(monkeypatch):
    m = _Native()
    assert _routed(m, monkeypatch, stub=m.engine) == ["attack", "get_grad"]


def test_estimate_threshold_takes_its_gradients_from_the_device_path(monkeypatch):
    class M(_DeviceModel):
        threshold = 10.0
        n = 0

        def score(self, audios, **kw):
            return np.array([1.0, 0.5, 0.2])

        def make_decisions(self, audios, **kw):
            M.n += 1
            return (1 if M.n > 3 else -1), np.array([0.9, 0.5, 0.2])
    stub = _StubEngine()
    fb = FakeBob("OSI", "targeted", M(), samples_per_draw=4, verbose=False)
    fb._own_engine = stub
    monkeypatch.setattr(FakeBob, "_cuda", lambda self: torch.device("cpu"))
    fb.estimate_threshold(synth_audio(800, 1))
    assert stub.calls and all(c[0] == "get_grad_dev" for c in stub.calls)


def test_bad_device_dtype_is_refused(monkeypatch):
    class M(_DeviceModel):
        device_dtype = torch.float16
    with pytest.raises(ValueError, match="device_dtype"):
        _routed(M(), monkeypatch)


# ---- the ABI
def test_ctypes_prototypes_exist():
    for name in ("fb_get_grad_dev", "fb_attack_dev", "fb_debug_foreign_path"):
        assert name in N.EXPORTS
    assert [f[0] for f in N.DevModel._fields_] == ["x_dtype", "x", "score_dtype", "scores", "look_every"]
    assert [f[0] for f in N.ForeignPathInfo._fields_] == ["path", "x_dtype", "score_dtype", "launches_per_iter",
                                                          "model_calls", "batch_bytes_d2h", "score_bytes_h2d"]
    assert (N.FB_DT_F32, N.FB_DT_F64) == (0, 1)
    assert N.SCORE_DEV_CB._argtypes_[1] is __import__("ctypes").c_void_p


def test_header_declares_the_device_path():
    with open(os.path.join(ROOT, "include", "fakebob_hip.h")) as r:
        h = r.read()
    with open(os.path.join(ROOT, "include", "fakebob_hip_test.h")) as r:
        ht = r.read()
    assert re.search(r"#define FB_DT_F32 0", h) and re.search(r"#define FB_DT_F64 1", h)
    assert re.search(r"typedef int \(\*fb_score_dev_cb\)\(void \*ctx, void \*stream, int64_t N, int B, int S\);", h)
    for fn in ("fb_get_grad_dev", "fb_attack_dev"):
        assert re.search(r"int %s\(fb_engine \*e, const fb_nes_params \*p, int S, const fb_dev_model \*m, "
                         r"fb_score_dev_cb cb, void \*ctx," % fn, h), fn
    for f in ("x_dtype", "x", "score_dtype", "scores", "look_every"):
        assert re.search(r"\b%s;" % f, h)
    assert "int fb_debug_foreign_path(fb_engine *e, fb_foreign_path_info *info);" in ht


def test_hip_runtime_listing_reads_the_maps():
    rt = N.hip_runtimes()
    assert isinstance(rt, list) and all("libamdhip64" in os.path.basename(p) for p in rt)
