"""Foreign models on the GPU for the device-path tests (FakeBob's score_device; fb_attack_dev / fb_get_grad_dev).

TorchSynthModel restates tests/golden/synth_model.py in torch: the same int64 products and sums and the same float64
power-of-two scaling, so its scores equal SynthModel.score bit for bit on any device.  FrameModel is a small float32
model (framing by unfold, matmul, log, mean: no convolutions) whose result depends only on its input's bits; ScoreOnly
wraps it with the host plugin API alone (score on an (N, B) float64 numpy batch), so the same model can drive both
paths.  Not part of the product: torch is imported here, and only the tests that use these import this module."""
import numpy as np
import torch

from tests.golden.synth_model import SynthModel


def int16_cast(x, bits_per_sample=16):
    """numpy's `(a * 2^(bits - 1)).astype(np.int16)` (gmm_ubm_OSI.py:85) as torch int64: truncation toward zero, then
    wrapping to 16 bits, as x86 does (98304 -> -32768, 65536 -> 0).  A float -> int16 conversion on the GPU need not
    wrap, hence no .to(torch.int16)."""
    t = torch.trunc(x * float(2 ** (bits_per_sample - 1))).to(torch.int64)
    return ((t + 32768) & 0xFFFF) - 32768


class TorchSynthModel(SynthModel):
    """SynthModel with score_device: x [B, N] (float32 / float64 torch tensor) -> [B, S] float64 scores ([B] for SV).
    score / make_decisions stay SynthModel's (host) ones; score_device calls are counted apart from them."""

    def __init__(self, *args, **kw):
        dev = kw.pop("device", "cpu")
        self.device_dtype = kw.pop("device_dtype", torch.float64)
        self.look_every = kw.pop("look_every", 0)
        SynthModel.__init__(self, *args, **kw)
        self.n_dev_calls = 0
        self.n_dev_scored = 0
        self.to(dev)

    def to(self, device):
        self.tW = torch.from_numpy(self.W).to(device)
        self.tDq = torch.from_numpy(self.Dq).to(device)
        self.tbias = torch.from_numpy(self.bias).to(device)
        return self

    def raw_device(self, x):
        q = int16_cast(x.reshape(x.shape[0], -1))
        q2 = q * q
        lin = torch.stack([(q * self.tW[s]).sum(dim=1) for s in range(self.S)], dim=1) + self.tbias
        quad = torch.stack([(q2 * self.tDq[s]).sum(dim=1) for s in range(self.S)], dim=1)
        return lin.to(torch.float64) * 2.0 ** -self.lin_shift - quad.to(torch.float64) * 2.0 ** -self.quad_shift

    def score_device(self, x):
        self.n_dev_calls += 1
        self.n_dev_scored += int(x.shape[0])
        sc = self.raw_device(x)
        return sc[:, 0] if self.task == "SV" else sc


class FrameModel(object):
    """float32 speaker scorer: 25 ms frames every 10 ms (unfold), a seeded projection (matmul), log energies, their mean
    over frames, a seeded speaker matrix.  score_device(x [B, N]) -> [B, S] float32 ([B] for SV)."""

    def __init__(self, task, n_spk, device, seed=0, frame=400, hop=160, n_feat=24, look_every=0,
                 device_dtype=torch.float32):
        g = torch.Generator().manual_seed(seed)
        self.task = task
        self.S = 1 if task == "SV" else n_spk
        self.frame, self.hop = frame, hop
        self.P = (torch.randn(frame, n_feat, generator=g) / frame ** 0.5).to(device)
        self.Wspk = torch.randn(n_feat, self.S, generator=g).to(device)
        self.spk_ids = ["spk%02d" % i for i in range(self.S)]
        self.device = device
        self.device_dtype = device_dtype
        self.look_every = look_every
        self.n_calls = 0

    def score_device(self, x):
        self.n_calls += 1
        x = x.float()
        B = x.shape[0]
        fr = x.unfold(1, self.frame, self.hop)                      # [B, T, frame]
        T = fr.shape[1]
        e = fr.reshape(B * T, self.frame) @ self.P                  # [B T, n_feat]
        f = torch.log(e * e + 1e-4).reshape(B, T, -1).mean(dim=1)   # [B, n_feat]
        sc = f @ self.Wspk                                          # [B, S]
        return sc[:, 0] if self.task == "SV" else sc


class ScoreOnly(object):
    """The host plugin API around a FrameModel: score((N, B) float64 numpy) -> numpy, through a GPU tensor and .float()
    exactly as the device path hands the model its float32 batch."""

    def __init__(self, model):
        self.m = model
        self.task = model.task
        self.spk_ids = model.spk_ids
        self.n_calls = 0

    def score(self, audios, fs=16000, bits_per_sample=16, n_jobs=1, debug=False):
        self.n_calls += 1
        a = np.asarray(audios, np.float64)
        a = a.reshape(-1, 1) if a.ndim == 1 else a
        x = torch.from_numpy(np.ascontiguousarray(a.T)).to(self.m.device).to(self.m.device_dtype)
        return self.m.score_device(x).double().cpu().numpy()
