"""Restatements of the white-box gradient THROUGH the over-the-air channel (include/fakebob_hip.h, "The over-the-air channel
(fb_set_wb_air)"), written from the header's contract.  Test infrastructure only.

numpy twin      the saturation mask from the exact integer sums of tests/air_channel_ref.py (conv_sums) and the correlation
                dx[m] = 2^-14 sum_k t[k] g[m + k] -- int64 for integer cotangents (exact), float64 or np.longdouble otherwise.
PyTorch         the channel as a custom autograd function whose forward is the numpy twin's int16 row and whose backward is
                that correlation, in front of tests/bpda_ref.py's defence chain and tests/whitebox_ref.py's front end, GMM and
                loss.  The taps of every replica are an ARGUMENT: the generator has its own contract and tests
                (tests/test_gpu_air_channel.py), the engine's draw is read with Engine.debug_air_taps."""
import numpy as np
import torch

from tests import air_channel_ref as A
from tests import bpda_ref as B
from tests import whitebox_ref as R

F64 = torch.float64


def sat_mask(x, t):
    """1 where the channel's output (y[i] + 8192) >> 14 lies outside [-32768, 32767] before the clip; uint8, x's length"""
    o = (A.conv_sums(x, t) + 8192) >> 14
    return ((o < -32768) | (o > 32767)).astype(np.uint8)


def correlate(t, g, dtype=np.float64):
    """S[m] = sum_{k = 0 .. min(L - 1, n - 1 - m)} t[k] g[m + k], one shifted product per tap, in `dtype` (np.int64: exact for
    integer g; np.longdouble: the reference of a float64 sum)"""
    g = np.asarray(g).astype(dtype)
    t = np.asarray(t).astype(np.int64)
    n = g.size
    s = np.zeros(n, dtype)
    for k in np.flatnonzero(t):
        if k < n:
            s[:n - k] += dtype(t[k]) * g[k:]
    return s


def conv_t(t, cot, sat=None, dtype=np.float64):
    """dx = 2^-14 * correlate(t, g), g = cot with the saturated positions zeroed.  dtype = np.int64 takes integer cotangents
    and returns float64 exactly (the sums are integers below 2^53, the scaling is a power of two)."""
    g = np.asarray(cot).astype(dtype).copy()
    if sat is not None:
        g[np.asarray(sat).astype(bool)] = 0
    s = correlate(t, g, dtype)
    if dtype is np.int64:
        assert np.abs(s).max(initial=0) < 2 ** 53
        return s.astype(np.float64) * 2.0 ** -14
    return s * dtype(2.0 ** -14)


def bound(t, cot, sat=None):
    """The float64 summation bound of the kernel's L + 15 terms, per sample: (L + 16) 2^-53 2^-14 sum_k |t[k]| |g[m + k]|"""
    g = np.abs(np.asarray(cot, np.float64))
    if sat is not None:
        g[np.asarray(sat).astype(bool)] = 0.0
    return (len(t) + 16) * 2.0 ** -53 * 2.0 ** -14 * correlate(np.abs(np.asarray(t).astype(np.int64)), g, np.longdouble).astype(np.float64)


def full_range_case(n=64):
    """Two taps of 16384 over +-32767 input: o[i] = x[i] + x[i - 1], saturated exactly where two neighbours of one sign add up
    beyond a rail.  The signs alternate, except that every tenth sample repeats its neighbours' sign: two saturated outputs
    in ten.  -> (taps int16 (2,), x int16 (n,))"""
    t = np.array([16384, 16384], np.int16)
    x = np.where(np.arange(n) % 2 == 0, 32767, -32767).astype(np.int16)
    x[9::10] = 32767                                  # x[8], x[9], x[10] = +, +, +
    return t, x


class AirChannel(torch.autograd.Function):
    """y = the channel's int16 output row (float64 tensor); backward: rounding and shift the identity, saturation passes zero,
    the taps constants"""

    @staticmethod
    def forward(ctx, x, taps):
        xi = B._i16(x)
        ctx.taps, ctx.sat = np.asarray(taps, np.int16), sat_mask(xi, taps)
        return torch.as_tensor(A.convolve(xi, ctx.taps).astype(np.float64))

    @staticmethod
    def backward(ctx, gy):
        return torch.as_tensor(conv_t(ctx.taps, gy.numpy(), ctx.sat)), None


def channel_defence(x, taps, chain, codec=None, normals=None):
    """channel, chain, codec on the row x (float64 tensor, int16 values) -> the row the front end reads.  (bpda_ref's defence
    takes an SNR stage's power from ITS input: the channel's output row, as the engine's k_tf_power does.)"""
    return B.defence(AirChannel.apply(x, taps), chain, codec, normals)


def defence_vjp(wav, taps, chain, codec, normals, cot):
    """-> (dwav [n] float64 = cot through codec, chain and channel at wav, out [n] int16 = the row the front end reads)"""
    x = torch.tensor(np.asarray(wav, np.float64).reshape(-1), requires_grad=True)
    y = channel_defence(x, taps, chain, codec, normals)
    (y * torch.as_tensor(np.asarray(cot, np.float64))).sum().backward()
    return x.grad.numpy().copy(), B._i16(y)


def loss_and_grad(cfg, models, task, attack_type, audio, taps, chain=(), codec=None, normals=None, bits=16, threshold=0.0,
                  adver_thresh=0.0, target=0, true=0, z_mean=None, z_std=None):
    """The EOT mean over len(taps) replicas -- taps[j] replica j's response, normals[j] its {stage: float32 normals} -- of
    whitebox_ref's loss behind channel, chain and codec.  -> bpda_ref.loss_and_grad's Result."""
    r = len(taps)
    normals = [None] * r if normals is None else normals
    a = torch.tensor(np.asarray(audio, np.float64).reshape(-1), requires_grad=True)
    x = R.cast_st(a, bits)
    losses, scores, margins = [], [], []
    for j in range(r):
        feats, _mask, margin = R.features(cfg, channel_defence(x, taps[j], list(chain), codec, normals[j]))
        s = R.system_scores(task, R.gmm_raw(feats, *models), z_mean, z_std)
        losses.append(R.loss_fn(task, attack_type, s, threshold, adver_thresh, target, true))
        scores.append(s.detach().numpy().copy())
        margins.append(margin)
    acc = losses[0]
    for l in losses[1:]:
        acc = acc + l
    mean = acc / float(r)
    mean.backward()
    res = R.Result()
    res.grad, res.loss = a.grad.numpy().copy(), float(mean.detach())
    res.losses, res.all_scores = [float(l.detach()) for l in losses], np.array(scores)
    res.scores = B.TN.eot_mean(res.all_scores.T)
    res.margin = min(margins)
    return res
