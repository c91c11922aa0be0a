"""PyTorch float64 restatement of the white-box gradient THROUGH a defended victim (include/fakebob_hip.h, "Defended victims:
BPDA and EOT"), written from the header's contract and from nothing else.  Test infrastructure only.

Every defence stage is  y = lin(x) + (value - lin(x)).detach():
  value   the stage's exact int16 result, from the numpy twins (tests/input_transform_ref.py, input_transform_noise_ref.py,
          codec_ref.py) -- the forward is theirs, bit for bit;
  lin     the differentiable surrogate the contract names: the FIR as conv1d, the median as a gather at the window position
          it selected, masks for saturation and decimation, the identity for quantisation, noise and the codecs.
The gradient comes from autograd, never from a hand-derived backward.  Front end, GMM and loss are tests/whitebox_ref.py's.

A chain is a list of (kind, k, taps) triples, as in the twins; the normals of its noise stages are an ARGUMENT
({stage index: float32 array}): the generator has its own contract and tests."""
import numpy as np
import torch

from tests import codec_ref as K
from tests import input_transform_noise_ref as TN
from tests import input_transform_ref as T
from tests import whitebox_ref as R

F64 = torch.float64
QUANT, MEDIAN, FIR, DECIMATE, NOISE = T.QUANT, T.MEDIAN, T.FIR, T.DECIMATE, TN.NOISE


def _i16(x):
    """the int16 samples a float64 tensor holds at the forward point (they are integers in range by construction)"""
    v = x.detach().numpy()
    q = v.astype(np.int16)
    assert np.array_equal(q.astype(np.float64), v)
    return q


def median_select(xi, k):
    """Window position selected by the median of x[i - r .. i + r] (zeros outside [0, n)): the entries ordered by (value,
    position), both ascending; the entry of rank r.  -> absolute sample index of the selected entry, possibly outside [0, n)."""
    r = (k - 1) // 2
    xp = np.concatenate([np.zeros(r, np.int64), np.asarray(xi, np.int64), np.zeros(r, np.int64)])
    win = np.lib.stride_tricks.sliding_window_view(xp, k)
    order = np.argsort(win, axis=1, kind="stable")          # ties keep their positions ascending
    return np.arange(win.shape[0]) - r + order[:, r]


def fir_acc(xi, k, taps):
    """the float64 accumulator of the FIR stage before rint and clip, by the contract's own loop"""
    h = np.asarray(taps, np.float64).reshape(-1)
    n, c = len(xi), (k - 1) // 2
    xp = np.concatenate([np.zeros(c), np.asarray(xi, np.float64), np.zeros(c)])
    acc = np.zeros(n, np.float64)
    for j in range(k):
        acc = acc + h[j] * xp[2 * c - j:2 * c - j + n]
    return acc


def _outside(v):
    return (v < -32768) | (v > 32767)


def stage(x, kind, k, taps=None, z=None, E=None, real=False):
    """One stage on x (float64 tensor holding int16 values).  real=True: the surrogate alone as a real-valued function --
    no rounding, no clip, no value replaced (linear kinds only: what a finite difference can be taken of)."""
    n, k = x.shape[0], int(k)
    xi = None if real else _i16(x)
    if kind == QUANT:
        assert not real
        lin = x * torch.as_tensor(~_outside(k * np.floor_divide(xi.astype(np.int64) + k // 2, k)), dtype=F64)
        value = T.ref_stage(xi, kind, k)
    elif kind == MEDIAN:
        assert not real
        r = (k - 1) // 2
        pos = median_select(xi, k)
        xp = torch.cat([torch.zeros(r, dtype=F64), x, torch.zeros(r, dtype=F64)])   # a selected padding position absorbs
        lin = xp[torch.as_tensor(pos + r)]
        value = T.ref_stage(xi, kind, k)
    elif kind == FIR:
        h = torch.as_tensor(np.asarray(taps, np.float64).reshape(-1))
        c = (k - 1) // 2
        lin = torch.nn.functional.conv1d(x[None, None, :], torch.flip(h, [0])[None, None, :], padding=c)[0, 0]   # sum_j h[j] x[i + c - j]
        if real:
            return lin
        lin = lin * torch.as_tensor(~_outside(np.rint(fir_acc(xi, k, taps))), dtype=F64)
        value = T.ref_stage(xi, kind, k, taps)
    elif kind == DECIMATE:
        lin = x * torch.as_tensor(np.arange(n) % k == 0, dtype=F64)
        if real:
            return lin
        value = T.ref_stage(xi, kind, k)
    elif kind == NOISE:
        t0 = float(np.ravel(taps)[0])
        if real:
            return x + float(TN.noise_scale(k, t0, E, n)) * torch.as_tensor(np.asarray(z, np.float64))
        v = xi.astype(np.float64) + TN.noise_scale(k, t0, E, n) * np.asarray(z, np.float32).astype(np.float64)
        lin = x * torch.as_tensor(~_outside(np.rint(v)), dtype=F64)      # s is held constant
        value = TN.ref_noise_stage(xi, k, t0, z, E)
    else:
        raise ValueError(kind)
    return lin + (torch.as_tensor(value.astype(np.float64)) - lin).detach()


def defence(x, chain, codec=None, normals=None, real=False):
    """chain, then codec, on the row x the defences are handed (float64 tensor, int16 values) -> the row the front end reads"""
    E = None if real and not any(kd == NOISE for kd, _k, _t in chain) else TN.power(np.rint(x.detach().numpy()).astype(np.int16))
    y = x
    for s, (kind, k, taps) in enumerate(chain):
        y = stage(y, kind, k, taps, z=None if normals is None else normals.get(s), E=E, real=real)
    if codec is not None:
        assert not real
        y = y + (torch.as_tensor(K.codec(codec, _i16(y)).astype(np.float64)) - y).detach()     # BPDA: the identity
    return y


def defence_vjp(wav, chain, codec, normals, cot):
    """-> (dwav [n] float64 = the vector-Jacobian product of cot through codec and chain at wav, out [n] int16)"""
    x = torch.tensor(np.asarray(wav, np.float64).reshape(-1), requires_grad=True)
    y = defence(x, chain, codec, normals)
    (y * torch.as_tensor(np.asarray(cot, np.float64))).sum().backward()
    return x.grad.numpy().copy(), _i16(y)


def loss_and_grad(cfg, models, task, attack_type, audio, chain, codec=None, normals=(None,), bits=16, threshold=0.0, adver_thresh=0.0,
                  target=0, true=0, z_mean=None, z_std=None, cast=True, real=False):
    """The EOT mean over len(normals) replicas (normals[j]: replica j's {stage: float32 normals}) of whitebox_ref's loss behind
    the defences.  -> Result with loss, grad [N] (d loss / d audio), scores (the mean), losses / all_scores (per replica),
    margin (the smallest VAD margin of any replica)."""
    a = torch.tensor(np.asarray(audio, np.float64).reshape(-1), requires_grad=True)
    x = R.cast_st(a, bits) if cast else a * float(2 ** (bits - 1))
    losses, scores, margins = [], [], []
    for nz in normals:
        feats, _mask, margin = R.features(cfg, defence(x, chain, codec, nz, real=real))
        s = R.system_scores(task, R.gmm_raw(feats, *models), z_mean, z_std)
        losses.append(R.loss_fn(task, attack_type, s, threshold, adver_thresh, target, true))
        scores.append(s.detach().numpy().copy())
        margins.append(margin)
    acc = losses[0]
    for l in losses[1:]:
        acc = acc + l
    mean = acc / float(len(losses))
    mean.backward()
    r = R.Result()
    r.grad, r.loss = a.grad.numpy().copy(), float(mean.detach())
    r.losses, r.all_scores = [float(l.detach()) for l in losses], np.array(scores)
    r.scores = TN.eot_mean(r.all_scores.T)
    r.margin = min(margins)
    return r
