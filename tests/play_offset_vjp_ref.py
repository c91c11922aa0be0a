"""Restatement of the white-box gradient under a play offset (include/fakebob_hip.h, "Play offset": "Composition" and
"Transposed rule"), written from the header in PyTorch float64 on top of tests/universal_vjp_ref.py.  Test infrastructure only.

One row q -- the int16 cast of the call's audio, straight-through -- is scored on R = K r replicas; replica rho = u * r + j is
    w_rho[i] = clip(a_u[i] + d[(i - tau_rho) mod N], -32768, 32767),   d = q - a_0,   EVERY u, u = 0 included
with a_0 (the cast of the ORIGINAL audio), the companions and the offsets constants.  The clip is differentiated by the
project's saturation rule (universal_vjp_ref.compose): inside the rails the sample passes, elsewhere it is the rail, a
constant.  Everything behind the composition -- channel, chain, the victims, the loss, the mean over rho ascending -- is
universal_vjp_ref's, replica by replica.  tau = None gives universal_vjp_ref's own composition (w_0 = q): the S = 0 yardstick.
The gradient is autograd's."""
import numpy as np
import torch

from tests import air_vjp_ref as AV
from tests import bpda_ref as B
from tests import feco_vjp_ref as F
from tests import universal_vjp_ref as U
from tests import whitebox_iv_ref as V
from tests import whitebox_ref as R
from tests.companions_ref import mean_over_replicas


def compose(x, a0, companions, r, tau):
    """x: float64 tensor [N] holding q -> the K r composed rows as tensors"""
    n = x.shape[0]
    comp = np.asarray(companions, np.int16).reshape(-1, n)
    if tau is None:
        rows = U.compose(x, a0, comp)
        return [rows[rho // r] for rho in range(len(rows) * r)]
    a0f = torch.as_tensor(np.asarray(a0, np.int16).astype(np.float64))
    hosts = [a0f] + [torch.as_tensor(a.astype(np.float64)) for a in comp]
    d = x - a0f
    out = []
    for rho in range(len(hosts) * r):
        v = hosts[rho // r] + torch.roll(d, int(tau[rho]))            # roll: out[i] = d[(i - tau) mod N]
        inside = (v.detach() >= -32768.0) & (v.detach() <= 32767.0)
        out.append(torch.where(inside, v, torch.clamp(v.detach(), -32768.0, 32767.0)))
    return out


def _finish(a, losses, scores, margins, tv, rows):
    acc = losses[0]
    for l in losses[1:]:
        acc = acc + l
    mean = acc / float(len(losses))
    mean.backward()
    res = R.Result()
    res.grad, res.loss = a.grad.numpy().copy(), float(mean.detach())
    res.all_scores = np.array(scores)
    res.scores = mean_over_replicas(res.all_scores.T) if len(losses) > 1 else res.all_scores[0]
    res.margin, res.tv = min(margins), tv
    res.rows = np.stack([np.rint(w.detach().numpy()).astype(np.int16) for w in rows])
    return res


def loss_and_grad(cfg, models, task, attack_type, audio, original, companions, r=1, tau=None, chain=(), normals=None, taps=None,
                  threshold=0.0, adver_thresh=0.0, target=0, true=0):
    """The GMM-UBM victim: the mean over the R replicas of whitebox_ref's loss.  normals / taps: lists over rho (None: no such
    stage).  -> Result with loss, grad [N], scores (the mean), margin (the smallest VAD margin), tv, rows (int16 [R][N])."""
    a = torch.tensor(np.asarray(audio, np.float64).reshape(-1), requires_grad=True)
    x = R.cast_st(a, 16)
    rows = compose(x, U.quantize(original), companions, r, tau)
    tab = R.Tables(cfg)
    losses, scores, margins, tv = [], [], [], []
    for rho, y in enumerate(rows):
        nz = None if normals is None else normals[rho]
        if taps is not None:
            y = AV.channel_defence(y, taps[rho], list(chain), None, nz)
        elif chain:
            y = B.defence(y, list(chain), None, nz)
        feats, _mask, margin = F.features(cfg, y, None, 0.0, tab)
        s = R.system_scores(task, R.gmm_raw(feats, *models), None, None)
        losses.append(R.loss_fn(task, attack_type, s, threshold, adver_thresh, target, true))
        scores.append(s.detach().numpy().copy())
        margins.append(margin)
        tv.append(feats.shape[0])
    return _finish(a, losses, scores, margins, tv, rows)


def loss_and_grad_iv(cfg, tab, task, attack_type, audio, original, companions, r=1, tau=None, chain=(), normals=None, taps=None,
                     sels=None, threshold=0.0, adver_thresh=0.0, target=0, true=0):
    """The same on the i-vector-PLDA victim (whitebox_iv_ref).  sels: per replica, the device's gselect on its voiced rows (None:
    the restatement's own).  The Result also carries reps, whitebox_iv_ref's per-replica Results."""
    sy = tab.sy
    a = torch.tensor(np.asarray(audio, np.float64).reshape(-1), requires_grad=True)
    x = R.cast_st(a, 16)
    rows = compose(x, U.quantize(original), companions, r, tau)
    tab_fe = R.Tables(cfg)
    losses, scores, margins, tv, reps = [], [], [], [], []
    for rho, y in enumerate(rows):
        nz = None if normals is None else normals[rho]
        if taps is not None:
            y = AV.channel_defence(y, taps[rho], list(chain), None, nz)
        elif chain:
            y = B.defence(y, list(chain), None, nz)
        feats, _mask, margin = F.features(cfg, y, None, 0.0, tab_fe)
        ex = V.ivector(tab, feats, None if sels is None else sels[rho])
        raw = V.backend_llr(tab, ex.ivec, bool(getattr(cfg, "text_scores", 0)), text_ivector=True)
        sc = (raw - torch.as_tensor(sy.z_mean)) / torch.as_tensor(sy.z_std)
        losses.append(R.loss_fn(task, attack_type, sc, threshold, adver_thresh, target, true))
        scores.append(sc.detach().numpy().copy())
        margins.append(margin)
        tv.append(feats.shape[0])
        reps.append(ex)
    res = _finish(a, losses, scores, margins, tv, rows)
    res.reps = reps
    return res
