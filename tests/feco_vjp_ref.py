"""Restatement of the white-box gradient THROUGH feature compression and dither (include/fakebob_hip.h, "Feature compression
and dither (fb_set_wb_frontend)"), written from the header's contract in PyTorch float64.  Test infrastructure only.

Both stages are differentiated with the forward's hard decisions held constant, so both decisions are ARGUMENTS here:
  dither   the float32 normals z[T][L] the forward drew for a replica (Engine.debug_dither_noise): the frames are
           (double) x + amp * (double) z, constants added to the extracted samples;
  FeCo     the final assignment labels[Tv] and k (tests/feco_ref.feco, or what the device kept): a centre with members is
           their mean, one without keeps a value handed in as a constant.
The front end, the back ends and the loss are tests/whitebox_ref.py's, the defences tests/bpda_ref.py's, the channel
tests/air_vjp_ref.py's, the i-vector victim tests/whitebox_iv_ref.py's; the gradient is autograd's."""
import numpy as np
import torch

from tests import air_vjp_ref as AV
from tests import bpda_ref as B
from tests import whitebox_iv_ref as V
from tests import whitebox_ref as R

F64 = torch.float64


class _Frames(object):
    """`cfg` as whitebox_ref.mfcc reads it when every frame is handed in as it was extracted, one after the other: frame f is
    samples f L .. f L + L - 1 (snip_edges, a shift of one frame length); everything else is cfg's"""

    def __init__(self, cfg):
        self._cfg = cfg
        self.snip_edges = 1
        self.frame_shift = cfg.frame_length

    def __getattr__(self, name):
        return getattr(self._cfg, name)


def mfcc(cfg, x, z=None, amp=0.0, tab=None):
    """whitebox_ref.mfcc of the row x with Kaldi's dither: the extracted frames (reflection included) plus amp * z, z [T][L]"""
    tab = tab or R.Tables(cfg)
    if z is None or amp == 0.0:
        return R.mfcc(cfg, x, tab)
    fr = x[torch.tensor(R.frame_index(cfg, x.shape[0]))]
    zz = torch.as_tensor(np.asarray(z, np.float32).astype(np.float64))
    assert zz.shape == fr.shape, (zz.shape, fr.shape)
    return R.mfcc(_Frames(cfg), (fr + float(amp) * zz).reshape(-1), tab)


def features(cfg, x, z=None, amp=0.0, tab=None):
    """whitebox_ref.features with the dithered MFCC -> (voiced rows [Tv][D], mask, min |c0 - thr|)"""
    tab = tab or R.Tables(cfg)
    mf = mfcc(cfg, x, z, amp, tab)
    mask, margin = R.vad_mask(cfg, mf)
    f = R.cmvn_sliding(cfg, R.add_deltas(cfg, mf, tab))
    return f[torch.tensor(mask)], mask, margin


def centres(feats, labels, k, empty=None):
    """C[j] = the mean of the rows t with labels[t] == j (float64; the float32 storage is the identity); a centre without members
    is row j of `empty` (k, D), a constant.  feats: tensor [Tv][D]; labels: ints [Tv]"""
    lab = torch.as_tensor(np.asarray(labels, np.int64))
    assert lab.shape[0] == feats.shape[0] and (k == 0 or int(lab.max()) < k)
    n = np.bincount(np.asarray(labels, np.int64), minlength=k)
    S = torch.zeros(k, feats.shape[1], dtype=F64).index_add(0, lab, feats)
    C = S / torch.as_tensor(np.maximum(n, 1).astype(np.float64))[:, None]
    if (n == 0).any():
        if empty is None:
            raise ValueError("centres %s have no members and no value was handed in" % np.flatnonzero(n == 0))
        C = torch.where(torch.as_tensor(n == 0)[:, None], torch.as_tensor(np.asarray(empty, np.float64)), C)
    return C


def gather_t(cbar, labels, k):
    """the transpose of `centres` in closed form: xbar[t] = cbar[labels[t]] / n[labels[t]] (numpy float64)"""
    labels = np.asarray(labels, np.int64)
    n = np.bincount(labels, minlength=k)
    return np.asarray(cbar, np.float64)[labels] / n[labels].astype(np.float64)[:, None]


def compressed(feats, fc):
    """fc: None (no compression) or a dict labels=, k=, empty= (optional) of one replica"""
    return feats if fc is None else centres(feats, fc["labels"], fc["k"], fc.get("empty"))


def loss_and_grad(cfg, models, task, attack_type, audio, feco=(None,), dither=(None,), amp=0.0, chain=(), codec=None, normals=None,
                  taps=None, bits=16, threshold=0.0, adver_thresh=0.0, target=0, true=0, z_mean=None, z_std=None, cast=True):
    """The EOT mean over r = len(feco) replicas of whitebox_ref's loss on the GMM-UBM victim behind (channel,) chain, codec,
    dithered front end and feature compression.  feco[j] / dither[j] / normals[j] / taps[j]: replica j's kept assignment, dither
    normals, noise-stage normals and room response.  -> Result with loss, grad [N], scores (the mean), losses, all_scores, margin,
    feats (per replica: the voiced rows, numpy)."""
    r = len(feco)
    dither = list(dither) if len(dither) == r else [dither[0]] * r
    normals = [None] * r if normals is None else normals
    a = torch.tensor(np.asarray(audio, np.float64).reshape(-1), requires_grad=True)
    x = R.cast_st(a, bits) if cast else a * float(2 ** (bits - 1))
    tab = R.Tables(cfg)
    losses, scores, margins, rows = [], [], [], []
    for j in range(r):
        if taps is not None:
            y = AV.channel_defence(x, taps[j], list(chain), codec, normals[j])
        elif chain or codec is not None:
            y = B.defence(x, list(chain), codec, normals[j])
        else:
            y = x
        feats, _mask, margin = features(cfg, y, dither[j], amp, tab)
        rows.append(feats.detach().numpy().copy())
        s = R.system_scores(task, R.gmm_raw(compressed(feats, feco[j]), *models), z_mean, z_std)
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
    res.scores = B.TN.eot_mean(res.all_scores.T) if r > 1 else res.all_scores[0]
    res.margin, res.feats = min(margins), rows
    return res


def loss_and_grad_iv(cfg, tab, task, attack_type, audio, feco=None, dither=None, amp=0.0, sel=None, bits=16, threshold=0.0,
                     adver_thresh=0.0, target=0, true=0, cast=True):
    """whitebox_iv_ref.loss_and_grad_iv with the dithered front end and the compression in front of the extractor (r = 1).
    sel: the device's gselect on the rows it scored (the centres).  -> its Result (+ feats: the voiced rows)."""
    if not isinstance(tab, V.IvTables):
        tab = V.IvTables(tab)
    sy = tab.sy
    a = torch.tensor(np.asarray(audio, np.float64).reshape(-1), requires_grad=True)
    x = R.cast_st(a, bits) if cast else a * float(2 ** (bits - 1))
    feats, mask, margin = features(cfg, x, dither, amp)
    ex = V.ivector(tab, compressed(feats, feco), sel)
    raw = V.backend_llr(tab, ex.ivec, cast and bool(getattr(cfg, "text_scores", 0)), text_ivector=cast)
    s = (raw - torch.as_tensor(sy.z_mean)) / torch.as_tensor(sy.z_std)
    l = R.loss_fn(task, attack_type, s, threshold, adver_thresh, target, true)
    l.backward()
    r = V.Result()
    r.grad, r.loss = a.grad.numpy().copy(), float(l.detach())
    r.scores, r.raw = s.detach().numpy().copy(), raw.detach().numpy().copy()
    r.mask, r.margin, r.tv = mask, margin, int(mask.sum())
    r.sel, r.own_sel, r.gsel_gap, r.prune_margin, r.keep = ex.sel, ex.own_sel, ex.gsel_gap, ex.prune_margin, ex.keep
    r.feats = feats.detach().numpy().copy()
    return r
