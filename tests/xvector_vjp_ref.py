"""The white-box reference for the x-vector (TDNN) victim: the function fb_get_grad_wb differentiates once fb_set_wb_xvector
is on, restated in PyTorch on the CPU.

TEST INFRASTRUCTURE ONLY.  Built from tests/xvector_ref.py (the frame layer, pooling) and tests/whitebox_ref.py (the cast, the
front end, loss_fn); the gradient comes from autograd only.

 - the frame layers run in `frame_dtype`: torch.float64, or torch.float32 with the feature rows rounded to float32 first -- what
   a float32 implementation of the same function gives; pooling, the segment affine and the back end are float64;
 - with `masks` given (one (T, dout) array of 0 / 1 per layer) a layer's value is still clamp(z, 0), but its derivative comes
   from the mask: clamp(z, 0).detach() + mask * (z - z.detach()) -- the forward's own decisions held constant;
 - the variance floor is torch.clamp: an active floor passes nothing;
 - the embedding's rounding to float32 in front of the back end is straight-through.
`system` is anything with models.XvectorSystem's attributes."""
import math

import numpy as np
import torch

from tests import whitebox_ref as W
from tests import xvector_ref as X

F64 = torch.float64
LOG2PI = 1.8378770664093454835606594728112


class Result(object):
    pass


def frame_layer(h, ly, dtype, mask=None):
    """xvector_ref.frame_layer with the pre-activation returned and, with `mask`, the ReLU's derivative taken from it"""
    T = h.shape[0]
    idx = torch.from_numpy(X.splice_index(T, ly["ctx"]))
    sp = h[idx].reshape(T, -1)
    z = sp @ torch.from_numpy(ly["W"]).to(dtype).T + torch.from_numpy(ly["bias"]).to(dtype)
    a = torch.clamp(z, min=0)
    if mask is not None:
        m = torch.as_tensor(np.asarray(mask, np.float64)).to(dtype)
        a = a.detach() + m * (z - z.detach())
    return torch.from_numpy(ly["bn_scale"]).to(dtype) * a + torch.from_numpy(ly["bn_offset"]).to(dtype), z


def embed(system, x, frame_dtype=F64, masks=None):
    """x: float64 tensor (T, D) -> Result: emb (tensor (R,), float64), stats (tensor (2 P,)), hs (the layers' inputs and the
    last output: n_layers + 1 tensors of frame_dtype, hs[0] the rows as the layers read them), zs (pre-activations), var (the
    pooled E[h^2] - mean^2, numpy)"""
    r = Result()
    h = x.to(frame_dtype)
    r.hs, r.zs = [h], []
    for l, ly in enumerate(system.layers):
        h, z = frame_layer(h, ly, frame_dtype, None if masks is None else masks[l])
        r.hs.append(h)
        r.zs.append(z)
    h64 = h.to(F64)
    r.stats = X.pool(h64)
    with torch.no_grad():
        mean = h64.mean(dim=0)
        r.var = ((h64 * h64).mean(dim=0) - mean * mean).numpy().copy()
    r.emb = torch.from_numpy(system.seg_W).to(F64) @ r.stats + torch.from_numpy(system.seg_bias).to(F64)
    return r


def feat_grad(system, x, ebar, frame_dtype=F64, masks=None):
    """d <ebar, emb(x)> / d every stage for one utterance x (T, D) -> Result: grads, a list of float64 numpy arrays indexed as
    fb_debug_xv_backward's stages (0: the feature rows; l: the input of layer l; n_layers: the last layer's output;
    n_layers + 1: the statistics), and emb, stats, zs (numpy, float64), var."""
    xt = torch.tensor(np.asarray(x, np.float32).astype(np.float64), requires_grad=True)
    f = embed(system, xt, frame_dtype, masks)
    for h in f.hs[1:]:
        h.retain_grad()
    f.stats.retain_grad()
    (f.emb * torch.as_tensor(np.asarray(ebar, np.float64))).sum().backward()
    r = Result()
    r.grads = [xt.grad.numpy().copy()] + [h.grad.to(F64).numpy().copy() for h in f.hs[1:]] + [f.stats.grad.numpy().copy()]
    r.emb, r.stats, r.var = f.emb.detach().numpy().copy(), f.stats.detach().numpy().copy(), f.var
    r.zs = [z.detach().to(F64).numpy().copy() for z in f.zs]
    return r


def backend_llr(system, emb, straight_through=True):
    """the embedding (tensor (R,)) -> raw LLRs (tensor (S,)) against system.enrolled, n = 1: - mean_vec, LDA, length
    normalisation, PLDA transform and normalisation, the closed-form LLR (xvector_ref.plda_llr in torch float64)"""
    R, L = system.R, system.L
    v = emb
    if straight_through:
        v = emb + (torch.as_tensor(emb.detach().numpy().astype(np.float32).astype(np.float64)) - emb.detach())
    x = v - torch.as_tensor(system.mean_vec.astype(np.float64))
    lda = torch.as_tensor(system.lda.astype(np.float64))
    z = lda[:, :R] @ x
    if lda.shape[1] == R + 1:
        z = z + lda[:, R]
    nrm = torch.sqrt((z * z).sum())
    if float(nrm.detach()) != 0.0:
        z = z * (math.sqrt(L) / nrm)
    psi = torch.as_tensor(np.asarray(system.plda_psi, np.float64))
    y0 = torch.as_tensor(np.asarray(system.plda_transform, np.float64)) @ (z - torch.as_tensor(np.asarray(system.plda_mean, np.float64)))
    y = y0 * torch.sqrt(L / (y0 * y0 / (psi + 1.0)).sum())
    tr = torch.as_tensor(np.stack([X.backend_transform(system, e) for e in system.enrolled]))
    mean = psi / (psi + 1.0) * tr
    var = 1.0 + psi / (psi + 1.0)
    given = -0.5 * ((torch.log(var) + (y[None, :] - mean) ** 2 / var).sum(dim=1) + LOG2PI * L)
    without = -0.5 * ((torch.log(psi + 1.0) + y * y / (psi + 1.0)).sum() + LOG2PI * L)
    return given - without


def loss_from_feats(system, task, attack_type, feats, frame_dtype=F64, masks=None, threshold=0.0, adver_thresh=0.0, target=0, true=0,
                    straight_through=True):
    """feats: float64 tensor (Tv, D) -> (loss tensor, scores tensor (S,), raw tensor (S,), embed()'s Result)"""
    f = embed(system, feats, frame_dtype, masks)
    raw = backend_llr(system, f.emb, straight_through)
    s = (raw - torch.as_tensor(np.asarray(system.z_mean, np.float64))) / torch.as_tensor(np.asarray(system.z_std, np.float64))
    return W.loss_fn(task, attack_type, s, threshold, adver_thresh, target, true), s, raw, f


def loss_and_grad_xv(cfg, system, task, attack_type, audio, bits=16, threshold=0.0, adver_thresh=0.0, target=0, true=0,
                     frame_dtype=F64, masks=None, want_grad=True, cast=True, feats=None):
    """-> Result with loss, grad (d loss / d audio, numpy [N]), scores, raw, emb, mask (VAD), margin, tv, feats (numpy), zs, var.
    cast=False: the real-valued function itself (no truncation, no rounding of the embedding): what a finite difference can be
    taken of.  feats (numpy (Tv, D), optional): the feature rows take these VALUES, straight-through -- the front end's
    Jacobian stays the restatement's, the TDNN is evaluated where another front end put the rows."""
    a = torch.tensor(np.asarray(audio, np.float64).reshape(-1), requires_grad=want_grad)
    x = W.cast_st(a, bits) if cast else a * float(2 ** (bits - 1))
    ft, mask, margin = W.features(cfg, x)
    if feats is not None:
        ft = ft + (torch.as_tensor(np.asarray(feats, np.float64)) - ft.detach())
    l, s, raw, f = loss_from_feats(system, task, attack_type, ft, frame_dtype, masks, threshold, adver_thresh, target, true, cast)
    r = Result()
    r.grad = None
    if want_grad:
        l.backward()
        r.grad = a.grad.numpy().copy()
    r.loss, r.scores, r.raw = float(l.detach()), s.detach().numpy().copy(), raw.detach().numpy().copy()
    r.emb = f.emb.detach().numpy().copy()
    r.mask, r.margin, r.tv = mask, margin, int(mask.sum())
    r.feats = ft.detach().numpy().copy()
    r.zs = [z.detach().to(F64).numpy().copy() for z in f.zs]
    r.var = f.var
    return r


def mask_conditions(zs, masks, var, edge=1e-4):
    """The fixture's conditions on one utterance or batch: zs / masks per layer (rows, dout) -- the float64 restatement's
    pre-activations and the masks under test --, var the pooled variances.  -> (flips on units with |z| >= edge * max |z| of
    their layer, the fraction of units below that margin, variances inside (1e-12, 1e-8))"""
    flips, near, total = 0, 0, 0
    for z, m in zip(zs, masks):
        big = np.abs(z) >= edge * np.abs(z).max()
        flips += int(np.sum((z > 0)[big] != (np.asarray(m) != 0)[big]))
        near += int(np.sum(~big))
        total += z.size
    v = np.asarray(var)
    return flips, near / float(total), int(np.sum((v > 1e-12) & (v < 1e-8)))
