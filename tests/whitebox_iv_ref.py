"""The white-box reference for the i-vector-PLDA victim: the function fb_get_grad_wb differentiates once
fb_set_wb_ivector is on, restated in PyTorch float64 on the CPU.

TEST INFRASTRUCTURE ONLY.  Written from SURVEY.md A.9 / A.10 and the i-vector part of the "white-box gradients" contract
of include/fakebob_hip.h; the front end is tests/whitebox_ref.py's.  The gradient comes from autograd only.

 - gmm-gselect and the --min-post kept set are DECIDED from the forward's values rounded the way the oracle rounds them
   (float32 diagonal log-likelihoods ranked by (value, index) descending; float32 full-covariance ll; float32 posteriors
   against the float32 min_post) and then held constant; `sel=` takes a selection handed in instead;
 - on the kept set the posterior is the soft-max of the float64 log-likelihoods restricted to it; a frame whose posteriors
   all fell below min_post keeps its first-maximum slot at a constant 1;
 - the float32 storage points are identities: the values are NOT rounded (the i-vector's float32 text form and text_scores,
   which move the forward's value, are straight-through roundings);
 - two fixture margins come back: gsel_gap [Tv] (diagonal ll at rank nsel minus rank nsel + 1; +inf where C <= nsel) and
   prune_margin (min |p - min_post| over all selected slots; +inf without pruning).
U and Sigma^-1 M are built for the components with posterior mass only, so a recipe-size system fits in memory.
`iv_feat_grad` and `backend_grad` are the plain-numpy closed forms of the contract's backward: the readable statement of
the formulas the kernels implement, checked against autograd in tests/test_whitebox_iv_ref_host.py.
"""
import math

import numpy as np
import torch

from tests import whitebox_ref as W

F64 = torch.float64
LOG2PI = 1.8378770664093454835606594728112


class IvTables(object):
    """Derived variables of a models.IvectorSystem, numpy float64 unless said (fgmm-global-to-gmm, FullGmm gconsts)."""

    def __init__(self, sy):
        f32, f64 = np.float32, np.float64
        C, D, R = sy.C, sy.D, sy.R
        self.sy, self.C, self.D, self.R, self.L, self.S = sy, C, D, R, sy.L, sy.S
        r, c = np.tril_indices(D)
        P = np.zeros((C, D, D), f64)
        P[:, r, c] = sy.fg_inv_covars.astype(f64)
        P[:, c, r] = sy.fg_inv_covars.astype(f64)
        self.P = P
        covar = np.linalg.inv(P)
        self.mic = sy.fg_means_invcovars.astype(f64)
        mean = np.einsum("kde,ke->kd", covar, self.mic)
        var = np.einsum("kdd->kd", covar)
        w = sy.fg_weights.astype(f64)
        self.dg_iv = (1.0 / var).astype(f32)
        self.dg_miv = (mean * (1.0 / var)).astype(f32)
        iv64, miv64 = self.dg_iv.astype(f64), self.dg_miv.astype(f64)
        self.dg_gc = (np.log(w) - 0.5 * D * np.log(2 * np.pi) + 0.5 * np.log(iv64).sum(1)
                      - 0.5 * (miv64 * miv64 / iv64).sum(1)).astype(f32)
        _, logdet = np.linalg.slogdet(P)
        self.fg_gc = (np.log(w) - 0.5 * (D * np.log(2 * np.pi) - logdet + np.einsum("kd,kd->k", self.mic, mean))).astype(f32).astype(f64)
        self.tri = (r, c)
        self.mean_vec = sy.mean_vec.astype(f64)
        self.lda = sy.lda.astype(f64)
        self.train = np.stack([self.backend_np(sy.enrolled[s].astype(f64)) for s in range(sy.S)])

    def sim_u(self, comps):
        """(Sigma^-1 M) [n][D][R] and U [n][R][R] (full, symmetric) of the listed components."""
        sy, D = self.sy, self.D
        r, c = self.tri
        Sinv = np.zeros((len(comps), D, D))
        Sinv[:, r, c] = sy.ie_sigma_inv[comps]
        Sinv[:, c, r] = sy.ie_sigma_inv[comps]
        sim = np.matmul(Sinv, sy.ie_M[comps])
        return sim, np.matmul(sy.ie_M[comps].transpose(0, 2, 1), sim)

    def backend_np(self, ivec):
        """The back end's forward in numpy (fbo_iv_backend's arithmetic): raw i-vector [R] -> PLDA-space y [L]."""
        sy, R, L = self.sy, self.R, self.L
        x = ivec.astype(np.float32).astype(np.float64) - self.mean_vec
        z = self.lda[:, :R] @ x + (self.lda[:, R] if self.lda.shape[1] == R + 1 else 0.0)
        nrm = math.sqrt(float(z @ z))
        if nrm != 0.0:
            z = z * (math.sqrt(L) / nrm)
        y0 = sy.plda_transform @ (z - sy.plda_mean)
        return y0 * math.sqrt(L / float((y0 * y0 / (sy.plda_psi + 1.0)).sum()))


# ------------------------------------------------------------------------------------------------ the extractor
def gselect(tab, feats32):
    """gmm-gselect on the diagonalised UBM with the oracle's roundings: feats32 [Tv][D] float32 -> (sel [Tv][n] int,
    gsel_gap [Tv])."""
    f = np.asarray(feats32, np.float32)
    xd = f.astype(np.float64)
    xq = (f * f).astype(np.float32).astype(np.float64)
    v = (tab.dg_gc.astype(np.float64)[None, :] + xd @ tab.dg_miv.astype(np.float64).T
         - 0.5 * (xq @ tab.dg_iv.astype(np.float64).T)).astype(np.float32)
    C, n = tab.C, min(tab.sy.num_gselect, tab.C)
    # descending by (value, index), std::greater<pair<float, int>>
    order = np.lexsort((-np.arange(C)[None, :].repeat(v.shape[0], 0), -v.astype(np.float64)), axis=1)
    sel = order[:, :n]
    sv = np.take_along_axis(v, order, axis=1).astype(np.float64)
    gap = sv[:, n - 1] - sv[:, n] if C > n else np.full(v.shape[0], np.inf)
    return sel.astype(np.int64), gap


def full_ll(tab, x, sel):
    """ll[t][j] = gconst_k + (Sigma_k^-1 mu_k) . x_t - 1/2 x_t' Sigma_k^-1 x_t, k = sel[t][j]; x a float64 tensor [Tv][D]."""
    out = []
    P, mic, gc = torch.as_tensor(tab.P), torch.as_tensor(tab.mic), torch.as_tensor(tab.fg_gc)
    for t0 in range(0, x.shape[0], 16):
        xs, ks = x[t0:t0 + 16], torch.as_tensor(sel[t0:t0 + 16])
        Px = torch.einsum("tjde,te->tjd", P[ks], xs)
        out.append(gc[ks] + torch.einsum("tjd,td->tj", mic[ks], xs) - 0.5 * torch.einsum("tjd,td->tj", Px, xs))
    return torch.cat(out, dim=0)


def kept_posteriors(tab, ll):
    """The forward's decisions on float32 values: ll float64 numpy [Tv][n] -> (keep [Tv][n] bool, rescue [Tv] int (-1: none;
    else the slot set to 1), prune_margin)."""
    l32 = ll.astype(np.float32).astype(np.float64)
    e = np.exp(l32 - l32.max(axis=1, keepdims=True))
    p = (e / e.sum(axis=1, keepdims=True)).astype(np.float32)
    mp = np.float32(tab.sy.min_post)
    Tv, n = p.shape
    if mp == 0.0:
        return np.ones((Tv, n), bool), np.full(Tv, -1), float("inf")
    keep = ~(p < mp)
    rescue = np.where(keep.any(axis=1), -1, np.argmax(p, axis=1))
    return keep, rescue, float(np.abs(p.astype(np.float64) - float(mp)).min())


class Result(object):
    pass


def ivector(tab, feats, sel=None):
    """feats: float64 tensor [Tv][D] (may require grad) -> Result: ivec (tensor [R], the raw i-vector w - prior e0), sel,
    own_sel, gsel_gap, prune_margin, keep, gamma (tensor [Tv][n]), and what the closed form needs: active (the components with
    posterior mass), sim, U, quad, w."""
    sy = tab.sy
    f32 = feats.detach().numpy().astype(np.float32)
    own_sel, gap = gselect(tab, f32)
    sel = own_sel if sel is None else np.asarray(sel, np.int64)
    ll = full_ll(tab, feats, sel)
    keep, rescue, margin = kept_posteriors(tab, ll.detach().numpy())
    masked = torch.where(torch.as_tensor(keep), ll, torch.full_like(ll, -float("inf")))
    res_rows = rescue >= 0
    if res_rows.any():   # a constant posterior: one slot at 1
        masked = masked.clone()
        onehot = torch.full_like(ll, -float("inf"))
        onehot[torch.as_tensor(np.nonzero(res_rows)[0]), torch.as_tensor(rescue[res_rows])] = 0.0
        masked = torch.where(torch.as_tensor(res_rows)[:, None], onehot, masked)
    gamma = torch.softmax(masked, dim=1)
    g_np = gamma.detach().numpy()
    active = np.unique(sel[g_np > 0.0])
    pos = np.full(tab.C, -1, np.int64)
    pos[active] = np.arange(active.size)
    idx = torch.as_tensor(np.where(g_np > 0.0, pos[sel], 0))
    gm = torch.where(torch.as_tensor(g_np > 0.0), gamma, torch.zeros_like(gamma))
    Nk = torch.zeros(active.size, dtype=F64).index_add(0, idx.reshape(-1), gm.reshape(-1))
    Fk = torch.zeros(active.size, tab.D, dtype=F64).index_add(
        0, idx.reshape(-1), (gm[:, :, None] * feats[:, None, :]).reshape(-1, tab.D))
    sim, U = tab.sim_u(active)
    lin = torch.einsum("kdr,kd->r", torch.as_tensor(sim), Fk)
    e0 = torch.zeros(tab.R, dtype=F64)
    e0[0] = sy.prior_offset
    quad = torch.eye(tab.R, dtype=F64) + torch.einsum("k,kij->ij", Nk, torch.as_tensor(U))
    w = torch.linalg.solve(quad, lin + e0)
    r = Result()
    r.ivec, r.sel, r.own_sel, r.gsel_gap, r.prune_margin = w - e0, sel, own_sel, gap, margin
    r.gamma, r.active, r.sim, r.U, r.quad, r.w, r.keep = gamma, active, sim, U, quad, w, keep
    return r


# ------------------------------------------------------------------------------------------------ the back end
def _round6(v):
    return float("%.6g" % np.float32(v))


def backend_llr(tab, ivec, text_scores=False, text_ivector=True):
    """raw i-vector (tensor [R]) -> raw LLRs (tensor [S]) against the enrolled speakers, n = 1.  text_ivector: the i-vector
    takes the float32 value ivector-extract writes (straight-through); text_scores likewise for the six digits of a score."""
    sy, R, L = tab.sy, tab.R, tab.L
    iv = ivec
    if text_ivector:
        iv = ivec + (torch.as_tensor(ivec.detach().numpy().astype(np.float32).astype(np.float64)) - ivec.detach())
    x = iv - torch.as_tensor(tab.mean_vec)
    lda = torch.as_tensor(tab.lda)
    z = lda[:, :R] @ x
    if lda.shape[1] == R + 1:
        z = z + lda[:, R]
    nrm = torch.sqrt((z * z).sum())
    if float(nrm.detach()) != 0.0:
        z = z * (math.sqrt(L) / nrm)
    y0 = torch.as_tensor(sy.plda_transform) @ (z - torch.as_tensor(sy.plda_mean))
    psi = torch.as_tensor(sy.plda_psi)
    y = y0 * torch.sqrt(L / (y0 * y0 / (psi + 1.0)).sum())
    tr = torch.as_tensor(tab.train)
    mean = psi / (psi + 1.0) * tr
    var = 1.0 + psi / (psi + 1.0)
    given = -0.5 * ((torch.log(var) + (y[None, :] - mean) ** 2 / var).sum(dim=1) + LOG2PI * L)
    without = -0.5 * ((torch.log(psi + 1.0) + y * y / (psi + 1.0)).sum() + LOG2PI * L)
    llr = given - without
    if text_scores:
        llr = llr + (torch.tensor([_round6(v) for v in llr.detach().numpy()], dtype=F64) - llr.detach())
    return llr


def loss_and_grad_iv(cfg, tab, task, attack_type, audio, bits=16, threshold=0.0, adver_thresh=0.0, target=0, true=0,
                     want_grad=True, cast=True, sel=None):
    """tab: IvTables (or a models.IvectorSystem).  -> Result with loss, grad (d loss / d audio, numpy [N]), scores, raw, ivec,
    mask, margin (VAD), tv, sel, own_sel, gsel_gap, prune_margin, keep (the kept set, [Tv][n] bool)."""
    if not isinstance(tab, IvTables):
        tab = IvTables(tab)
    sy = tab.sy
    a = torch.tensor(np.asarray(audio, np.float64).reshape(-1), requires_grad=want_grad)
    x = W.cast_st(a, bits) if cast else a * float(2 ** (bits - 1))
    feats, mask, margin = W.features(cfg, x)
    ex = ivector(tab, feats, sel)
    # (cast=False is the real-valued function a finite difference is taken of: no value is replaced by a rounded one)
    raw = backend_llr(tab, ex.ivec, cast and bool(getattr(cfg, "text_scores", 0)), text_ivector=cast)
    s = (raw - torch.as_tensor(sy.z_mean)) / torch.as_tensor(sy.z_std)   # every task z-normalises
    l = W.loss_fn(task, attack_type, s, threshold, adver_thresh, target, true)
    r = Result()
    r.grad = None
    if want_grad:
        l.backward()
        r.grad = a.grad.numpy().copy()
    r.loss, r.scores, r.raw = float(l.detach()), s.detach().numpy().copy(), raw.detach().numpy().copy()
    r.ivec = ex.ivec.detach().numpy().copy()
    r.mask, r.margin, r.tv = mask, margin, int(mask.sum())
    r.sel, r.own_sel, r.gsel_gap, r.prune_margin, r.keep = ex.sel, ex.own_sel, ex.gsel_gap, ex.prune_margin, ex.keep
    r.feats = feats.detach().numpy().copy()
    return r


# ------------------------------------------------------------------------------------------------ the two hooks' references
def backend_grad_autograd(tab, ivec, w):
    """d (sum_s w_s LLR_s) / d ivec by autograd -> numpy [R]."""
    v = torch.tensor(np.asarray(ivec, np.float64), requires_grad=True)
    (backend_llr(tab, v) * torch.as_tensor(np.asarray(w, np.float64))).sum().backward()
    return v.grad.numpy().copy()


def feat_grad_autograd(tab, feats, cot, sel=None):
    """d <cot, ivec(feats)> / d feats by autograd -> (numpy [Tv][D], the forward's Result)."""
    x = torch.tensor(np.asarray(feats, np.float64), requires_grad=True)
    ex = ivector(tab, x, sel)
    (ex.ivec * torch.as_tensor(np.asarray(cot, np.float64))).sum().backward()
    return x.grad.numpy().copy(), ex


def backend_grad(tab, ivec, w):
    """The closed form of the back end's backward in numpy float64 (the stages of k_wb_iv_backend_t)."""
    sy, R, L = tab.sy, tab.R, tab.L
    psi = sy.plda_psi
    x = np.asarray(ivec, np.float64).astype(np.float32).astype(np.float64) - tab.mean_vec
    z0 = tab.lda[:, :R] @ x + (tab.lda[:, R] if tab.lda.shape[1] == R + 1 else 0.0)
    n2 = float(z0 @ z0)
    a1 = math.sqrt(L) / math.sqrt(n2) if n2 != 0.0 else 1.0
    y0 = sy.plda_transform @ (a1 * z0 - sy.plda_mean)
    dot = float((y0 * y0 / (psi + 1.0)).sum())
    nf = math.sqrt(L / dot)
    y = nf * y0
    var = 1.0 + psi / (psi + 1.0)
    gy = np.zeros(L)
    for s in range(sy.S):
        gy += w[s] * (y / (psi + 1.0) - (y - psi / (psi + 1.0) * tab.train[s]) / var)
    gy0 = nf * (gy - float(gy @ y0) / dot * y0 / (psi + 1.0))
    gz = sy.plda_transform.T @ gy0
    gz0 = a1 * (gz - z0 * float(gz @ z0) / n2) if n2 != 0.0 else gz
    return tab.lda[:, :R].T @ gz0


def iv_feat_grad(tab, feats, cot, ex):
    """The closed form of the extractor's backward in numpy float64, from the forward `ex` (ivector()'s Result: sel, gamma,
    active, sim, U, quad, w):
        lambda = quad^-1 cot;  Fbar_k = A_k lambda;  Nbar_k = - lambda' U_k w
        gammabar_tk = Nbar_k + Fbar_k . x_t;  llbar_tk = gamma_tk (gammabar_tk - sum_j gamma_tj gammabar_tj)
        xbar_t = sum_k gamma_tk Fbar_k + sum_k llbar_tk (Sigma_k^-1 mu_k - Sigma_k^-1 x_t)
    (a rescued frame's posterior is constant: its llbar is zero because its one gamma is 1)."""
    x = np.asarray(feats, np.float64)
    g = ex.gamma.detach().numpy()
    lam = np.linalg.solve(ex.quad.detach().numpy(), np.asarray(cot, np.float64))
    w = ex.w.detach().numpy()
    Fbar = np.zeros((tab.C, tab.D))
    Nbar = np.zeros(tab.C)
    Fbar[ex.active] = ex.sim @ lam
    Nbar[ex.active] = -np.einsum("i,kij,j->k", lam, ex.U, w)
    out = np.zeros_like(x)
    for t in range(x.shape[0]):
        ks = ex.sel[t]
        gb = Nbar[ks] + Fbar[ks] @ x[t]
        gb = np.where(g[t] > 0.0, gb, 0.0)
        llb = g[t] * (gb - float(g[t] @ gb))
        out[t] = g[t] @ Fbar[ks]
        for j, k in enumerate(ks):
            if llb[j] != 0.0:
                out[t] += llb[j] * (tab.mic[k] - tab.P[k] @ x[t])
    return out
