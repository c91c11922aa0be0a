"""The host references of the masking attack (the "masking" contract of include/fakebob_hip.h):
  threshold_ref   the threshold model restated independently of fakebob_amd/masking.py -- plain loops, an explicit DFT, one frame
                  and one masker at a time;
  loss            D, n_over, gd = dD/d delta and P in PyTorch float64 with autograd (torch.fft.rfft, or an explicit DFT matrix:
                  the two against each other are the reference's own error, from which the device's bar is taken);
  control / adam_step   k_psy_ctl's decisions and k_psy_step's update in numpy, written as the contract writes them;
  replay          fb_attack_psy on the host in the manner of cw2_ref.replay: the engine's g, this file's gd.
"""
import math

import numpy as np

from tests import cw2_ref as C2

TEN_96 = 10.0 ** 9.6


def frames_of(n, W):
    hop = W // 4
    return 1 if n == W else -(-(n - W) // hop) + 1


def _dft_matrix(W):
    """exp(-2 pi i k n / W) for k <= W/2, the angle reduced modulo W in integers first"""
    kn = (np.arange(W // 2 + 1)[:, None] * np.arange(W)[None, :]) % W
    ang = 2.0 * np.pi * kn.astype(np.float64) / float(W)
    return np.cos(ang), -np.sin(ang)


def power_ref(v, W):
    """p(v) [F, K] by the explicit DFT, frame by frame"""
    v = np.asarray(v, np.float64).reshape(-1)
    F, hop = frames_of(v.size, W), W // 4
    h = np.array([0.5 - 0.5 * math.cos(2.0 * math.pi * n / W) for n in range(W)])
    cr, ci = _dft_matrix(W)
    p = np.zeros((F, W // 2 + 1))
    for f in range(F):
        fr = np.zeros(W)
        seg = v[f * hop:f * hop + W]
        fr[:seg.size] = seg
        fr = fr * h
        xr, xi = cr @ fr, ci @ fr
        p[f] = (8.0 / 3.0) * (xr * xr + xi * xi) / float(W * W)
    return p


def threshold_ref(a0, fs, W):
    """-> (theta [F, K], psd_max, maskers: per frame the list of (bin, level))"""
    p = power_ref(a0, W)
    psd_max = float(p.max())
    if not psd_max > 0.0:
        raise ValueError("silence")
    F, K = p.shape
    z, ath = [], []
    for k in range(K):
        fr = k * float(fs) / W
        zk = 13.0 * math.atan(0.00076 * fr) + 3.5 * math.atan((fr / 7500.0) ** 2)
        z.append(zk)
        if zk > 1.0:
            q = fr / 1000.0
            ath.append(3.64 * q ** -0.8 - 6.5 * math.exp(-0.6 * (q - 3.3) ** 2) + 1e-3 * q ** 4 - 12.0)
        else:
            ath.append(-math.inf)
    theta = np.zeros((F, K))
    maskers = []
    for f in range(F):
        psd = [96.0 + 10.0 * math.log10(p[f, k] / psd_max + 1e-20) for k in range(K)]
        kept = []
        for k in range(1, K - 1):
            if not (psd[k] > psd[k - 1] and psd[k] > psd[k + 1]):
                continue
            L = 10.0 * math.log10(10.0 ** (psd[k - 1] / 10.0) + 10.0 ** (psd[k] / 10.0) + 10.0 ** (psd[k + 1] / 10.0))
            if L < ath[k]:
                continue
            if kept and z[k] - z[kept[-1][0]] < 0.5:
                if L > kept[-1][1]:
                    kept[-1] = (k, L)
            else:
                kept.append((k, L))
        maskers.append(kept)
        for k in range(K):
            t = 0.0
            for j, L in kept:
                dz = z[k] - z[j]
                sf = 27.0 * dz if dz <= 0.0 else (-27.0 + 0.37 * max(L - 40.0, 0.0)) * dz
                t += 10.0 ** ((L - 6.025 - 0.275 * z[j] + sf) / 10.0)
            theta[f, k] = t + (10.0 ** (ath[k] / 10.0) if ath[k] > -math.inf else 0.0)
    return theta, psd_max, maskers


def loss(delta, theta, psd_max, W, dft=False):
    """The loss of the contract in PyTorch float64 -> dict(D, n_over, gd [N], P [F, K], margin = min |P - theta| / theta)"""
    import torch
    d = torch.tensor(np.asarray(delta, np.float64).reshape(-1), dtype=torch.float64, requires_grad=True)
    N = d.numel()
    F, hop, K = frames_of(N, W), W // 4, W // 2 + 1
    ext = torch.cat([d, torch.zeros((F - 1) * hop + W - N, dtype=torch.float64)])
    fr = ext.unfold(0, W, hop)
    assert fr.shape == (F, W)
    h = 0.5 - 0.5 * torch.cos(2.0 * math.pi * torch.arange(W, dtype=torch.float64) / W)
    fr = fr * h
    if dft:
        cr, ci = _dft_matrix(W)
        xr, xi = fr @ torch.tensor(cr).T, fr @ torch.tensor(ci).T
    else:
        X = torch.fft.rfft(fr, dim=1)
        xr, xi = X.real, X.imag
    P = (8.0 / 3.0) * (xr * xr + xi * xi) / float(W * W) * (TEN_96 / float(psd_max))
    th = torch.tensor(np.asarray(theta, np.float64))
    D = torch.clamp(P - th, min=0.0).sum() / float(F * K)
    D.backward()
    Pn = P.detach().numpy()
    return dict(D=float(D.detach()), n_over=int((Pn > theta).sum()), gd=d.grad.numpy().copy(), P=Pn,
                margin=float(np.min(np.abs(Pn - theta) / theta)))


def control(adver_loss, l2, D, l2_weight, c, gbest_dist, t, prev, abort_every):
    """k_psy_ctl's decisions -> dict(gate, take, found, gbest_dist, dist, L, abort, prev)"""
    dist = D + l2_weight * l2
    gate = 1 if adver_loss > 0 else 0
    L = (c * gate) * adver_loss + dist
    take = bool(adver_loss < 0 and dist < gbest_dist)
    abort = False
    if abort_every > 0 and t % abort_every == 0:
        if L > 0.9999 * prev:
            abort = True
        else:
            prev = L
    return dict(gate=gate, take=int(take), found=bool(adver_loss < 0), gbest_dist=dist if take else gbest_dist, dist=dist, L=L,
                abort=abort, prev=prev)


def adam_step(g, gd, x, a0, w0, mod, m1, m2, c, gate, l2_weight, p1, p2, lr=1e-2, beta1=0.9, beta2=0.999, adam_eps=1e-8):
    """k_psy_step's update -> (mod, m1, m2, x_next)"""
    G = (((c * gate) * g + gd) + l2_weight * (2.0 * (x - a0))) * (1.0 - x * x)
    m1 = beta1 * m1 + (1.0 - beta1) * G
    m2 = beta2 * m2 + ((1.0 - beta2) * G) * G
    mod = mod - ((lr / (1.0 - p1)) * m1) / (np.sqrt(m2) / math.sqrt(1.0 - p2) + adam_eps)
    return mod, m1, m2, np.tanh(w0 + mod)


def replay(eng, p, q, m, audio):
    """fb_attack_psy on the host: the contract's pseudo-code, g from Engine.get_grad_wb_iter(p, x, epoch) and D, n_over, gd from
    loss() at every iterate -> dict like Engine.attack_psy's, plus min_margin (cw2_ref.replay's: the distance of any iterate's
    sample from an int16 rounding boundary, LSB) and min_theta_margin (the smallest |P - theta| / theta met)"""
    a0 = np.asarray(audio, np.float64).reshape(-1)
    bits = p.bits_per_sample or 16
    theta, psd_max, W, lw = m._theta, m.psd_max, m.window, m.l2_weight
    w0 = C2.w0_of(a0)
    c, lo, hi = q.initial_const, 0.0, 1e10
    gbest, gbest_l2, gbest_no, gbest_row, gbest_x = float("inf"), float("inf"), 0, C2.cast_i16(a0, bits), a0.copy()
    rows, per, margin, tmargin = [], [], float("inf"), float("inf")
    for s in range(q.search_steps):
        mod, m1, m2 = np.zeros_like(a0), np.zeros_like(a0), np.zeros_like(a0)
        x = np.tanh(w0)
        p1 = p2 = 1.0
        prev, found, n_rows = float("inf"), False, 0
        for t in range(p.max_iter):
            epoch = s * p.max_iter + t
            scaled = x * float(2 ** (bits - 1))
            near = np.round(scaled)
            margin = min(margin, float(np.min(np.where(near == 0.0, 1.0 - np.abs(scaled), np.abs(scaled - near)))))
            g, al, sc = eng.get_grad_wb_iter(p, x, epoch)
            l2 = C2.l2_blocks(x, a0)
            ls = loss(x - a0, theta, psd_max, W)
            tmargin = min(tmargin, ls["margin"])
            d = control(al, l2, ls["D"], lw, c, gbest, t, prev, q.abort_every)
            rows.append([d["dist"], l2, float(ls["n_over"]), al, c] + list(sc))
            n_rows += 1
            if d["take"]:
                gbest, gbest_l2, gbest_no, gbest_row, gbest_x = d["dist"], l2, ls["n_over"], C2.cast_i16(x, bits), x.copy()
            found = found or d["found"]
            prev = d["prev"]
            if d["abort"]:
                break
            p1 *= q.beta1
            p2 *= q.beta2
            mod, m1, m2, x = adam_step(g, ls["gd"], x, a0, w0, mod, m1, m2, c, d["gate"], lw, p1, p2, q.lr, q.beta1, q.beta2, q.adam_eps)
        per.append(n_rows)
        lo, hi, c = C2.next_const(found, lo, hi, c)
    return dict(adv=gbest_row, success=1 if gbest < float("inf") else -1, adver_f64=gbest_x, trace=np.array(rows),
                rows_per_step=np.array(per, np.int32), best_dist=gbest, best_l2=gbest_l2, n_over=gbest_no, const=c,
                min_margin=margin, min_theta_margin=tmargin)
