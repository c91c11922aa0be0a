"""The white-box reference: the function fb_get_grad_wb differentiates, restated in PyTorch float64 on the CPU.

TEST INFRASTRUCTURE ONLY.  Written from SURVEY.md Appendix A and the "white-box gradients" contract of
include/fakebob_hip.h, independently of the engine's kernels and of oracle/: the forward is the front end (int16 cast,
MFCC, VAD, add-deltas, sliding CMVN, voiced rows), the per-model mean frame log-likelihood, the system scores and the
reference's loss_fn; the gradient comes from autograd, never from a hand-derived backward.

 - the cast is a straight-through identity (the forward uses the truncated int16 value);
 - the float32 storage points of the engine / Kaldi are NOT rounded here (they are identities for the gradient, and the
   forward then agrees with the CPU oracle to a few 1e-6: tests/test_whitebox_ref_host.py);
 - the voiced mask is computed from the forward's values (float32 C0 against a float32 threshold, as compute-vad-decision
   does) and held constant;
 - an active floor (a mel bin or a frame energy below FLT_EPSILON, energy_floor) contributes zero: torch.clamp;
 - a maximum takes the subgradient of the FIRST maximal index, as make_decisions does.
`cfg` is any object with fb_frontend_cfg's fields (fakebob_amd._native.FrontendCfg, oracle.FrontendCfg).
"""
import math

import numpy as np
import torch

FLT_EPSILON = float(np.finfo(np.float32).eps)
F64 = torch.float64


def test_audio(n):
    """The utterance the white-box tests use at length n: models.synthetic_audio(0, n); from 40 000 samples on its
    low-energy stretches are four times quieter.  (As it stands the VAD threshold of a three-second utterance falls
    INSIDE the spread of the quiet frames' C0 -- min |c0 - thr| 6e-4 at N = 48 000 --, and a mask that a rounding can flip
    is no fixture; quieter, the margin is 2.2.)  int16-exact float64 in [-1, 1)."""
    from fakebob_amd.models import synthetic_audio
    x = synthetic_audio(0, n)
    if n >= 40000:
        quiet = (np.arange(n) // 8000) % 3 == 2
        x[quiet] = np.round(x[quiet] * 0.25 * 32768.0) / 32768.0
    return x


test_audio.__test__ = False   # (a helper, not a test case)


# ------------------------------------------------------------------------------------------------ tables (A.2, A.5)
def num_frames(cfg, n):
    if cfg.snip_edges:
        return 0 if n < cfg.frame_length else 1 + (n - cfg.frame_length) // cfg.frame_shift
    return (n + cfg.frame_shift // 2) // cfg.frame_shift


def frame_index(cfg, n):
    """idx[T][L]: the sample every frame position reads -- the oracle's rule, `while (k < 0 || k >= n)` reflect."""
    T, L = num_frames(cfg, n), cfg.frame_length
    idx = np.empty((T, L), np.int64)
    for f in range(T):
        start = f * cfg.frame_shift if cfg.snip_edges else f * cfg.frame_shift + cfg.frame_shift // 2 - L // 2
        for s in range(L):
            k = start + s
            while k < 0 or k >= n:
                k = -k - 1 if k < 0 else 2 * n - 1 - k
            idx[f, s] = k
    return idx


def _mel(f):
    return 1127.0 * math.log(1.0 + f / 700.0)


class Tables(object):
    def __init__(self, cfg):
        L, P, nb, nc = cfg.frame_length, cfg.padded_length, cfg.num_mel_bins, cfg.num_ceps
        a = 2.0 * math.pi / (L - 1)
        self.window = torch.tensor(np.array([(0.5 - 0.5 * math.cos(a * i)) ** 0.85 for i in range(L)], np.float32).astype(np.float64))
        nfft = P // 2
        nyq = 0.5 * cfg.sample_freq
        hi = cfg.high_freq if cfg.high_freq > 0.0 else nyq + cfg.high_freq
        bw = cfg.sample_freq / P
        mlo, mhi = _mel(cfg.low_freq), _mel(hi)
        md = (mhi - mlo) / (nb + 1)
        w = np.zeros((nb, nfft), np.float32)
        for b in range(nb):
            left, center, right = mlo + b * md, mlo + (b + 1) * md, mlo + (b + 2) * md
            for i in range(nfft):
                mel = _mel(bw * i)
                if left < mel < right:
                    w[b, i] = (mel - left) / (center - left) if mel <= center else (right - mel) / (right - center)
        self.mel_w = torch.tensor(w.astype(np.float64))
        dct = np.empty((nc, nb), np.float32)
        for k in range(nc):
            for n in range(nb):
                dct[k, n] = math.sqrt(1.0 / nb) if k == 0 else math.sqrt(2.0 / nb) * math.cos(math.pi / nb * (n + 0.5) * k)
        self.dct = torch.tensor(dct.astype(np.float64))
        lif = np.ones(nc, np.float32)
        if cfg.cepstral_lifter != 0.0:
            for i in range(nc):
                lif[i] = 1.0 + 0.5 * cfg.cepstral_lifter * math.sin(math.pi * i / cfg.cepstral_lifter)
        self.lifter = torch.tensor(lif.astype(np.float64))
        # delta kernels: order i has 2 i W + 1 taps, each stored as float32 (A.5)
        W, order = cfg.delta_window, cfg.delta_order
        self.scales = [np.array([1.0])]
        for i in range(1, order + 1):
            prev, po, co = self.scales[i - 1], (i - 1) * W, i * W
            cur = np.zeros(2 * co + 1)
            norm = 0.0
            for j in range(-W, W + 1):
                norm += float(j) * j
                for k in range(-po, po + 1):
                    cur[j + k + co] += float(j) * prev[k + po]
            self.scales.append((cur / norm).astype(np.float32).astype(np.float64))


# ------------------------------------------------------------------------------------------------ the front end
def cast_st(audio, bits):
    """int16 cast with 2^(bits - 1), straight-through: the value is the truncated one, the derivative the scale."""
    scale = float(2 ** (bits - 1))
    v = audio * scale
    q = torch.trunc(v.detach())
    q = ((q + 32768.0) % 65536.0) - 32768.0      # the low 16 bits (1.0 -> -32768)
    return v + (q - v.detach())


def mfcc(cfg, x, tab=None):
    """x: float64 [n] in int16 units -> MFCC [T][num_ceps] float64."""
    tab = tab or Tables(cfg)
    n, L, P = x.shape[0], cfg.frame_length, cfg.padded_length
    fr = x[torch.tensor(frame_index(cfg, n))]                   # [T][L]
    if cfg.remove_dc:
        fr = fr - fr.sum(dim=1, keepdim=True) / L
    energy = (fr * fr).sum(dim=1) if cfg.raw_energy else None
    if cfg.preemph != 0.0:
        prev = torch.cat([fr[:, :1], fr[:, :-1]], dim=1)
        fr = fr - cfg.preemph * prev
    fr = fr * tab.window
    if not cfg.raw_energy:
        energy = (fr * fr).sum(dim=1)
    log_energy = torch.log(torch.clamp(energy, min=FLT_EPSILON))
    spec = torch.fft.rfft(torch.nn.functional.pad(fr, (0, P - L)), dim=1)
    pw = (spec.real ** 2 + spec.imag ** 2)[:, :P // 2]
    mel = torch.clamp(pw @ tab.mel_w.T, min=FLT_EPSILON)
    cep = (torch.log(mel) @ tab.dct.T) * tab.lifter
    if cfg.use_energy:
        if cfg.energy_floor > 0.0:
            log_energy = torch.clamp(log_energy, min=math.log(cfg.energy_floor))
        cep = torch.cat([log_energy[:, None], cep[:, 1:]], dim=1)
    return cep


def vad_mask(cfg, mf):
    """compute-vad-decision on the forward's C0 (A.4): float32 values against a float32 threshold.  Also returns
    min |c0 - thr|, what the tests bound from below."""
    c0 = mf.detach().numpy()[:, 0].astype(np.float32)
    T = c0.shape[0]
    thr = np.float32(cfg.vad_energy_threshold + cfg.vad_energy_mean_scale * float(c0.astype(np.float64).sum()) / T)
    above = c0 > thr
    ctx = cfg.vad_frames_context
    out = np.zeros(T, bool)
    for t in range(T):
        lo, hi = max(0, t - ctx), min(T - 1, t + ctx)
        num, den = int(above[lo:hi + 1].sum()), hi - lo + 1
        out[t] = np.float32(num) >= np.float32(den) * np.float32(cfg.vad_proportion_threshold)
    return out, float(np.abs(c0.astype(np.float64) - float(thr)).min())


def add_deltas(cfg, mf, tab):
    T = mf.shape[0]
    t = torch.arange(T)
    cols = []
    for i in range(cfg.delta_order + 1):
        sc, off = tab.scales[i], i * cfg.delta_window
        acc = torch.zeros_like(mf)
        for j in range(-off, off + 1):
            if sc[j + off] != 0.0:
                acc = acc + float(sc[j + off]) * mf[torch.clamp(t + j, 0, T - 1)]
        cols.append(acc)
    return torch.cat(cols, dim=1)


def cmvn_sliding(cfg, df):
    """apply-cmvn-sliding --center=true --norm-vars=false (A.6), any T against cmn_window."""
    T, Wn = df.shape[0], cfg.cmn_window
    pre = torch.cat([torch.zeros(1, df.shape[1], dtype=F64), torch.cumsum(df, dim=0)], dim=0)
    wb_, we_, al_ = [], [], []
    for t in range(T):
        wb = t - Wn // 2
        we = wb + Wn
        if wb < 0:
            we -= wb
            wb = 0
        if we > T:
            wb -= we - T
            we = T
            wb = max(wb, 0)
        wb_.append(wb)
        we_.append(we)
        al_.append(float(np.float32(-1.0 / (we - wb))))
    alpha = torch.tensor(al_, dtype=F64)[:, None]
    return df + alpha * (pre[torch.tensor(we_)] - pre[torch.tensor(wb_)])


def features(cfg, x, tab=None):
    """x float64 [n] (int16 units) -> (compacted voiced rows [Tv][D], mask [T] bool, min |c0 - thr|)."""
    tab = tab or Tables(cfg)
    mf = mfcc(cfg, x, tab)
    mask, margin = vad_mask(cfg, mf)
    f = cmvn_sliding(cfg, add_deltas(cfg, mf, tab))
    return f[torch.tensor(mask)], mask, margin


# ------------------------------------------------------------------------------------------------ the back end
def gmm_raw(feats, gc, miv, iv):
    """mean frame log-likelihood per model: feats [Tv][D]; gc [M][C], miv / iv [M][C][D] (any float) -> raw [M]."""
    gc, miv, iv = (torch.as_tensor(np.asarray(a, np.float64)) for a in (gc, miv, iv))
    ll = gc[:, None, :] + torch.einsum("td,mcd->mtc", feats, miv) - 0.5 * torch.einsum("td,mcd->mtc", feats * feats, iv)
    return torch.logsumexp(ll, dim=2).mean(dim=1)


def system_scores(task, raw, z_mean=None, z_std=None):
    if task == "CSI":
        zm = torch.zeros_like(raw) if z_mean is None else torch.as_tensor(np.asarray(z_mean, np.float64))
        zs = torch.ones_like(raw) if z_std is None else torch.as_tensor(np.asarray(z_std, np.float64))
        return (raw - zm) / zs
    return raw[1:] - raw[0]


def _first_max(s, skip=None):
    """the first maximal index of s (skipping one index), as a Python int: make_decisions' argmax"""
    v = s.detach().numpy().copy()
    if skip is not None:
        v[skip] = -np.inf
    return int(np.argmax(v))


def loss_fn(task, attack_type, s, threshold=0.0, adver_thresh=0.0, target=0, true=0):
    """FakeBob.loss_fn (FAKEBOB.py:248-299) of one row of scores, maxima by first-maximum index."""
    if task == "SV":
        return (threshold + adver_thresh) - s[0]
    if task == "OSI" and attack_type == "untargeted":
        return (threshold + adver_thresh) - s[_first_max(s)]
    if task == "OSI":
        if s.shape[0] > 1:
            om = s[_first_max(s, target)]
            mx = om if float(om.detach()) > threshold else torch.tensor(threshold, dtype=F64)   # np.maximum: the threshold wins a tie
        else:
            mx = torch.tensor(threshold, dtype=F64)
        return (mx + adver_thresh) - s[target]
    if attack_type == "targeted":
        return (s[_first_max(s, target)] + adver_thresh) - s[target]
    return (s[true] + adver_thresh) - s[_first_max(s, true)]


class Result(object):
    pass


def loss_and_grad(cfg, models, task, attack_type, audio, bits=16, threshold=0.0, adver_thresh=0.0, target=0, true=0,
                  z_mean=None, z_std=None, want_grad=True, cast=True):
    """models = (gc [M][C], miv [M][C][D], iv [M][C][D]).  -> Result with loss, grad (d loss / d audio, numpy [N]; None
    without want_grad), scores, raw, mask, margin, tv.  cast=False: the real-valued function itself, audio * 2^(bits - 1)
    without the truncation (what a finite difference can be taken of)."""
    a = torch.tensor(np.asarray(audio, np.float64).reshape(-1), requires_grad=want_grad)
    x = cast_st(a, bits) if cast else a * float(2 ** (bits - 1))
    feats, mask, margin = features(cfg, x)
    raw = gmm_raw(feats, *models)
    s = system_scores(task, raw, z_mean, z_std)
    l = loss_fn(task, attack_type, s, threshold, adver_thresh, target, true)
    r = Result()
    r.grad = None
    if want_grad:
        l.backward()
        r.grad = a.grad.numpy().copy()
    r.loss, r.scores, r.raw = float(l.detach()), s.detach().numpy().copy(), raw.detach().numpy().copy()
    r.mask, r.margin, r.tv = mask, margin, int(mask.sum())
    return r


# ------------------------------------------------------------------------------------------------ the two hooks' references
def frontend_vjp(cfg, wav, cot):
    """d <cot, feats(wav)> / d wav in int16 units for a cotangent cot [Tv][D] on the compacted rows -> (dwav [n], mask)."""
    x = torch.tensor(np.asarray(wav, np.float64).reshape(-1), requires_grad=True)
    feats, mask, _ = features(cfg, x)
    (feats * torch.as_tensor(np.asarray(cot, np.float64))).sum().backward()
    return x.grad.numpy().copy(), mask


def gmm_feat_grad(feats, w, gc, miv, iv):
    """The closed form of the GMM backward in numpy float64:
    g_t = (1 / Tv) sum_m w_m sum_c gamma_mtc (miv_mc - iv_mc * x_t), gamma the posteriors of model m."""
    x = np.asarray(feats, np.float64)
    gc, miv, iv = (np.asarray(a, np.float64) for a in (gc, miv, iv))
    out = np.zeros_like(x)
    for m in range(miv.shape[0]):
        if w[m] == 0.0:
            continue
        ll = gc[m][None, :] + x @ miv[m].T - 0.5 * (x * x) @ iv[m].T
        g = np.exp(ll - ll.max(axis=1, keepdims=True))
        g /= g.sum(axis=1, keepdims=True)
        out += w[m] * (g @ miv[m] - (g @ iv[m]) * x)
    return out / x.shape[0]
