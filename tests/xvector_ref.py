"""The x-vector contract of include/fakebob_hip.h restated on the CPU: from feature rows to the embedding in PyTorch -- once
in float64 throughout, once with the frame layers in float32 (what a float32 implementation of the same function gives) --
and the back end (mean subtraction, LDA, length normalisation, PLDA) in float64 numpy.  No GPU, no engine import: `system`
is anything with models.XvectorSystem's attributes."""
import numpy as np
import torch


def splice_index(T, ctx):
    """(T, n_ctx) source rows: clamp(t + ctx[j], 0, T - 1)"""
    t = np.arange(T)[:, None] + np.asarray(ctx, np.int64)[None, :]
    return np.clip(t, 0, T - 1)


def frame_layer(h, ly, dtype):
    """h (T, din) tensor of dtype -> (T, dout): bn_scale * max(W . splice(h) + bias, 0) + bn_offset, every step in dtype"""
    T = h.shape[0]
    idx = torch.from_numpy(splice_index(T, ly["ctx"]))
    sp = h[idx].reshape(T, -1)                                  # offsets-major along the columns
    W = torch.from_numpy(ly["W"]).to(dtype)
    a = sp @ W.T + torch.from_numpy(ly["bias"]).to(dtype)
    a = torch.clamp(a, min=0)
    return torch.from_numpy(ly["bn_scale"]).to(dtype) * a + torch.from_numpy(ly["bn_offset"]).to(dtype)


def pool(h):
    """(T, P) float64 tensor -> (2 P,): mean, sqrt(max(E[h^2] - mean^2, 1e-10))"""
    mean = h.mean(dim=0)
    var = (h * h).mean(dim=0) - mean * mean
    return torch.cat([mean, torch.sqrt(torch.clamp(var, min=1e-10))])


def stages(system, x, frame_dtype=torch.float64):
    """One utterance x (T, D) -> ([every frame layer's output (T, dout)], statistics (2 P,), embedding (R,)) as float64
    numpy arrays; the frame layers run in frame_dtype, pooling and the segment affine in float64."""
    with torch.no_grad():
        h = torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(frame_dtype)
        outs = []
        for ly in system.layers:
            h = frame_layer(h, ly, frame_dtype)
            outs.append(h.to(torch.float64).numpy().copy())
        st = pool(h.to(torch.float64))
        emb = torch.from_numpy(system.seg_W).to(torch.float64) @ st + torch.from_numpy(system.seg_bias).to(torch.float64)
    return outs, st.numpy().copy(), emb.numpy().copy()


def backend_transform(system, v):
    """a float32-rounded embedding / i-vector (R,) -> its PLDA-space vector (L,)"""
    R, L = system.R, system.L
    x = np.asarray(v, np.float32).astype(np.float64) - system.mean_vec.astype(np.float64)
    lda = system.lda.astype(np.float64)
    z = lda[:, :R] @ x + (lda[:, R] if lda.shape[1] == R + 1 else 0.0)
    ratio = np.sqrt(z @ z) / np.sqrt(L)
    if ratio != 0.0:
        z = z / ratio
    y = system.plda_transform @ (z - system.plda_mean)
    return y * np.sqrt(L / np.sum(y * y / (system.plda_psi + 1.0)))


def plda_llr(system, emb):
    """embeddings (B, R) float64 -> PLDA log-likelihood ratios (B, S) against system.enrolled (Plda::LogLikelihoodRatio,
    one enrolment utterance), before z-norm"""
    psi = system.plda_psi
    tr = np.stack([backend_transform(system, e) for e in system.enrolled])
    out = np.empty((len(emb), len(tr)))
    for b, e in enumerate(emb):
        y = backend_transform(system, e)
        for s, t in enumerate(tr):
            mean = psi / (psi + 1.0) * t
            var = 1.0 + psi / (psi + 1.0)
            d = y - mean
            given = -0.5 * (np.sum(np.log(var)) + np.sum(d * d / var))
            var0 = 1.0 + psi
            without = -0.5 * (np.sum(np.log(var0)) + np.sum(y * y / var0))
            out[b, s] = given - without      # (the L log(2 pi) terms cancel)
    return out
