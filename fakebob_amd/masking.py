"""The psychoacoustic masking threshold of an utterance (Qin et al., "Imperceptible, robust and targeted adversarial examples
for ASR"; the MPEG-1 model 1 with tonal maskers only), float64 numpy.  It is host work, done once per attack: the engine takes
theta as data (include/fakebob_hip.h, "masking", states the framing and the loss; this module states the threshold).

Framing: window W in {512, 1024, 2048}, hop W/4, K = W/2 + 1 bins; N >= W samples make F = 1 frames if N == W, else
ceil((N - W) / hop) + 1, the signal extended with zeros to (F-1)*hop + W; periodic Hann h[n] = 0.5 - 0.5 cos(2 pi n / W);
  p(v)[f,k] = (8/3) |sum_n h[n] v[f*hop+n] exp(-2 pi i k n / W)|^2 / W^2.
Threshold: psd_max = max p(a0); PSD = 96 + 10 log10(p / psd_max + 1e-20) dB; fr = k fs / W;
  Bark z = 13 atan(0.00076 fr) + 3.5 atan((fr / 7500)^2);
  ATH = 3.64 (fr/1000)^-0.8 - 6.5 exp(-0.6 (fr/1000 - 3.3)^2) + 1e-3 (fr/1000)^4 - 12 dB where z > 1, -inf below.
Per frame: (1) candidates are the bins 1 .. K-2 with PSD strictly above both neighbours; (2) a candidate's level is
L = 10 log10 of the sum of the three linear powers at k-1, k, k+1; (3) a candidate with L < ATH[k] is dropped; (4) the rest
are swept in ascending bin order: one less than 0.5 Bark above the last kept masker replaces it if its L is strictly larger
and is dropped otherwise, one 0.5 Bark or more above is kept; (5) a kept masker j spreads to bin k as
T = L_j - 6.025 - 0.275 z_j + SF, SF = 27 dz for dz = z_k - z_j <= 0, else (-27 + 0.37 max(L_j - 40, 0)) dz.
theta[f,k] = sum_j 10^(T/10) + 10^(ATH[k]/10), linear power (10^-inf = 0).
"""
import numpy as np

WINDOWS = (512, 1024, 2048)


def n_frames(n, window):
    """F(N, W) of the framing above"""
    n, window = int(n), int(window)
    if window not in WINDOWS:
        raise ValueError("masking: window %d is not one of %s" % (window, WINDOWS))
    if n < window:
        raise ValueError("masking: %d samples are fewer than the window %d" % (n, window))
    hop = window // 4
    return 1 if n == window else -(-(n - window) // hop) + 1


def hann(window):
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(window) / window)


def frame_power(v, window):
    """p(v) [F, K]"""
    v = np.asarray(v, np.float64).reshape(-1)
    F = n_frames(v.size, window)
    hop = window // 4
    ext = np.zeros((F - 1) * hop + window, np.float64)
    ext[:v.size] = v
    idx = np.arange(F)[:, None] * hop + np.arange(window)[None, :]
    X = np.fft.rfft(ext[idx] * hann(window)[None, :], axis=1)
    return (8.0 / 3.0) * (X.real * X.real + X.imag * X.imag) / float(window * window)


def bark(fr):
    fr = np.asarray(fr, np.float64)
    return 13.0 * np.arctan(0.00076 * fr) + 3.5 * np.arctan((fr / 7500.0) ** 2)


def threshold_in_quiet(fs, window):
    """(ATH [K] in dB with -inf where z <= 1, z [K])"""
    fr = np.arange(window // 2 + 1, dtype=np.float64) * float(fs) / float(window)
    z = bark(fr)
    khz = fr / 1000.0
    ath = np.full(fr.size, -np.inf)
    m = z > 1.0
    ath[m] = 3.64 * khz[m] ** -0.8 - 6.5 * np.exp(-0.6 * (khz[m] - 3.3) ** 2) + 1e-3 * khz[m] ** 4 - 12.0
    return ath, z


def frame_maskers(psd, ath, z):
    """steps 1 to 4 on one frame's PSD [K] in dB -> (bins, levels) of the kept maskers, ascending"""
    K = psd.size
    k = np.arange(1, K - 1)
    cand = k[(psd[1:-1] > psd[:-2]) & (psd[1:-1] > psd[2:])]
    lin = 10.0 ** (psd / 10.0)
    L = 10.0 * np.log10(lin[cand - 1] + lin[cand] + lin[cand + 1])
    keep = ~(L < ath[cand])
    bins, levels = [], []
    for kk, ll in zip(cand[keep].tolist(), L[keep].tolist()):
        if bins and z[kk] - z[bins[-1]] < 0.5:
            if ll > levels[-1]:
                bins[-1], levels[-1] = kk, ll
        else:
            bins.append(kk)
            levels.append(ll)
    return np.array(bins, np.int64), np.array(levels, np.float64)


def spread(bins, levels, z):
    """step 5: sum_j 10^(T_j[k] / 10) over the maskers -> [K] linear power"""
    if bins.size == 0:
        return np.zeros(z.size, np.float64)
    zj = z[bins][:, None]
    Lj = levels[:, None]
    dz = z[None, :] - zj
    sf = np.where(dz <= 0.0, 27.0 * dz, (-27.0 + 0.37 * np.maximum(Lj - 40.0, 0.0)) * dz)
    T = Lj - 6.025 - 0.275 * zj + sf
    return np.sum(10.0 ** (T / 10.0), axis=0)


def masking_threshold(a0, fs, window):
    """a0: the float audio in [-1, 1] -> (theta [F, K] float64 linear power, psd_max).  ValueError on an all-zero utterance."""
    p = frame_power(a0, window)
    psd_max = float(p.max())
    if not psd_max > 0.0:
        raise ValueError("masking: the utterance is silent (psd_max = %r)" % psd_max)
    psd = 96.0 + 10.0 * np.log10(p / psd_max + 1e-20)
    ath, z = threshold_in_quiet(fs, window)
    quiet = 10.0 ** (ath / 10.0)
    theta = np.empty_like(p)
    for f in range(p.shape[0]):
        bins, levels = frame_maskers(psd[f], ath, z)
        theta[f] = spread(bins, levels, z) + quiet
    return theta, psd_max


def masking_loss(delta, theta, psd_max, window):
    """D(delta) and n_over on the host (numpy; no gradient) -> (D, n_over, P [F, K])"""
    P = frame_power(delta, window) * (10.0 ** 9.6 / float(psd_max))
    return float(np.maximum(P - theta, 0.0).sum() / P.size), int((P > theta).sum()), P
