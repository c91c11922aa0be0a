"""numpy restatement of the over-the-air channel's contract (include/fakebob_hip.h: fb_set_air_channel -- "Arithmetic"),
written from the header and from nothing else.  The float32 normals z and the decay's 32-bit word w are ARGUMENTS, as the
normals are in tests/input_transform_noise_ref.py: the generator has its own contract (the counter and key are stated in the
header; air_counter / air_key below restate them for the tests that check the words themselves).

    U = ((double)w + 0.5) * 2^-32;  rho = clip(rho_lo + U * (rho_hi - rho_lo), rho_lo, rho_hi)
    Q[0] = 1, Q[i] = Q[i-1] * rho (i < 64);  S = Q[63] * rho;  P[0] = 1, P[j] = P[j-1] * S (j < 64);  e[m] = P[m >> 6] * Q[m & 63]
    t[0] = 16384;  t[k] = 0 (0 < k < d);  t[k] = clip(rint((amp * z[k]) * e[k - d]), -32767, 32767)
    y[i] = sum_{k <= min(i, L-1)} t[k] x[i-k]  (exact);  o[i] = clip16((y[i] + 8192) >> 14)

numpy's float64 scalars and arrays round every operation once and never fuse: each line below is one rounding, as written."""
import numpy as np

AIRC = 0x41495243
DECAY_C0 = 0xFFFFFFFF


def air_key(seed, stream):
    """The Philox key of the channel's stream: (seed_lo ^ "AIRC", seed_hi ^ stream)"""
    return ((seed & 0xFFFFFFFF) ^ AIRC, ((seed >> 32) & 0xFFFFFFFF) ^ (stream & 0xFFFFFFFF))


def air_counter(c0, replica, utt, epoch):
    """The counter of tap quad c0 (taps 4 c0 .. 4 c0 + 3), or with c0 = DECAY_C0 of the decay's word (output word 0)"""
    return (c0 & 0xFFFFFFFF, replica, utt, epoch)


def decay(w, rho_lo, rho_hi):
    U = (np.float64(int(w)) + np.float64(0.5)) * np.float64(2.0 ** -32)
    span = np.float64(rho_hi) - np.float64(rho_lo)
    prod = U * span
    rho = np.float64(rho_lo) + prod
    return np.float64(min(max(rho, np.float64(rho_lo)), np.float64(rho_hi)))


def envelope(rho, n):
    """e[0 .. n) of the blocked recurrence (n <= 4096)"""
    rho = np.float64(rho)
    Q = np.empty(64, np.float64)
    Q[0] = 1.0
    for i in range(1, 64):
        Q[i] = Q[i - 1] * rho
    S = Q[63] * rho
    P = np.empty(64, np.float64)
    P[0] = 1.0
    for j in range(1, 64):
        P[j] = P[j - 1] * S
    m = np.arange(int(n))
    return P[m >> 6] * Q[m & 63]


def taps(L, d, amp, rho_lo, rho_hi, z, w):
    """The int16 response of one row: z (>= L,) float32 normals, w its decay word"""
    z = np.asarray(z)
    assert z.dtype == np.float32 and z.size >= L and 1 <= d <= L - 1
    t = np.zeros(L, np.int64)
    t[0] = 16384
    e = envelope(decay(w, rho_lo, rho_hi), L - d)
    az = np.float64(amp) * z[d:L].astype(np.float64)          # (amp * (double)z[k]): one rounding
    v = az * e                                                # ... * e[k - d]: one more
    t[d:] = np.minimum(np.maximum(np.rint(v), -32767.0), 32767.0).astype(np.int64)
    return t.astype(np.int16)


def conv_sums(x, t):
    """y[i] = sum_k t[k] x[i - k] in exact integers (int64), written as the sum it is: one shifted product per tap"""
    x = np.asarray(x).astype(np.int64)
    t = np.asarray(t).astype(np.int64)
    y = np.zeros(x.size, np.int64)
    for k in np.flatnonzero(t):
        if k < x.size:
            y[k:] += t[k] * x[:x.size - k]
    return y


def convolve(x, t):
    """o = clip16((y + 8192) >> 14): int16, the input's length"""
    assert np.asarray(x).dtype == np.int16 and np.asarray(t).dtype == np.int16
    y = conv_sums(x, t)
    return np.clip((y + 8192) >> 14, -32768, 32767).astype(np.int16)     # (>> on int64: arithmetic, floor)


def channel(x, L, d, amp, rho_lo, rho_hi, z, w):
    """One row through the channel"""
    return convolve(x, taps(L, d, amp, rho_lo, rho_hi, z, w))
