"""numpy restatement of the input-transform stage contract (include/fakebob_hip.h, "Stage contract"), written from the
contract's table and from nothing else: what the device kernel and the Python builders are held to.

A chain is a list of (kind, k, taps) triples -- fakebob_amd.input_transform.Stage unpacks as one.  Every stage maps the
int16 samples x[0 .. n) of ONE utterance to y[0 .. n); indices outside [0, n) read as 0 at every stage."""
import numpy as np

QUANT, MEDIAN, FIR, DECIMATE = 0, 1, 2, 3


def _clip(v):
    return np.clip(v, -32768, 32767).astype(np.int16)


def ref_stage(x, kind, k, taps=None):
    x = np.asarray(x)
    assert x.dtype == np.int16 and x.ndim == 1
    n, k = x.size, int(k)
    xi = x.astype(np.int64)
    if kind == QUANT:
        assert 1 <= k <= 16384
        return _clip(k * np.floor_divide(xi + k // 2, k))       # floor_divide rounds toward -inf
    if kind == MEDIAN:
        assert 3 <= k <= 31 and k % 2 == 1
        r = (k - 1) // 2
        xp = np.concatenate([np.zeros(r, np.int64), xi, np.zeros(r, np.int64)])
        win = np.lib.stride_tricks.sliding_window_view(xp, k)   # win[i] = x[i - r .. i + r]
        return np.sort(win, axis=1)[:, r].astype(np.int16)
    if kind == FIR:
        h = np.asarray(taps, np.float64).reshape(-1)
        assert h.size == k and 1 <= k <= 511 and k % 2 == 1 and np.all(np.abs(h) <= 2.0 ** 20)
        c = (k - 1) // 2
        xp = np.concatenate([np.zeros(c), xi.astype(np.float64), np.zeros(c)])   # xp[m] = x[m - c]
        acc = np.zeros(n, np.float64)
        for j in range(k):                                       # ascending; product rounded, then the sum: numpy fuses nothing
            acc = acc + h[j] * xp[2 * c - j:2 * c - j + n]       # x[i + c - j]
        return _clip(np.rint(acc))                               # rint: ties to even
    if kind == DECIMATE:
        assert 2 <= k <= 64
        return np.where(np.arange(n) % k == 0, xi, 0).astype(np.int16)
    raise ValueError(kind)


def ref(x, chain):
    y = np.asarray(x)
    for kind, k, taps in chain:
        y = ref_stage(y, kind, k, taps)
    return y
