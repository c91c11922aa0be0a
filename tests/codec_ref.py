"""The telephone-line codecs restated in numpy from the stage contract of include/fakebob_hip.h (fb_set_codec), line by line:
G.711 mu-law and A-law over whole arrays, IMA ADPCM sample by sample.  It imports neither audioop nor fakebob_amd.codec: the
golden file (tests/golden/codec_audioop.npz, written from audioop) and the device are compared against THIS."""
import numpy as np

KINDS = ("ulaw", "alaw", "adpcm")
IDX = (-1, -1, -1, -1, 2, 4, 6, 8)
STEP = tuple(int(v) for v in """
7 8 9 10 11 12 13 14 16 17 19 21 23 25 28 31 34 37 41 45 50 55 60 66 73 80 88 97 107 118 130 143 157 173 190 209 230 253 279 307
337 371 408 449 494 544 598 658 724 796 876 963 1060 1166 1282 1411 1552 1707 1878 2066 2272 2499 2749 3024 3327 3660 4026 4428
4871 5358 5894 6484 7132 7845 8630 9493 10442 11487 12635 13899 15289 16818 18500 20350 22385 24623 27086 29794 32767""".split())
assert len(STEP) == 89

ULAW_SEG = (0x3F, 0x7F, 0xFF, 0x1FF, 0x3FF, 0x7FF, 0xFFF, 0x1FFF)
ALAW_SEG = (0x1F, 0x3F, 0x7F, 0xFF, 0x1FF, 0x3FF, 0x7FF, 0xFFF)


def _i32(x):
    x = np.asarray(x)
    assert x.dtype == np.int16, x.dtype
    return x.astype(np.int32)


def ulaw(x):
    x = _i32(x)
    v = x >> 2
    neg = v < 0
    m = np.minimum(np.where(neg, -v, v), 8159) + 33
    seg = sum((m > t).astype(np.int32) for t in ULAW_SEG)
    top = seg == 8
    assert np.all(m[top] == 8192)
    seg = np.where(top, 7, seg)
    q = np.where(top, 15, (m >> (seg + 1)) & 15)
    t = (((q << 3) + 0x84) << seg) - 0x84
    return np.where(neg, -t, t).astype(np.int16)


def alaw(x):
    x = _i32(x)
    v = x >> 3
    neg = v < 0
    m = np.where(neg, -v - 1, v)
    seg = sum((m > t).astype(np.int32) for t in ALAW_SEG)
    assert seg.size == 0 or seg.max() <= 7
    q = np.where(seg < 2, (m >> 1) & 15, (m >> seg) & 15)
    t = q << 4
    u = np.where(seg == 0, t + 8, np.where(seg == 1, t + 0x108, (t + 0x108) << np.maximum(seg - 1, 0)))
    return np.where(neg, -u, u).astype(np.int16)


def adpcm_trace(x):
    """One row through the ADPCM round trip: (y int16 (n,), ix int (n,), raw int (n,)) -- the output, the step index behind
    every sample and the predictor BEFORE its clip (so that a test can see both clips act)."""
    x = np.asarray(x)
    assert x.dtype == np.int16 and x.ndim == 1
    n = x.size
    y, ixs, raws = np.empty(n, np.int16), np.empty(n, np.int64), np.empty(n, np.int64)
    vp, ix = 0, 0
    for i in range(n):
        step = STEP[ix]
        d = int(x[i]) - vp
        s = d < 0
        d = abs(d)
        delta = 0
        vd = step >> 3
        if d >= step:
            delta = 4
            d -= step
            vd += step
        step >>= 1
        if d >= step:
            delta |= 2
            d -= step
            vd += step
        step >>= 1
        if d >= step:
            delta |= 1
            vd += step
        raw = vp - vd if s else vp + vd
        vp = min(max(raw, -32768), 32767)
        ix = min(max(ix + IDX[delta], 0), 88)
        y[i], ixs[i], raws[i] = vp, ix, raw
    return y, ixs, raws


def adpcm(x):
    return adpcm_trace(x)[0]


def codec(kind, x):
    """One row (1-D int16) through the named codec."""
    return {"ulaw": ulaw, "alaw": alaw, "adpcm": adpcm}[kind](x)


def clamp_row():
    """The 392-sample row that drives the ADPCM index to 0 and to 88 and the predictor into both clips: 12 periods of
    8 x 32767 followed by 8 x -32768, then 200 zeros."""
    period = np.concatenate([np.full(8, 32767, np.int16), np.full(8, -32768, np.int16)])
    return np.concatenate([np.tile(period, 12), np.zeros(200, np.int16)])
