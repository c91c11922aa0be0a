"""The telephone-line codec in front of the victim (fb_set_codec; the contract is in include/fakebob_hip.h): the names the
Python side takes, and the three round trips on the host, so that audio can be coded without the engine -- bit for bit what
k_codec writes, and what Python's audioop gives (ulaw2lin(lin2ulaw), alaw2lin(lin2alaw), adpcm2lin(lin2adpcm) at width 2).

    "ulaw"     G.711 mu-law      memoryless companding, 8 bit per sample
    "alaw"     G.711 A-law       the same, the European law
    "adpcm"    IMA/DVI ADPCM     4 bit per sample; predictor and step index run along the whole utterance from (0, 0)
    None, "none"                 no codec

The codec runs at the utterance's own sampling rate; a narrow-band line is a low-pass or band-pass stage of the
input-transform chain in front of it."""
import numpy as np

FB_CODEC_NONE, FB_CODEC_ULAW, FB_CODEC_ALAW, FB_CODEC_ADPCM = 0, 1, 2, 3
KINDS = {"none": FB_CODEC_NONE, "ulaw": FB_CODEC_ULAW, "alaw": FB_CODEC_ALAW, "adpcm": FB_CODEC_ADPCM}
NAMES = ("ulaw", "alaw", "adpcm")  # what a command line offers besides "none"

IDX = (-1, -1, -1, -1, 2, 4, 6, 8)
STEP = (7, 8, 9, 10, 11, 12, 13, 14, 16, 17, 19, 21, 23, 25, 28, 31, 34, 37, 41, 45, 50, 55, 60, 66, 73, 80, 88, 97, 107, 118,
        130, 143, 157, 173, 190, 209, 230, 253, 279, 307, 337, 371, 408, 449, 494, 544, 598, 658, 724, 796, 876, 963, 1060,
        1166, 1282, 1411, 1552, 1707, 1878, 2066, 2272, 2499, 2749, 3024, 3327, 3660, 4026, 4428, 4871, 5358, 5894, 6484,
        7132, 7845, 8630, 9493, 10442, 11487, 12635, 13899, 15289, 16818, 18500, 20350, 22385, 24623, 27086, 29794, 32767)


def kind_of(codec):
    """A codec as the Python side names it -- "ulaw", "alaw", "adpcm", None / "none" / "", or the library's integer -- as
    the library's FB_CODEC_* value.  ValueError for anything else."""
    if codec is None:
        return FB_CODEC_NONE
    if isinstance(codec, str):
        key = codec.strip().lower() or "none"
        if key not in KINDS:
            raise ValueError("codec %r: one of %s, or none" % (codec, ", ".join(NAMES)))
        return KINDS[key]
    if isinstance(codec, (int, np.integer)) and not isinstance(codec, bool) and int(codec) in KINDS.values():
        return int(codec)
    raise ValueError("codec %r: one of %s, or none" % (codec, ", ".join(NAMES)))


def name_of(kind):
    """The name of an FB_CODEC_* value (None for FB_CODEC_NONE)."""
    kind = kind_of(kind)
    return None if kind == FB_CODEC_NONE else NAMES[kind - 1]


def _segments(m, first):
    """how many of first, 2 * first + 1, 4 * first + 3, ... (eight thresholds) m exceeds"""
    seg = np.zeros_like(m)
    for k in range(8):
        seg += m > ((first + 1) << k) - 1
    return seg


def _ulaw_table():
    x = np.arange(-32768, 32768, dtype=np.int32)
    v = x >> 2
    neg = v < 0
    m = np.minimum(np.where(neg, -v, v), 8159) + 33
    seg = _segments(m, 0x3F)
    top = seg == 8
    seg = np.where(top, 7, seg)
    q = np.where(top, 15, (m >> (seg + 1)) & 15)
    t = (((q << 3) + 0x84) << seg) - 0x84
    return np.where(neg, -t, t).astype(np.int16)


def _alaw_table():
    x = np.arange(-32768, 32768, dtype=np.int32)
    v = x >> 3
    neg = v < 0
    m = np.where(neg, -v - 1, v)
    seg = _segments(m, 0x1F)
    q = np.where(seg < 2, (m >> 1) & 15, (m >> seg) & 15)
    t = q << 4
    u = np.where(seg == 0, t + 8, np.where(seg == 1, t + 0x108, (t + 0x108) << np.maximum(seg - 1, 0)))
    return np.where(neg, -u, u).astype(np.int16)


_tables = {}


def _table(kind):
    if kind not in _tables:
        _tables[kind] = _ulaw_table() if kind == FB_CODEC_ULAW else _alaw_table()
    return _tables[kind]


def ulaw(x):
    """The G.711 mu-law round trip of int16 samples (any shape)."""
    return _table(FB_CODEC_ULAW)[np.asarray(x, np.int16).astype(np.int32) + 32768]


def alaw(x):
    """The G.711 A-law round trip of int16 samples (any shape)."""
    return _table(FB_CODEC_ALAW)[np.asarray(x, np.int16).astype(np.int32) + 32768]


def adpcm(x):
    """The IMA ADPCM round trip of ONE utterance of int16 samples (1-D): the state starts at (0, 0) and runs along it."""
    x = np.ascontiguousarray(x, np.int16).reshape(-1)
    y = np.empty_like(x)
    vp, ix = 0, 0
    for i, xi in enumerate(x.tolist()):
        step = STEP[ix]
        d = xi - vp
        ad = -d if d < 0 else d
        # the quantiser's three decisions as comparisons of |d| with running thresholds
        base, delta = 0, 0
        for bit, part in ((4, step), (2, step >> 1), (1, step >> 2)):
            if ad >= base + part:
                delta |= bit
                base += part
        vd = base + (step >> 3)
        vp = max(-32768, min(32767, vp - vd if d < 0 else vp + vd))
        ix = max(0, min(88, ix + IDX[delta]))
        y[i] = vp
    return y


def roundtrip(codec, x):
    """x through the named codec (kind_of's names): int16 of x's shape.  G.711 takes any shape; ADPCM treats the last axis
    as time and every row on its own.  No codec: a copy."""
    kind = kind_of(codec)
    x = np.asarray(x, np.int16)
    if kind == FB_CODEC_NONE:
        return x.copy()
    if kind == FB_CODEC_ULAW:
        return ulaw(x)
    if kind == FB_CODEC_ALAW:
        return alaw(x)
    if x.ndim <= 1:
        return adpcm(x).reshape(x.shape)
    rows = x.reshape(-1, x.shape[-1])
    return np.stack([adpcm(r) for r in rows]).reshape(x.shape)
