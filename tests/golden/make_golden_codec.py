"""Writes tests/golden/codec_audioop.npz from Python's stdlib audioop (present up to Python 3.12): the G.711 mu-law and A-law
round trips of all 65 536 int16 values and the IMA ADPCM round trip of three even-length rows -- code this project did not
write, against which tests/codec_ref.py (and through it the device) is pinned bit for bit.

    python -m tests.golden.make_golden_codec
"""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "codec_audioop.npz")


def rows():
    """speech-like (4 000 samples: a pitch pulse train through two resonances under a syllable envelope, plus a little noise),
    full-range noise (4 000), and the 392-sample clamp row"""
    g = np.random.default_rng(20261019)
    n = 4000
    t = np.arange(n) / 16000.0
    f0 = 120.0 + 25.0 * np.sin(2.0 * np.pi * 2.3 * t)
    phase = 2.0 * np.pi * np.cumsum(f0) / 16000.0
    voiced = sum(np.sin(k * phase) / k for k in range(1, 12))
    formants = np.sin(2.0 * np.pi * 700.0 * t) * 0.6 + np.sin(2.0 * np.pi * 1800.0 * t) * 0.3
    env = 0.15 + 0.85 * np.abs(np.sin(2.0 * np.pi * 3.1 * t)) ** 2
    x = env * (voiced * (1.0 + 0.5 * formants)) * 5000.0 + g.normal(0.0, 60.0, n)
    speech = np.clip(np.rint(x), -32768, 32767).astype(np.int16)
    noise = g.integers(-32768, 32768, n).astype(np.int16)
    period = np.concatenate([np.full(8, 32767, np.int16), np.full(8, -32768, np.int16)])
    clamp = np.concatenate([np.tile(period, 12), np.zeros(200, np.int16)])
    return speech, noise, clamp


def main():
    import audioop
    allv = np.arange(-32768, 32768, dtype=np.int32).astype(np.int16)
    raw = allv.tobytes()
    out = {
        "all_values": allv,
        "ulaw": np.frombuffer(audioop.ulaw2lin(audioop.lin2ulaw(raw, 2), 2), np.int16),
        "alaw": np.frombuffer(audioop.alaw2lin(audioop.lin2alaw(raw, 2), 2), np.int16),
    }
    for name, x in zip(("speech", "noise", "clamp"), rows()):
        assert x.size % 2 == 0            # (a byte of ADPCM holds two samples)
        code, _state = audioop.lin2adpcm(x.tobytes(), 2, None)
        y, _state = audioop.adpcm2lin(code, 2, None)
        out["adpcm_in_" + name] = x
        out["adpcm_out_" + name] = np.frombuffer(y, np.int16)
        assert out["adpcm_out_" + name].size == x.size
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
