"""numpy restatement of the randomised stage of the input-transform chain (include/fakebob_hip.h: FB_TF_NOISE in the
"Stage contract", and the EOT mean of fb_set_eot), written from the header and from nothing else.  It extends
tests/input_transform_ref.py, which restates the four deterministic kinds.

The normals are an ARGUMENT: the generator has its own contract ("Noise RNG contract") and its own tests; what is
restated here is what the stage does with them.

    y[i] = clip(rint(x[i] + s * z[i]))      float64: the product is rounded, then the sum; rint ties to even
    k = 0: s = taps[0]                      k = 1: s = sqrt(E / n / rho), rho = taps[0], E = the exact integer sum of
                                            squares of the utterance as it is handed to the CHAIN"""
import numpy as np

from tests.input_transform_ref import ref_stage

NOISE = 4
ABSOLUTE, SNR = 0, 1


def power(x):
    """E: the exact sum of squares of an int16 utterance, a Python integer"""
    xi = np.asarray(x).astype(np.int64)
    return int(np.sum(xi * xi))          # < 2^15 * 2^15 * 2^31 = 2^61: exact in int64


def noise_scale(mode, t0, E, n):
    if mode == ABSOLUTE:
        assert 0.0 <= t0 <= 32768.0
        return np.float64(t0)
    assert mode == SNR and t0 > 0.0 and np.isfinite(t0)
    return np.sqrt(np.float64(E) / np.float64(n) / np.float64(t0))    # int -> float64, /, /, sqrt: each correctly rounded


def ref_noise_stage(x, mode, t0, z, E):
    """x: the stage's int16 input; z: float32 normals, one per sample; E: the power of the CHAIN's input"""
    x = np.asarray(x)
    z = np.asarray(z)
    assert x.dtype == np.int16 and x.ndim == 1 and z.dtype == np.float32 and z.shape == x.shape
    s = noise_scale(mode, float(t0), E, x.size)
    v = x.astype(np.float64) + s * z.astype(np.float64)               # numpy fuses nothing: two roundings
    return np.clip(np.rint(v), -32768, 32767).astype(np.int16)


def ref_noisy(x, chain, normals):
    """The chain applied to one utterance.  normals: {stage index: float32 array} for its noise stages."""
    y = np.asarray(x)
    E = power(y)
    for s, (kind, k, taps) in enumerate(chain):
        if kind == NOISE:
            y = ref_noise_stage(y, int(k), float(np.ravel(taps)[0]), normals[s], E)
        else:
            y = ref_stage(y, kind, k, taps)
    return y


def eot_mean(v):
    """The EOT mean of the contract over the LAST axis: acc = v[0]; acc += v[j], j ascending; acc / r -- float64, one
    rounding per addition and one for the division"""
    v = np.asarray(v, np.float64)
    acc = v[..., 0].copy()
    for j in range(1, v.shape[-1]):
        acc = acc + v[..., j]
    return acc / np.float64(v.shape[-1])
