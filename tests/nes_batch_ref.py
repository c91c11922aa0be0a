"""The NES batch restated in numpy (FAKEBOB.py:234-237 as the kernels write it), for tests/test_nes_batch_ref_host.py and
tests/test_gpu_nes_normals.py.  With z float32 (half, N) -- the tests pass oracle.noise(seed, it, stream, N, half) -- and a
the float64 iterate, the rows are

    row 0            a
    row 1 + j        sigma * z[j] + a
    row 1 + half + j sigma * (-z[j]) + a

one numpy ufunc call per float64 operation (one IEEE rounding, no fused multiply-add: __dmul_rn, __dadd_rn), so the values
are the device's bit for bit.  A float64 batch is the rows as they are, a float32 batch their round-to-nearest cast, an
int16 batch the engine's cast (tests/hsj_ref.py: cast_i16).  Not part of the product."""
import numpy as np

from tests.hsj_ref import cast_i16

SEED, STREAM, SIGMA = 77, 3, 0.001     # every case of the two test files


def rows_f64(a, z, sigma=SIGMA):
    """-> (2 half + 1, N) float64"""
    a = np.asarray(a, np.float64).reshape(-1)
    z = np.asarray(z)
    assert z.dtype == np.float32 and z.ndim == 2 and z.shape[1] == a.size, (z.dtype, z.shape, a.shape)
    z64 = z.astype(np.float64)
    s = np.float64(sigma)
    out = np.empty((2 * z.shape[0] + 1, a.size), np.float64)
    out[0] = a
    out[1:1 + z.shape[0]] = s * z64 + a[None, :]
    out[1 + z.shape[0]:] = s * (-z64) + a[None, :]
    return out


def rows(a, z, kind, sigma=SIGMA, bits=16):
    """kind: "float64" | "float32" | "int16" (with bits_per_sample = bits)"""
    x = rows_f64(a, z, sigma)
    if kind == "float64":
        return x
    if kind == "float32":
        return x.astype(np.float32)
    assert kind == "int16", kind
    return cast_i16(x, bits)


def bits_of(x):
    """the array as unsigned words of its element size: equality of these is equality of bits (-0.0 != 0.0, NaN == NaN)"""
    x = np.ascontiguousarray(x)
    return x.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[x.dtype.itemsize])


def padded(n):
    return (int(n) + 3) // 4 * 4


def pair_patterns(zrow):
    """The sign pattern of each Box-Muller pair of a padded row (its length a multiple of 4): an int array (len / 2,) of the
    quadrant q, since the sine and cosine factors are >= 0 -- (+, +) 0, (-, +) 1, (-, -) 2, (+, -) 3.  Pair 2 c of the result
    is the first pair of Philox counter c, pair 2 c + 1 its second."""
    zrow = np.asarray(zrow, np.float32).reshape(-1)
    assert zrow.size % 4 == 0, zrow.size
    n0, n1 = np.signbit(zrow[0::2]), np.signbit(zrow[1::2])
    return np.where(~n0 & ~n1, 0, np.where(n0 & ~n1, 1, np.where(n0 & n1, 2, 3)))


def last_counter_patterns(noise, n, halves, iters, seed=SEED, stream=STREAM):
    """The quadrants the last Philox counter of a row takes (the quad that holds sample n - 1), pooled over the rows of
    every half in `halves` and every iteration in `iters` -> (set of the first pair's, set of the second pair's).
    noise: oracle.noise."""
    first, second = set(), set()
    for half in halves:
        for it in iters:
            z = noise(seed, it, stream, padded(n), half)
            for j in range(half):
                q = pair_patterns(z[j])
                first.add(int(q[-2]))
                second.add(int(q[-1]))
    return first, second


# ---- the (route, N) groups of tests/test_gpu_nes_normals.py: {name: (the N, the half values, the iterations drawn)}
TINY_N = (1, 2, 3, 5, 254, 257, 1026)
UPD_N = (254, 257, 1026, 1024)
GMM_N = tuple(4096 + r for r in (0, 1, 2, 3, 5, 130))
PERTURB_HALVES = (7, 41)                          # (b), (c): ... and half = 63 at N = 2
UPD_HALVES = (1, 4, 7, 33, 40)                    # (d), (f)
GMM_PERTURB_HALVES = (1, 7, 41, 63)               # (e)


def groups():
    """Every (route, N) group as {name: (n, halves, iterations)}: what the coverage condition is asserted over."""
    g = {}
    for n in TINY_N:
        g["a k_noise N=%d" % n] = (n, (1, 16, 63), (0, 7))
        h = PERTURB_HALVES + ((63,) if n == 2 else ())
        g["b k_perturb_f64 N=%d" % n] = (n, h, (0, 1, 2))
        g["c k_perturb_x N=%d" % n] = (n, h, (0, 1, 2))
    for n in UPD_N:
        g["d k_update_perturb_x N=%d" % n] = (n, UPD_HALVES, (1, 2, 3))
    for n in GMM_N:
        g["e k_perturb N=%d" % n] = (n, GMM_PERTURB_HALVES, (0, 1, 2))
        g["f update N=%d" % n] = (n, UPD_HALVES, (1, 2, 3))
    return g
