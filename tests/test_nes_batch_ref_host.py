"""What tests/test_gpu_nes_normals.py stands on, checked without a GPU: properties of the reference alone.

1. The coverage condition.  fb_box_muller's quadrant chain has been compiled wrongly in single kernels, in single arms.  A
   case proves something about a launch only if the lanes that matter draw every quadrant: for each (route, N) group of the
   GPU file, the expected normals of the LAST Philox counter of a row (the quad that holds sample N - 1: the partly filled
   one, in the partly filled wave), pooled over the group's half values and iterations, show all four sign patterns in the
   counter's first pair and in its second.
2. oracle.noise at N is a prefix of oracle.noise at N rounded up to a multiple of 4, row by row: the padded rows (1) reads
   are the rows the GPU tests compare.
3. The restatement itself, against a scalar Python loop, and the sign-pattern helper on hand-made pairs."""
import numpy as np
import pytest

from tests import nes_batch_ref as R


@pytest.mark.parametrize("name", sorted(R.groups()))
def test_last_counter_draws_every_quadrant_in_both_pairs(oracle, name):
    n, halves, iters = R.groups()[name]
    first, second = R.last_counter_patterns(oracle.noise, n, halves, iters)
    assert first == {0, 1, 2, 3}, (name, "first pair", sorted(first))
    assert second == {0, 1, 2, 3}, (name, "second pair", sorted(second))


def test_single_halves_that_cover_alone_and_those_that_do_not(oracle):
    """Half 7, 33 and 40 each cover every N = 4096 + r alone, over iterations 0 - 2 and over 1 - 3; the tiny N at half 63 in
    iteration 0 alone.  Half 4 at N = 4101 over iterations 0 - 2 does not: such a half counts only inside its group's pool."""
    full = {0, 1, 2, 3}
    for n in R.GMM_N:
        for half in (7, 33, 40):
            for iters in ((0, 1, 2), (1, 2, 3)):
                assert R.last_counter_patterns(oracle.noise, n, (half,), iters) == (full, full), (n, half, iters)
    for n in R.TINY_N:
        assert R.last_counter_patterns(oracle.noise, n, (63,), (0,)) == (full, full), n
    first, second = R.last_counter_patterns(oracle.noise, 4101, (4,), (0, 1, 2))
    assert first != full or second != full


@pytest.mark.parametrize("n", sorted(set(R.TINY_N + R.UPD_N + R.GMM_N)))
def test_noise_is_a_prefix_of_the_padded_noise(oracle, n):
    for half, it in ((1, 0), (7, 2), (63, 7)):
        z = oracle.noise(R.SEED, it, R.STREAM, n, half)
        zp = oracle.noise(R.SEED, it, R.STREAM, R.padded(n), half)
        assert z.dtype == np.float32 and z.shape == (half, n) and zp.shape == (half, R.padded(n))
        assert np.array_equal(R.bits_of(z), R.bits_of(zp[:, :n])), (n, half, it)


def test_pair_patterns_on_hand_made_pairs():
    z = np.array([1.0, 2.0, -1.0, 2.0, -1.0, -2.0, 1.0, -2.0, 0.0, 0.0, -0.0, 0.0, -0.0, -0.0, 0.0, -0.0], np.float32)
    assert R.pair_patterns(z).tolist() == [0, 1, 2, 3, 0, 1, 2, 3]   # (a zero factor keeps its sign bit)


def test_rows_against_a_scalar_loop(oracle):
    n, half = 5, 3
    z = oracle.noise(R.SEED, 1, R.STREAM, n, half)
    a = np.linspace(-0.9, 0.9, n) + 1e-7
    x = R.rows_f64(a, z)
    assert x.shape == (2 * half + 1, n) and x.dtype == np.float64
    for k in range(n):
        assert x[0, k] == a[k]
        for j in range(half):
            zz = float(z[j, k])                                       # Python floats: one rounding per operation
            assert x[1 + j, k] == 0.001 * zz + a[k]
            assert x[1 + half + j, k] == 0.001 * (-zz) + a[k]
    assert np.array_equal(R.rows(a, z, "float32"), x.astype(np.float32))
    q16, q8 = R.rows(a, z, "int16"), R.rows(a, z, "int16", bits=8)
    assert q16.dtype == np.int16 and np.array_equal(q16, np.trunc(x * 32768.0).astype(np.int64).astype(np.int16))
    assert np.array_equal(q8, np.trunc(x * 128.0).astype(np.int64).astype(np.int16))
    assert np.array_equal(R.bits_of(np.array([0.0, -0.0])), np.array([0, 1 << 63], np.uint64))
