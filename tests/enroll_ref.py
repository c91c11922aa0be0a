"""Plain numpy references of enrolment statistics (`gmm-global-acc-stats --update-flags=m`), for the tests of the dump,
k_gmm_lse and k_gmm_post_stats through Engine.debug_gmm_acc_rows.  Everything works on the float32 parameters and rows
widened to float64.

  ll64          gc + x.miv - x^2.iv / 2, the component log-likelihoods
  S             |gc| + |x|.|miv| + x^2.iv / 2, the magnitude their rounding scales with
  stats64       float64 soft-max of ANY ll, occ = sum_t p, F = p^T x, A = p^T |x| (the magnitude F's rounding scales with)
  stats_kaldi   the Kaldi-order twin fbo_gmm_acc_stats restates: float32 exp(ll - max), float32 SEQUENTIAL sum, scaled by
                the float32 1/sum, posteriors widened and accumulated in float64 in frame order
  stats_lanes   the same with the summation order of k_gmm_lse (64 strided partial sums, then the xor butterfly)

and the models, rows and tolerances the tests share (tests/test_enroll_ref_host.py checks on the CPU what the GPU tests
rely on)."""
import numpy as np

from fakebob_amd.models import DiagGmm, synthetic_gmm_system, synthetic_ubm_moments

SHRINK = 0.12
SEED = 5
# (C, D, T) of tests/test_gpu_enroll_stats.py and what each is there for
SHAPES = [
    (64, 39, 65),      # one exact 64-component slab, D % 4 = 3, one row past a 64-row staging round
    (65, 77, 129),     # a second slab holding one component (ld = 96), D % 4 = 1
    (100, 60, 130),    # a partial 32-tile and a partial slab at once
    (160, 72, 300),    # the front-end test's shape, now with shared posteriors
    (96, 80, 1100),    # FB_PS_DMAX4 full, 18 staging rounds, 9 dump strips
    (2048, 72, 130),   # the recipe's UBM: several component chunks in the dump
]
EPS_LL = 2e-6                    # per-component dump values: the relative figure the suite holds k_gmm_fx2 / k_gmm_bx3 to
GAMMA_FLOOR = 32 * 2.0 ** -24    # rounding of ll - max down to -16, expf, reciprocal, product, a short tree sum


def f64(a):
    return np.asarray(a, np.float32).astype(np.float64)


def ll64(gc, miv, iv, x):
    x = f64(x)
    return f64(gc)[None, :] + x @ f64(miv).T - 0.5 * ((x * x) @ f64(iv).T)


def S(gc, miv, iv, x):
    x = f64(x)
    return np.abs(f64(gc))[None, :] + np.abs(x) @ np.abs(f64(miv)).T + 0.5 * ((x * x) @ f64(iv).T)


def posteriors64(ll):
    ll = np.asarray(ll).astype(np.float64)
    e = np.exp(ll - ll.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def _accumulate(p, x):
    """occ, F, A of float64 posteriors p[T, C] and rows x[T, D], frames in order"""
    x = f64(x)
    occ = np.zeros(p.shape[1])
    F = np.zeros((p.shape[1], x.shape[1]))
    A = np.zeros_like(F)
    ax = np.abs(x)
    for t in range(p.shape[0]):
        occ += p[t]
        F += p[t][:, None] * x[t][None, :]
        A += p[t][:, None] * ax[t][None, :]
    return occ, F, A


def stats64(ll, x):
    return _accumulate(posteriors64(ll), x)


def _seq_sum32(e):
    return np.cumsum(e, axis=1, dtype=np.float32)[:, -1]


def _lane_sum32(e):
    """k_gmm_lse: lane l adds e[l], e[l + 64], ... in order, then s[l] += s[l ^ o] for o = 32 .. 1; lane 0's value"""
    T, C = e.shape
    pad = np.zeros((T, (C + 63) // 64 * 64), np.float32)
    pad[:, :C] = e
    s = np.zeros((T, 64), np.float32)
    for i in range(pad.shape[1] // 64):
        s = (s + pad[:, 64 * i:64 * i + 64]).astype(np.float32)
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        s = (s + s[:, lanes ^ o]).astype(np.float32)
    return s[:, 0]


def posteriors_kaldi(ll32, expf=np.exp, row_sum=_seq_sum32):
    ll32 = np.ascontiguousarray(ll32, np.float32)
    e = np.asarray(expf((ll32 - ll32.max(axis=1, keepdims=True)).astype(np.float32)), np.float32)
    inv = (np.float32(1.0) / row_sum(e)).astype(np.float32)
    return (e * inv[:, None]).astype(np.float32).astype(np.float64)


def stats_kaldi(ll32, x, expf=np.exp):
    """expf: the float32 exponential (numpy's by default; a test that compares with a C program bit for bit hands in
    that program's)."""
    return _accumulate(posteriors_kaldi(ll32, expf, _seq_sum32), x)


def stats_lanes(ll32, x):
    return _accumulate(posteriors_kaldi(ll32, np.exp, _lane_sum32), x)


def twin_distance(st, st_ref):
    """max_k |occ - occ_ref|_k / occ_ref,k and max_kd |F - F_ref|_kd / A_kd: the distance g_K of a float32 soft-max from
    the float64 one fed the same ll (a component the reference gives no mass at all has to be exactly empty)."""
    return max(_ratio(st[0], st_ref[0], st_ref[0]), _ratio(st[1], st_ref[1], st_ref[2]))


def _ratio(got, ref, scale):
    err = np.abs(np.asarray(got) - ref)
    return float(np.max(np.where(scale > 0.0, err / np.where(scale > 0.0, scale, 1.0), np.where(err > 0.0, np.inf, 0.0))))


def gamma(g_K):
    """tolerance (b), relative to occ_ref / A: the device sums in another order and its expf may differ by an ulp or two
    from numpy's -- four times the twin's own distance, and never below 32 float32 ulps"""
    return max(GAMMA_FLOOR, 4.0 * g_K)


def ratio_a(ll_dev, gc, miv, iv, x, where=False):
    """worst |ll_dev - ll64| / (EPS_LL * max(1, S)); with `where` also its (row, component)"""
    r = np.abs(np.asarray(ll_dev, np.float64) - ll64(gc, miv, iv, x)) / (EPS_LL * np.maximum(1.0, S(gc, miv, iv, x)))
    if where:
        return float(r.max()), tuple(int(i) for i in np.unravel_index(np.argmax(r), r.shape))
    return float(r.max())


def ratios_b(occ, F, ll_dev, x):
    """-> (worst error / (gamma * scale) over occ, F and the total, gamma, g_K, reference statistics) of k_gmm_lse +
    k_gmm_post_stats against float64 on the device's own ll"""
    ref = stats64(ll_dev, x)
    g_K = twin_distance(stats_kaldi(ll_dev, x), ref)
    g = gamma(g_K)
    T = np.asarray(ll_dev).shape[0]
    r = max(_ratio(occ, ref[0], g * ref[0]), _ratio(F, ref[1], g * ref[2]), abs(float(np.sum(occ)) - T) / (g * T))
    return r, g, g_K, ref


def ratio_c(occ, F, gc, miv, iv, x, g):
    """worst end-to-end error / first-order bound: a posterior moves by at most p_tk (eps_tk + sum_j p_tj eps_tj) when
    every ll moves by at most eps, eps_tk = EPS_LL * max(1, S_tk); plus (b)'s gamma on the sums"""
    p = posteriors64(ll64(gc, miv, iv, x))
    eps = EPS_LL * np.maximum(1.0, S(gc, miv, iv, x))
    dp = p * (eps + np.sum(p * eps, axis=1, keepdims=True))
    occ64, F64, A64 = _accumulate(p, x)
    b_occ = dp.sum(axis=0) + g * occ64
    b_F = dp.T @ np.abs(f64(x)) + g * A64
    return max(_ratio(occ, occ64, b_occ), _ratio(F, F64, b_F))


# ------------------------------------------------------------------------------------------------ models and rows
def moments(C, D):
    """w, mu, var of synthetic_gmm_system(1, C, D)'s UBM"""
    return synthetic_ubm_moments(C, D, 2001)


def overlapping_ubm(C, D, shrink=SHRINK):
    """The synthetic UBM with its means pulled to shrink * mu: the components overlap, so a frame's posterior is shared
    among several of them and every component is occupied (the unshrunk model's posteriors are nearly one-hot)."""
    w, mu, var = moments(C, D)
    ubm, _ = synthetic_gmm_system(1, C, D)
    return DiagGmm.from_internal(w, (shrink * mu / var).astype(np.float32), ubm.inv_vars)


def params(gmm):
    return gmm.gconsts, gmm.means_invvars, gmm.inv_vars


def shared(C, D, T, seed=SEED, shrink=SHRINK):
    """rows drawn from the overlapping model's own components"""
    _, mu, var = moments(C, D)
    rng = np.random.default_rng(seed)
    ks = rng.integers(0, C, T)
    return (shrink * mu[ks] + np.sqrt(var[ks]) * rng.standard_normal((T, D))).astype(np.float32)


def far(C, D, T, seed=SEED + 1, shrink=SHRINK):
    """rows 25 spreads away from every component"""
    _, mu, var = moments(C, D)
    rng = np.random.default_rng(seed)
    ks = rng.integers(0, C, T)
    sd = np.sqrt(var.mean(axis=0) + (shrink * mu).var(axis=0))
    return (shrink * mu[ks] + 25.0 * sd * rng.standard_normal((T, D))).astype(np.float32)


def zero(D, T):
    return np.zeros((T, D), np.float32)


def huge(D, T, seed=SEED + 2):
    """rows of magnitude 1e3 .. 1e4"""
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((T, D)) * np.logspace(3, 4, T)[:, None]).astype(np.float32)


def one_hot_rows(C, D, T, n_comp=32, seed=SEED + 3, out=1.0):
    """rows on components 0 .. n_comp - 1 of the UNSHRUNK synthetic UBM: posteriors are one-hot there to 1e-5 or so.  The
    other components' mass is tiny but not 0.0 in float32 (the components lie tens of nats apart, exp underflows at 104);
    out = 8 puts the rows at 8 mu_k, thousands of nats apart: most components then get exactly no mass."""
    _, mu, var = moments(C, D)
    rng = np.random.default_rng(seed)
    ks = rng.integers(0, n_comp, T)
    return (out * mu[ks] + np.sqrt(var[ks]) * rng.standard_normal((T, D))).astype(np.float32)
