"""k_gmm_fx2w's parameter fetches in runs of up to four pieces (fb_glds16_at), at the smallest shapes where a run can go wrong.

A wave brings PW = ceil(10 G / 4) one-kilobyte pieces of a group of G items, five at the head of the group and five per step
after it, each five as a run of four behind one M0 value and one address plus a run of one.  The models counts below give
groups of 2/1, 2/2, 4/3, 4/4 and 6/5 items, i.e. PW = 5/3, 5/5, 10/8, 10/10 and 15/13 pieces: remainders 0 .. 3 modulo four,
steps with 0, 3 and 5 pieces, groups that end inside a run.  One, two and three component tiles, as one chunk (the tile loop's
back edge: the next tile's first group is fetched under this tile's second) and as one tile per chunk (no next tile: the
clamped refetch), one and two chunks per workgroup; 1, 65 and 257 rows (a lone row, a second wave with one row, a second strip
with one row); every tile class.  A stale or misplaced piece shows against the float64 formula, between the two sub-chunk
forms, or between two calls on one engine."""
import os

import numpy as np
import pytest

from fakebob_amd.engine import Engine
from fakebob_amd.models import synthetic_gmm_system

pytestmark = pytest.mark.gpu
MODELS = (2, 3, 6, 7, 10)
COMPONENTS = (32, 64, 96)
ROWS = (1, 65, 257)
KNOBS = ("FB_GMM_TARGET_BLOCKS", "FB_GMM_SUB", "FB_GMM_NARROW", "FB_GMM_MODE", "FB_GMM_DELTA_P")


@pytest.fixture(autouse=True)
def _clean_knobs(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


def _frame_lls(models, x):
    """float64 reference of gmm-global-get-frame-likes: [M, T] from [T, D] features"""
    x = np.asarray(x, np.float64)
    out = []
    for m in models:
        ll = (m.gconsts.astype(np.float64)[None, :] + x @ m.means_invvars.astype(np.float64).T
              - 0.5 * (x * x) @ m.inv_vars.astype(np.float64).T)
        mx = ll.max(axis=1)
        out.append(mx + np.log(np.exp(ll - mx[:, None]).sum(axis=1)))
    return np.stack(out)


def _draw(ubm, n, seed):
    rng = np.random.default_rng(seed)
    var = 1.0 / ubm.inv_vars.astype(np.float64)
    mu = ubm.means_invvars.astype(np.float64) * var
    ks = rng.integers(0, var.shape[0], n)
    return (mu[ks] + np.sqrt(var[ks]) * rng.standard_normal((n, var.shape[1]))).astype(np.float32)


@pytest.fixture(scope="module")
def cases():
    """(models, {rows: (features, float64 per-frame values)}) of every (model count, component count), computed once"""
    out = {}
    for M in MODELS:
        for C in COMPONENTS:
            # the enrolment frames per component of the SURVEY.md 8(d) system (200 on 2048 components): a forced tile class 1
            # drops the delta items' two cross products, 2^-12 of |delta . x|, and is only what fb_load_gmm would pick --
            # and the 1e-4 of the raw scores only holds -- where the speakers moved the means as little as they do there
            ubm, spk = synthetic_gmm_system(n_speakers=M - 1, C=C, D=72, enrol_frames=200.0 * C / 2048.0)
            models = [ubm] + spk
            feats = _draw(ubm, max(ROWS), 100 * M + C)
            want = _frame_lls(models, feats)
            out[(M, C)] = (models, {T: (feats[:T], want[:, :T]) for T in ROWS})
    return out


@pytest.mark.parametrize("tile_class", ["1", "3", "6"])
def test_fetch_runs_at_every_group_size_tile_count_and_strip_edge(cases, tile_class, monkeypatch):
    monkeypatch.setenv("FB_GMM_DELTA_P", tile_class)     # read when the model is loaded: the same class in every tile
    worst, n_runs, over = 0.0, 0, []
    for (M, C), (models, by_rows) in cases.items():
        e = Engine(0)
        try:
            e.load_gmm(models)
            assert e.gmm_kernel_variant.startswith("fx2w/"), (M, C, e.gmm_kernel_variant)
            for T, (feats, want) in by_rows.items():
                strips = (T + 255) // 256
                for n in sorted({1, C // 32}):           # one chunk of every tile | one tile per chunk
                    got = {}
                    for sub in (1, 2):
                        os.environ["FB_GMM_TARGET_BLOCKS"] = str(strips * n)
                        os.environ["FB_GMM_SUB"] = str(sub)
                        try:
                            a = e.debug_gmm_frames(feats)
                            sh = e.debug_launch_shape()
                            b = e.debug_gmm_frames(feats)
                        finally:
                            os.environ.pop("FB_GMM_TARGET_BLOCKS")
                            os.environ.pop("FB_GMM_SUB")
                        label = (tile_class, M, C, T, n, sub)
                        assert sh["gmm"] == "fx2w" and sh["n_chunks"] == n and sh["strips"] == strips, (label, sh)
                        assert sh["sub"] == (sub if n % sub == 0 else 1), (label, sh)
                        # a second call on the same engine: the slots start from what the first one left in them
                        assert np.array_equal(a.view(np.uint64), b.view(np.uint64)), label
                        got[sub] = a
                        n_runs += 1
                    assert np.array_equal(got[1].view(np.uint64), got[2].view(np.uint64)), (tile_class, M, C, T, n)
                    # raw scores: a model's mean log-likelihood over the rows, as score_raw averages them
                    assert np.isfinite(got[1]).all(), (tile_class, M, C, T, n)
                    err = float(np.abs(got[1].mean(axis=1) - want.mean(axis=1)).max())
                    worst = max(worst, err)
                    if err > 1e-4:
                        over.append((M, C, T, n, err))
        finally:
            e.close()
    print("tile class %s: %d launches compared, worst raw-score error %.2e" % (tile_class, 2 * n_runs, worst))
    assert not over, (tile_class, over)
    assert n_runs == len(MODELS) * len(ROWS) * (1 + 2 + 2) * 2
