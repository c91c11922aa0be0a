"""The i-vector chain against the CPU oracle AWAY from the D = 72 recipe: the kernels the engine switches to at other feature
dimensions, UBM sizes, T-matrix ranks and gselect counts (fb_load_ivector takes D <= 80, R <= 512, num_gselect <= 64).

Every case loads a synthetic system into its own Engine with the matching front-end, compares i-vectors and PLDA LLRs with
oracle.IvSystemCtx.score_batch at the tolerances of test_gpu_ivector.py, and asserts the gselect path it took
(engine.debug_iv_gselect()["path"]: 0 dump + k_iv_select, 1 general threshold form k_gmm_fx2_sel, 2 wide form k_gsel_w), so
that a change of the routing cannot silently stop exercising the kernel a case exists for.  A threshold-path case also
runs the dump path on the same batch: the same selection slot for slot and bit-identical i-vectors.

The kernels each shape reaches (NK = NKF = ceil((D + 1) / 16), at least 2; the threshold forms need 2 n_tiles >= 4 nsel, that
is C >= 1280 at nsel = 20; the wide form needs NK = 5, C % 32 == 0 and nsel <= 32):
  D = 60    general gselect NK = 4, k_iv_fullcov<42>, the generic statistics
  D = 39    NK = 3; odd D in the packed-triangle / statistics / contraction indexing
  D = 80    NK = 6, k_iv_fullcov<52> (D (D + 1) / 2 > 42 * 64)
  D = 24    NK = 2
  C = 2000  general gselect with a padded last tile at D != 72
  R = 50, R = 101   R (R + 1) / 2 odd or R odd: the k_iv_contract_gemm fallback of fb_launch_iv_contract
  nsel = 5 / 40 / 64   threshold forms with few selections; nsel > 32: dump path and k_iv_post; the upper bound

Batches of more than 32 768 frames get ONE component chunk (choose_chunks targets 512 blocks of 128-frame strips), so pass A
of the general form holds the maxima of all n_tiles tiles in LDS: 4096 NK + 1024 n_tiles bytes, above 64 KB at C = 2048 --
launch_gsel_t opts the kernel into more than the 64 KB default.  Those batches run on the general form (D = 60; D = 72 with
FB_GSEL_NARROW=1) and on the wide form (D = 72).

Last, the device's selection against an independent one: the oracle's diagonal log-likelihoods of every component, ranked
like gmm-gselect."""
import functools
import os

import numpy as np
import pytest

from fakebob_amd.engine import Engine
from fakebob_amd.models import IvectorSystem, synthetic_audio, synthetic_ivector_system

pytestmark = pytest.mark.gpu
SCORE_TOL = 1e-4
IVEC_RTOL = 1e-6
GSEL_ENV = ("FB_IV_GSEL_DUMP", "FB_GSEL_CAP", "FB_GSEL_NARROW", "FB_GSEL_A_HALF")
DUMP, GENERAL, WIDE = 0, 1, 2

FE_D60 = dict(num_ceps=20)
FE_D39 = dict(num_ceps=13)
FE_D80 = dict(num_ceps=20, num_mel_bins=23, delta_order=3, delta_window=2)
FE_D24 = dict(delta_order=0)


def _wav(utt, n):
    return (synthetic_audio(utt, n) * 32768.0).astype(np.int16)


def _threads():
    try:
        return max(1, min(32, len(os.sched_getaffinity(0))))
    except AttributeError:
        return 8


def _ragged(base=0):
    """Five utterances; two of them longer than the 300-frame CMN window."""
    return [_wav(base, 72000), _wav(base + 1, 16000), _wav(base + 2, 52345), _wav(base + 3, 9000), _wav(base + 4, 31000)]


@functools.lru_cache(maxsize=None)
def _system(C, D, R, L, nsel=20):
    sy = synthetic_ivector_system(C=C, D=D, R=R, L=L, n_speakers=2)
    sy = sy.with_enrolled(sy.enrolled, z_mean=[-40.0, -35.0], z_std=[10.0, 8.0])
    if nsel != sy.num_gselect:
        sy = IvectorSystem(sy.fg_weights, sy.fg_means_invcovars, sy.fg_inv_covars, sy.ie_M, sy.ie_sigma_inv, sy.prior_offset,
                           sy.mean_vec, sy.lda, sy.plda_mean, sy.plda_transform, sy.plda_psi, sy.enrolled, sy.z_mean, sy.z_std,
                           num_gselect=nsel, min_post=sy.min_post)
    return sy


def _engine(system, fe):
    e = Engine(0)
    try:
        if fe:
            e.set_frontend(**fe)
        assert e.feat_dim == system.D
        e.load_ivector(system, "OSI")
    except Exception:
        e.close()
        raise
    return e


def _run(engine, system, wavs, monkeypatch, **env):
    for k in GSEL_ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    llr, tv = engine.score_raw(wavs)
    sel, info = engine.debug_iv_gselect()
    ivs = engine.debug_ivectors(len(wavs), system.R)
    for k in GSEL_ENV:
        monkeypatch.delenv(k, raising=False)
    return llr, tv, sel, info, ivs


def _assert_oracle(ref, llr, tv, ivs, what):
    llr_o, ivs_o, tv_o = ref
    assert np.array_equal(tv, tv_o), what
    scale = max(1.0, np.abs(ivs_o).max())
    d_iv, d_llr = np.abs(ivs - ivs_o).max(), np.abs(llr - llr_o).max()
    print("%s: max |i-vector err| %.3g (scale %.3g), max |LLR err| %.3g" % (what, d_iv, scale, d_llr))
    assert d_iv <= IVEC_RTOL * scale, what
    assert d_llr <= SCORE_TOL, what


def _assert_same_as_dump(e, sy, wavs, monkeypatch, sel, ivs, what):
    """The threshold forms are exact by construction: the dump path's selection, slot for slot, and the same i-vectors
    bit for bit."""
    _, _, sel_d, info_d, ivs_d = _run(e, sy, wavs, monkeypatch, FB_IV_GSEL_DUMP="1")
    assert info_d["path"] == DUMP, what
    assert np.array_equal(sel_d, sel), what
    assert np.array_equal(ivs_d.view(np.uint64), ivs.view(np.uint64)), what


# (id, front-end overrides, C, D, R, L, num_gselect, path, env of the run)
SHAPES = [
    ("d60_general_nk4_fullcov42", FE_D60, 2048, 60, 100, 50, 20, GENERAL, {}),
    ("d39_odd_general_nk3", FE_D39, 1536, 39, 64, 32, 20, GENERAL, {}),
    ("d80_general_nk6_fullcov52", FE_D80, 1536, 80, 64, 32, 20, GENERAL, {}),
    ("d24_general_nk2", FE_D24, 1280, 24, 48, 24, 20, GENERAL, {}),
    ("d39_dump_small_ubm", FE_D39, 512, 39, 64, 32, 20, DUMP, {}),          # 2 n_tiles < 4 nsel: the dump at NK = 3
    ("d80_dump_small_ubm", FE_D80, 256, 80, 64, 32, 20, DUMP, {}),
    ("d60_c2000_padded_last_tile", FE_D60, 2000, 60, 64, 32, 20, GENERAL, {}),
    ("r50_odd_triangle_contract_fallback", {}, 256, 72, 50, 24, 20, DUMP, {}),
    ("r101_odd_rank_contract_fallback", {}, 256, 72, 101, 24, 20, DUMP, {}),
    ("nsel5_wide", {}, 2048, 72, 64, 32, 5, WIDE, {}),
    ("nsel5_general", {}, 2048, 72, 64, 32, 5, GENERAL, {"FB_GSEL_NARROW": "1"}),
    ("nsel40_dump_iv_post", {}, 2048, 72, 64, 32, 40, DUMP, {}),
    ("nsel64_dump_iv_post_upper_bound", {}, 2048, 72, 64, 32, 64, DUMP, {}),
]


@pytest.mark.parametrize("name,fe,C,D,R,L,nsel,path,env", SHAPES, ids=[s[0] for s in SHAPES])
def test_ivector_chain_matches_the_oracle_off_recipe(oracle, monkeypatch, name, fe, C, D, R, L, nsel, path, env):
    sy = _system(C, D, R, L, nsel)
    ctx = oracle.IvSystemCtx(oracle.default_cfg(**fe), sy, nthreads=_threads())
    wavs = _ragged(40)
    e = _engine(sy, fe)
    try:
        llr, tv, sel, info, ivs = _run(e, sy, wavs, monkeypatch, **env)
        assert info["path"] == path, (name, info)
        assert sel.shape == (int(np.sum(tv)), nsel)
        assert sel.min() >= 0 and sel.max() < C
        _assert_oracle(ctx.score_batch(wavs), llr, tv, ivs, name)
        if path != DUMP:
            assert info["overflow"] == 0
            _assert_same_as_dump(e, sy, wavs, monkeypatch, sel, ivs, name)
    finally:
        e.close()


# ---- batches of more than 32 768 frames: one component chunk
ONE_CHUNK = [
    ("d60_general", FE_D60, 60, GENERAL, {}),
    ("d72_narrow", {}, 72, GENERAL, {"FB_GSEL_NARROW": "1"}),
    ("d72_wide", {}, 72, WIDE, {}),
]


@functools.lru_cache(maxsize=None)
def _long_batch():
    return [_wav(60 + u, 30 * 16000) for u in range(13)]


@functools.lru_cache(maxsize=None)
def _long_oracle(D):
    """score_batch of the long batch (the D = 72 cases share it)."""
    from oracle import oracle as O
    fe = FE_D60 if D == 60 else {}
    sy = _system(2048, D, 64, 32)
    return O.IvSystemCtx(O.default_cfg(**fe), sy, nthreads=_threads()).score_batch(_long_batch())


@pytest.mark.parametrize("name,fe,D,path,env", ONE_CHUNK, ids=[s[0] for s in ONE_CHUNK])
def test_one_component_chunk_batch_matches_the_oracle_and_the_dump(oracle, monkeypatch, name, fe, D, path, env):
    sy = _system(2048, D, 64, 32)
    wavs = _long_batch()
    cfg = oracle.default_cfg(**fe)
    frames = sum(oracle.num_frames(cfg, w.size) for w in wavs)
    assert frames > 32768                                     # choose_chunks: 512 / strips < 2 -> one chunk of 64 tiles
    e = _engine(sy, fe)
    try:
        llr, tv, sel, info, ivs = _run(e, sy, wavs, monkeypatch, **env)
        assert info["path"] == path and info["chunks"] == 1, (name, info)
        assert info["overflow"] == 0
        assert info["rows"] == int(np.sum(tv)) == sel.shape[0]
        _assert_oracle(_long_oracle(D), llr, tv, ivs, "one chunk, %s, %d frames" % (name, frames))
        _assert_same_as_dump(e, sy, wavs, monkeypatch, sel, ivs, name)
    finally:
        e.close()


# ---- the selection against an independent reference
# The device computes each component's log-likelihood with f32-equivalent arithmetic (csrc/gmm_kernels.hip: the f16 matrix
# pipe with a two-term split).  At these magnitudes (|log-likelihood| < 512) a float32 ulp is at most 2^-14 = 6.1e-5 and a
# few ulps of the accumulation stay under 1e-4 nats; the oracle's values are float64 sums rounded to float32.  Two components
# whose oracle values are within that margin can legitimately come out in either order on the device -- and only those.
SEL_MARGIN = 1e-4
SEL = [
    ("d72_wide", {}, 72, WIDE, {}),
    ("d72_general", {}, 72, GENERAL, {"FB_GSEL_NARROW": "1"}),
    ("d60_general", FE_D60, 60, GENERAL, {}),
    ("d60_dump", FE_D60, 60, DUMP, {"FB_IV_GSEL_DUMP": "1"}),
]


def _oracle_component_loglikes(oracle, ctx, feats):
    """[frames, C] float32: each component's diagonal log-likelihood (a one-component GMM through diag_gmm_loglikes)."""
    C = ctx.dg_gc.shape[0]
    ll = np.empty((feats.shape[0], C), np.float32)
    for k in range(C):
        ll[:, k] = oracle.diag_gmm_loglikes(ctx.dg_gc[k:k + 1], ctx.dg_miv[k:k + 1], ctx.dg_iv[k:k + 1], feats)[0]
    return ll


def _gselect(ll, nsel):
    """gmm-gselect's order: descending (value, index) pairs (std::greater<pair<float, int>>)."""
    idx = np.broadcast_to(np.arange(ll.shape[1]), ll.shape)
    return np.lexsort((-idx, -ll), axis=-1)[:, :nsel]


@pytest.mark.parametrize("name,fe,D,path,env", SEL, ids=[s[0] for s in SEL])
def test_selection_equals_the_oracles_ranking(oracle, monkeypatch, name, fe, D, path, env):
    sy = _system(2048, D, 64, 32)
    cfg = oracle.default_cfg(**fe)
    ctx = oracle.IvSystemCtx(cfg, sy, nthreads=_threads())
    wavs = _ragged(80)
    e = _engine(sy, fe)
    try:
        _, tv, sel, info, _ = _run(e, sy, wavs, monkeypatch, **env)
    finally:
        e.close()
    assert info["path"] == path, (name, info)
    feats = np.concatenate([oracle.frontend(cfg, w)[0] for w in wavs])
    assert feats.shape == (int(np.sum(tv)), D) and sel.shape == (feats.shape[0], sy.num_gselect)
    ll = _oracle_component_loglikes(oracle, ctx, feats)
    ref = _gselect(ll, sy.num_gselect)
    rows = np.arange(ll.shape[0])[:, None]
    diff = sel != ref
    # a position may differ only where the oracle's values of the two components are within the margin
    gap = np.abs(ll[rows, sel].astype(np.float64) - ll[rows, ref].astype(np.float64))
    n_margin = int(np.sum(diff.any(axis=1)))
    worst = float(gap[diff].max()) if diff.any() else 0.0
    print("%s: %d of %d rows differ from the oracle's ranking, all within %.3g nats (worst %.3g)"
          % (name, n_margin, sel.shape[0], SEL_MARGIN, worst))
    assert np.all(gap[diff] <= SEL_MARGIN), (name, worst)
    assert n_margin <= max(2, sel.shape[0] // 100), (name, n_margin)
