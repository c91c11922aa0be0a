"""The launch shapes of a GPU shared by three or more attacks (fb_set_fused_chain(e, 0): what bench.py's headline number
runs) and the component-chunk splits around them, each against an independent reference.

  - k_gmm_fx2w with one or two component chunks per workgroup (FB_GMM_SUB), over every chunk count FB_GMM_TARGET_BLOCKS
    reaches: uneven tiles per chunk, odd chunk counts, XCD-mapped grids of 1 .. 8 chunks next to the plain 2-D grid, tile
    classes falling into different chunks, several passes -- per-frame values against the float64 formula, and the two
    sub-chunk forms bit for bit;
  - the same sweep for k_gmm_fx2 (FB_GMM_NARROW=1) and k_gmm_bx3 (FB_GMM_MODE=bx3), with a padded last tile and a short
    last chunk;
  - the XCD mapping switched off (FB_GMM_NO_XCD_MAP, read once per process: a child process) against the mapped runs;
  - k_mfcc_f32 on 1 .. 255 compute units (FB_MFCC_CUS), i.e. over several rounds, against the oracle's float32 twin;
  - configs[1] and configs[2] at full size with the unfused launch chain against the fused one and the oracle;
  - the gselect kernels at 1, 2, 4 and 8 selection chunks against the dump path.
Every case asserts the shape it ran (Engine.debug_launch_shape), and every sweep the set of shapes it reached."""
import os
import subprocess
import sys

import numpy as np
import pytest

from fakebob_amd._native import FB_E_STATE, NativeError
from fakebob_amd.engine import Engine, nes_params
from fakebob_amd.models import ENROL_REALISTIC, stack_models, synthetic_audio, synthetic_gmm_system, synthetic_ivector_system

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NTHR = max(1, min(16, len(os.sched_getaffinity(0))))
COUNTS = (1, 2, 3, 4, 5, 7, 8, 13, 16, 22, 32, 64)
KNOBS = ("FB_GMM_TARGET_BLOCKS", "FB_GMM_SUB", "FB_GMM_NARROW", "FB_GMM_MODE", "FB_GMM_DELTA_P", "FB_MFCC_CUS",
         "FB_MFCC_HALFWORDS", "FB_MFCC_RECORDS", "FB_GSEL_TARGET_BLOCKS", "FB_GSEL_NARROW", "FB_IV_GSEL_DUMP")


@pytest.fixture(autouse=True)
def _clean_knobs(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


def _wav(utt, n):
    return (synthetic_audio(utt, n) * 32768.0).astype(np.int16)


def _frame_lls(models, x):
    """float64 reference of gmm-global-get-frame-likes: [M, T] from [T, D] features."""
    x = np.asarray(x, np.float64)
    out = []
    for m in models:
        ll = (m.gconsts.astype(np.float64)[None, :] + x @ m.means_invvars.astype(np.float64).T
              - 0.5 * (x * x) @ m.inv_vars.astype(np.float64).T)
        mx = ll.max(axis=1)
        out.append(mx + np.log(np.exp(ll - mx[:, None]).sum(axis=1)))
    return np.stack(out)


def _rows(ubm, n=2500, seed=7):
    """n feature rows drawn from the UBM's components: ten 256-frame strips, the last one ragged (196 rows)."""
    rng = np.random.default_rng(seed)
    var = 1.0 / ubm.inv_vars.astype(np.float64)
    mu = ubm.means_invvars.astype(np.float64) * var
    ks = rng.integers(0, var.shape[0], n)
    return (mu[ks] + np.sqrt(var[ks]) * rng.standard_normal((n, var.shape[1]))).astype(np.float32)


def _system(name):
    """The models of a sweep system (deterministic: the child process rebuilds them)."""
    if name == "realistic":
        ubm, spk = synthetic_gmm_system(n_speakers=5, C=2048, D=72, **ENROL_REALISTIC)
    elif name == "pass2":
        ubm, spk = synthetic_gmm_system(n_speakers=18, C=2048, D=72)
    elif name == "c2000":
        ubm, spk = synthetic_gmm_system(n_speakers=5, C=2000, D=72)
    else:
        ubm, spk = synthetic_gmm_system(n_speakers=5, C=2048, D=72)
    return [ubm] + spk


ENVS = {"fx2w": {}, "fx2w/3": {"FB_GMM_DELTA_P": "3"}, "fx2w/6": {"FB_GMM_DELTA_P": "6"},
        "fx2": {"FB_GMM_NARROW": "1"}, "bx3": {"FB_GMM_MODE": "bx3"}}


def _sweep(models, kernel, counts, subs, rows):
    """debug_gmm_frames at every chunk count x sub-chunk setting: {(n, sub): (per-frame values, recorded shape)}.  The
    process environment selects the kernel (ENVS[kernel], set by the caller before the model is loaded)."""
    strip = 256 if kernel.startswith("fx2w") else 128
    strips = (rows.shape[0] + strip - 1) // strip
    e = Engine(0)
    out = {}
    try:
        e.load_gmm(models)
        assert e.gmm_kernel_variant.split("/")[0] == kernel.split("/")[0], (kernel, e.gmm_kernel_variant)
        for n in counts:
            for sub in subs:
                os.environ["FB_GMM_TARGET_BLOCKS"] = str(strips * n)   # choose_chunks: want = target / strips
                os.environ["FB_GMM_SUB"] = str(sub)
                got = e.debug_gmm_frames(rows)
                out[(n, sub)] = (got, e.debug_launch_shape())
    finally:
        os.environ.pop("FB_GMM_TARGET_BLOCKS", None)
        os.environ.pop("FB_GMM_SUB", None)
        e.close()
    return out


def _check_shape(sh, kernel, n, sub, strips, n_tiles, passes=1):
    """What the launchers recorded, against what each kernel's launch rule says."""
    assert sh["gmm"] == kernel.split("/")[0] and sh["n_chunks"] == n and sh["strips"] == strips and sh["passes"] == passes, sh
    assert sh["cus"] == sh["rounds"] == sh["blocks"] == 0, sh                      # no front end in this hook
    if sh["gmm"] == "fx2w":                      # strided: chunk c scores tiles c, c + n, ...
        eff = sub if n % sub == 0 else 1
        assert sh["sub"] == eff and sh["grid_chunks"] == n // eff, sh
        assert (sh["tiles_min"], sh["tiles_max"]) == (n_tiles // n, -(-n_tiles // n)), sh
    else:                                        # contiguous ranges of tpc tiles, the last chunk what is left
        tpc = -(-n_tiles // n)
        assert sh["sub"] == 1 and sh["grid_chunks"] == n, sh
        assert (sh["tiles_min"], sh["tiles_max"]) == (n_tiles - (n - 1) * tpc, tpc) and sh["tiles_min"] >= 1, sh
    assert sh["xcd_map"] == (sh["grid_chunks"] if sh["grid_chunks"] in (1, 2, 4, 8) else 0), sh


def _assert_close(got, want, kernel, label):
    assert np.isfinite(got).all(), label
    rel = np.abs(got - want) / np.maximum(1.0, np.abs(want))
    sysd = np.abs((got[1:] - got[:1]) - (want[1:] - want[:1]))
    # the bounds of test_wide_kernel_reference_rescue_and_range_paths (rows drawn from the model): float32 accumulation
    # of values ~1e2, the speaker rows of the fx2w classes P < 3 carrying the dropped products (~1e-4 per frame)
    assert rel[0].max() <= 2e-6, (label, rel[0].max())
    assert rel.max() <= (2e-6 if kernel == "fx2w/3" else 1e-5), (label, rel.max())
    assert sysd.max() <= 2e-3, (label, sysd.max())
    return rel.max()


@pytest.fixture(scope="module")
def systems():
    """Each sweep system with its rows and their float64 per-frame values, computed once."""
    out = {}
    for name in ("default", "realistic", "pass2", "c2000"):
        models = _system(name)
        rows = _rows(models[0])
        out[name] = (models, rows, _frame_lls(models, rows))
    return out


def test_launch_shape_is_a_state_error_before_the_first_batch():
    e = Engine(0)
    try:
        with pytest.raises(NativeError) as ei:
            e.debug_launch_shape()
        assert ei.value.code == FB_E_STATE
    finally:
        e.close()


@pytest.mark.parametrize("variant", ["fx2w", "fx2w/3", "fx2w/6", "realistic"])
def test_wide_kernel_over_every_chunk_count_and_both_sub_chunk_forms(systems, variant):
    """k_gmm_fx2w through fb_debug_gmm_frames: 2 500 rows (10 strips, the last ragged) at every chunk count of COUNTS, one
    and two chunks per workgroup.  Per-frame values against float64; the two forms bit for bit (the kernel promises the same
    partial sums: each sub-chunk starts from the state of a fresh workgroup).  The heavily enrolled system at 4 and 5 chunks
    is what caught the kernel's tail adding a deferred update to a state a rescue had moved off the tile's reference."""
    kernel = "fx2w" if variant == "realistic" else variant
    models, rows, want = systems["realistic" if variant == "realistic" else "default"]
    for k, v in ENVS[kernel].items():
        os.environ[k] = v
    try:
        res = _sweep(models, kernel, COUNTS, (1, 2), rows)
    finally:
        for k in ENVS[kernel]:
            os.environ.pop(k, None)
    seen = set()
    worst = 0.0
    for (n, sub), (got, sh) in res.items():
        _check_shape(sh, kernel, n, sub, 10, 64)
        seen.add((sh["n_chunks"], sh["sub"], sh["grid_chunks"], sh["xcd_map"]))
        worst = max(worst, _assert_close(got, want, kernel, (variant, n, sub)))
    for n in COUNTS:
        a, b = res[(n, 1)][0], res[(n, 2)][0]
        assert np.array_equal(a.view(np.uint64), b.view(np.uint64)), (variant, n)
    print("%s: %d shapes, worst relative error %.2e" % (variant, len(seen), worst))
    # the shapes the sweep must reach: an odd grid under sub = 2 (22 -> 11), an odd count where sub falls back to 1,
    # XCD-mapped grids of 1, 2, 4 and 8 chunks in either form, uneven tiles per chunk, the plain 2-D grid
    need = {(22, 2, 11, 0), (13, 1, 13, 0), (64, 2, 32, 0), (1, 1, 1, 1), (2, 1, 2, 2), (4, 1, 4, 4), (8, 1, 8, 8),
            (2, 2, 1, 1), (4, 2, 2, 2), (8, 2, 4, 4), (16, 2, 8, 8), (5, 1, 5, 0), (3, 1, 3, 0)}
    assert need <= seen, sorted(need - seen)
    assert any(r[1]["tiles_min"] < r[1]["tiles_max"] for r in res.values())


def test_wide_kernel_in_two_passes_with_two_sub_chunks(systems):
    """UBM + 18 speakers: two launches of k_gmm_fx2w (nine delta models each), both with the sub-chunk form."""
    models, rows, want = systems["pass2"]
    res = _sweep(models, "fx2w", (4, 13, 22), (1, 2), rows)
    for (n, sub), (got, sh) in res.items():
        _check_shape(sh, "fx2w", n, sub, 10, 64, passes=2)
        _assert_close(got, want, "fx2w", ("pass2", n, sub))
    for n in (4, 13, 22):
        assert np.array_equal(res[(n, 1)][0].view(np.uint64), res[(n, 2)][0].view(np.uint64)), n
    assert {(r[1]["n_chunks"], r[1]["grid_chunks"]) for r in res.values()} >= {(4, 2), (13, 13), (22, 11)}


@pytest.mark.parametrize("kernel", ["fx2", "bx3"])
@pytest.mark.parametrize("system", ["default", "c2000"])
def test_narrow_kernels_over_chunk_counts(systems, kernel, system):
    """k_gmm_fx2 and k_gmm_bx3 (contiguous ranges of tpc tiles per chunk) at C = 2048 and at C = 2000 (63 tiles, the last
    one padded): short last chunks, XCD-mapped grids of 1, 2, 4 and 8 chunks, the plain grid.  FB_GMM_SUB changes nothing
    here."""
    models, rows, want = systems[system]
    n_tiles = -(-models[0].gconsts.shape[0] // 32)
    counts = COUNTS if system == "default" else (1, 2, 3, 4, 5, 7, 8, 13, 16, 32)
    for k, v in ENVS[kernel].items():
        os.environ[k] = v
    try:
        res = _sweep(models, kernel, counts, (1, 2), rows)
    finally:
        for k in ENVS[kernel]:
            os.environ.pop(k, None)
    seen = set()
    for (n, sub), (got, sh) in res.items():
        _check_shape(sh, kernel, n, 1, 20, n_tiles)
        seen.add((sh["n_chunks"], sh["xcd_map"], sh["tiles_min"] < sh["tiles_max"]))
        _assert_close(got, want, "fx2w/3", (kernel, system, n, sub))
        assert np.array_equal(got.view(np.uint64), res[(n, 1)][0].view(np.uint64)), (kernel, system, n)
    need = {(1, 1, False), (2, 2, False), (4, 4, False), (8, 8, False), (5, 0, True), (13, 0, True)}
    if system == "c2000":
        need = {(1, 1, False), (2, 2, True), (4, 4, True), (8, 8, True), (5, 0, True), (16, 0, True), (7, 0, False)}
    assert need <= seen, sorted(need - seen)


CHILD = r'''
import os, sys
import numpy as np
sys.path.insert(0, %(root)r)
from tests.test_gpu_launch_shapes import ENVS, _rows, _sweep, _system
out = {}
for kernel, name, subs in (("fx2w", "default", (1, 2)), ("fx2", "default", (1,)), ("bx3", "c2000", (1,))):
    models = _system(name)
    rows = _rows(models[0])
    os.environ.update(ENVS[kernel])
    for (n, sub), (got, sh) in _sweep(models, kernel, (1, 2, 4, 8, 16), subs, rows).items():
        assert sh["xcd_map"] == 0 and sh["n_chunks"] == n, sh
        out["%%s_%%d_%%d" %% (kernel, n, sub)] = got
    for k in ENVS[kernel]:
        os.environ.pop(k)
np.savez(sys.argv[1], **out)
'''


def test_plain_grid_equals_the_xcd_mapped_grid(systems, tmp_path):
    """FB_GMM_NO_XCD_MAP (read once per process): the chunk counts the mapping takes, on the plain 2-D grid in a fresh
    child process, bit for bit against the mapped launches of this one."""
    path = str(tmp_path / "plain.npz")
    env = dict(os.environ, FB_GMM_NO_XCD_MAP="1")
    r = subprocess.run([sys.executable, "-c", CHILD % {"root": ROOT}, path], env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:]
    plain = np.load(path)
    n_cmp = 0
    for kernel, name, subs in (("fx2w", "default", (1, 2)), ("fx2", "default", (1,)), ("bx3", "c2000", (1,))):
        models, rows, _ = systems[name]
        for k, v in ENVS[kernel].items():
            os.environ[k] = v
        try:
            res = _sweep(models, kernel, (1, 2, 4, 8, 16), subs, rows)
        finally:
            for k in ENVS[kernel]:
                os.environ.pop(k, None)
        for (n, sub), (got, sh) in res.items():
            assert sh["xcd_map"] == (sh["grid_chunks"] if sh["grid_chunks"] in (1, 2, 4, 8) else 0), sh
            key = "%s_%d_%d" % (kernel, n, sub)
            assert np.array_equal(got.view(np.uint64), plain[key].view(np.uint64)), key
            n_cmp += 1
    assert n_cmp == len(plain.files) == 20


# ---------------------------------------------------------------------------------------------------------- k_mfcc_f32
CUS = (1, 3, 7, 64, 128, 255, None)


def _set_cus(cus):
    if cus is None:
        os.environ.pop("FB_MFCC_CUS", None)
    else:
        os.environ["FB_MFCC_CUS"] = str(cus)


def _check_mfcc_shape(sh, cus, frames):
    groups = -(-frames // 4)
    c = cus if cus is not None else 256
    assert sh["cus"] == c and sh["rounds"] == -(-groups // (16 * c)), (sh, cus, frames)
    assert sh["blocks"] <= c and sh["blocks"] * sh["rounds"] * 16 >= groups, sh


def test_mfcc_f32_over_rounds_is_bit_identical_to_the_oracle_twin(oracle, small_system):
    """k_mfcc_f32 held to 1 .. 255 compute units: each wave walks its groups of four frames over several rounds and prefetches
    the next one.  Lone utterances (debug_mfcc) bit for bit against the oracle's float32 twin; a ragged batch (per-frame
    records) and an equal-length one (records computed from the common length) with the same scores at every unit count,
    within 2e-5 of the twin."""
    cfg32 = oracle.default_cfg(mfcc_f32=1)
    utts = [_wav(0, 48000), _wav(1, 128000)]
    want = [oracle.mfcc(cfg32, w) for w in utts]
    rng = np.random.default_rng(3)
    ragged = [_wav(20 + k, int(n)) for k, n in enumerate(rng.integers(16000, 96000, size=30))]
    equal = [_wav(50 + k, 48000) for k in range(51)]
    ubm, spk = small_system
    models = [ubm] + spk
    gc, miv, iv = stack_models(models)
    twin = {name: oracle.gmm_score_batch(cfg32, b, gc, miv, iv, nthreads=NTHR) for name, b in (("ragged", ragged), ("equal", equal))}
    e = Engine(0)
    e.set_frontend(mfcc_f32=1)
    ref = {}
    rounds = {}
    try:
        e.load_gmm(models)
        for variant in ("default", "FB_MFCC_HALFWORDS", "FB_MFCC_RECORDS"):
            if variant != "default":
                os.environ[variant] = "1"
            try:
                for cus in (CUS if variant == "default" else (3,)):
                    _set_cus(cus)
                    for w, mo in zip(utts, want):
                        mg = e.debug_mfcc(w)
                        sh = e.debug_launch_shape()
                        _check_mfcc_shape(sh, cus, mg.shape[0])
                        assert sh["gmm"] is None
                        rounds[(cus, w.size)] = sh["rounds"]
                        same = mg.view(np.uint32) == mo.view(np.uint32)
                        zero = (mg == 0.0) & (mo == 0.0)
                        assert mg.shape == mo.shape and np.all(same | zero), (variant, cus, w.size, int((~(same | zero)).sum()))
                    for name, batch in (("ragged", ragged), ("equal", equal)):
                        raw, tv = e.score_raw(batch)
                        sh = e.debug_launch_shape()
                        frames = sum(e._num_frames(w.size) for w in batch)
                        _check_mfcc_shape(sh, cus, frames)
                        rounds[(cus, name)] = sh["rounds"]
                        raw_o, tv_o = twin[name]
                        assert np.array_equal(tv, tv_o) and np.abs(raw - raw_o).max() <= 2e-5, (variant, cus, name)
                        if name not in ref:
                            ref[name] = raw
                        assert np.array_equal(raw.view(np.uint64), ref[name].view(np.uint64)), (variant, cus, name)
            finally:
                os.environ.pop(variant, None)
                os.environ.pop("FB_MFCC_CUS", None)
    finally:
        e.close()
    print("k_mfcc_f32 rounds:", rounds)
    assert min(rounds[(c, n)] for c in (1, 3) for n in (48000, 128000)) >= 2 and rounds[(7, 128000)] >= 2
    assert rounds[(128, "equal")] == 2 and rounds[(128, "ragged")] >= 2 and rounds[(1, "equal")] >= 100
    assert rounds[(None, "equal")] == 1


# ------------------------------------------------------------------------------------------ the shared configuration
KW = dict(samples_per_draw=50, epsilon=0.002, sigma=0.001, max_lr=0.001, min_lr=1e-6, momentum=0.9,
          plateau_length=5, plateau_drop=2.0, adver_thresh=0.0, target=0, threshold=0.2277)


def test_config1_unfused_chain_at_full_size(oracle, full_system):
    """configs[1] (UBM + 5, C = 2048, spd = 50, 3 s, mfcc_f32 = 1) on the launch chain of a shared GPU: k_gmm_fx2w with two
    chunks per workgroup, k_mfcc_f32 in two rounds on 128 units.  get_grad and a 3-iteration attack bit for bit against
    the fused chain, get_grad within test_config1_get_grad_and_attack_at_full_size's bounds of the oracle twin."""
    ubm, spk = full_system
    models = [ubm] + spk
    audio = synthetic_audio(0, 48000)
    res = {}
    for fused in (False, True):
        e = Engine(0)
        try:
            e.set_frontend(mfcc_f32=1)
            e.load_gmm(models)
            e.set_system("OSI")
            e.set_fused_chain(fused)
            pg = nes_params("OSI", "targeted", seed=42, stream=0, max_iter=1000, **KW)
            flg, gg, alg, scg = e.get_grad(pg, audio, it=0)
            sh = e.debug_launch_shape()
            assert sh["gmm"] == "fx2w" and sh["strips"] * 256 >= 51 * 150, sh
            if fused:
                assert sh["sub"] == 1 and sh["grid_chunks"] == sh["n_chunks"] and sh["cus"] == 256 and sh["rounds"] == 1, sh
            else:
                assert sh["sub"] == 2 and 2 * sh["grid_chunks"] == sh["n_chunks"], sh
                assert sh["cus"] == 128 and sh["rounds"] == 2, sh
            pg.max_iter = 3
            adv, flag, advf, tr = e.attack(pg, audio)
            sh = e.debug_launch_shape()
            assert sh["sub"] == (1 if fused else 2) and sh["rounds"] == (1 if fused else 2), sh
            res[fused] = (flg, gg, alg, scg, adv, flag, advf, tr)
        finally:
            e.close()
    a, b = res[False], res[True]
    assert a[0] == b[0] and a[2] == b[2] and a[5] == b[5]
    for x, y in zip((a[1], a[3], a[6], a[7]), (b[1], b[3], b[6], b[7])):
        assert np.array_equal(np.asarray(x).view(np.uint64), np.asarray(y).view(np.uint64))
    assert np.array_equal(a[4], b[4])
    gc, miv, iv = stack_models(models)
    ctx = oracle.GmmSystemCtx(oracle.default_cfg(mfcc_f32=1), "OSI", gc, miv, iv, nthreads=NTHR)
    po = oracle.nes_params("OSI", "targeted", ctx.S, max_iter=1000, **KW)
    flo, go, alo, sco = oracle.get_grad(po, ctx.fn, ctx.ctx, audio, seed=42, it=0, stream=0)
    flg, gg, alg, scg = a[:4]
    assert abs(alg - alo) <= 1e-4 and abs(flg - flo) <= 1e-4
    assert np.abs(scg[:ctx.S] - sco).max() <= 1e-4
    rms = float(np.sqrt(np.mean(go * go)))
    flips = np.sign(gg) != np.sign(go)
    assert np.abs(gg - go).max() <= 0.02 * rms
    assert flips.mean() <= 1e-3 and (not flips.any() or np.abs(go[flips]).max() <= 0.02 * rms)


@pytest.fixture(scope="module")
def full_iv():
    return synthetic_ivector_system(C=2048, D=72, R=400, L=200, n_speakers=2)


def test_config2_unfused_chain_at_full_size(oracle, full_iv):
    """configs[2] (i-vector-PLDA SV, C = 2048, spd = 50, 3 s, mfcc_f32 = 1) with the unfused chain: k_mfcc_f32 in two
    rounds, against the oracle twin at test_gpu_fullsize_ivector.py's bounds."""
    sv = full_iv.with_enrolled(full_iv.enrolled[:1], [-40.0], [10.0])
    ctx = oracle.IvSystemCtx(oracle.default_cfg(mfcc_f32=1), sv, nthreads=NTHR)
    audio = synthetic_audio(7, 48000)
    kw = dict(samples_per_draw=50, threshold=1.0)
    e = Engine(0)
    try:
        e.set_frontend(mfcc_f32=1)
        e.load_ivector(sv, "SV")
        e.set_fused_chain(False)
        pg = nes_params("SV", "targeted", seed=42, stream=3, **kw)
        flg, gg, alg, scg = e.get_grad(pg, audio, it=4)
        sh = e.debug_launch_shape()
        assert sh["cus"] == 128 and sh["rounds"] == 2, sh
    finally:
        e.close()
    po = oracle.nes_params("SV", "targeted", ctx.S, **kw)
    flo, go, alo, sco = oracle.get_grad(po, ctx.fn, ctx.ctx, audio, seed=42, it=4, stream=3)
    tol = 1e-4
    assert abs(alg - alo) <= tol and abs(flg - flo) <= tol
    assert np.abs(scg[:1] - sco).max() <= tol
    assert np.abs(gg - go).max() <= tol * 6.0 / pg.sigma
    big = np.abs(go) > 10 * tol / pg.sigma
    assert np.all(np.sign(gg[big]) == np.sign(go[big]))


# ------------------------------------------------------------------------------------------------------------- gselect
def test_gselect_at_every_selection_chunk_count(full_iv):
    """The wide form (FB_GSEL_TARGET_BLOCKS) and the general form (FB_GSEL_NARROW=1, FB_GMM_TARGET_BLOCKS) of the threshold
    selection at 1, 2, 4 and 8 selection chunks: slot for slot the dump path's selection, bit-identical i-vectors."""
    wavs = [_wav(0, 48000), _wav(1, 31000), _wav(2, 11200)]
    e = Engine(0)
    seen = set()
    try:
        e.load_ivector(full_iv, "OSI")
        os.environ["FB_IV_GSEL_DUMP"] = "1"
        try:
            e.score_raw(wavs)
        finally:
            os.environ.pop("FB_IV_GSEL_DUMP")
        sel_d, info_d = e.debug_iv_gselect()
        ivs_d = e.debug_ivectors(len(wavs), full_iv.R)
        assert info_d["path"] == 0 and e.debug_launch_shape()["gmm"] == "fx2"
        frames = sum(e._num_frames(w.size) for w in wavs)   # (both forms size their chunks from the batch's frames)
        for form, knob, strip in (("wide", "FB_GSEL_TARGET_BLOCKS", 256), ("general", "FB_GMM_TARGET_BLOCKS", 128)):
            for n in (1, 2, 4, 8):
                os.environ[knob] = str(-(-frames // strip) * n)
                if form == "general":
                    os.environ["FB_GSEL_NARROW"] = "1"
                try:
                    e.score_raw(wavs)
                finally:
                    os.environ.pop(knob)
                    os.environ.pop("FB_GSEL_NARROW", None)
                sel, info = e.debug_iv_gselect()
                ivs = e.debug_ivectors(len(wavs), full_iv.R)
                sh = e.debug_launch_shape()
                assert info["path"] == (2 if form == "wide" else 1) and info["overflow"] == 0, (form, n, info)
                assert info["chunks"] == n, (form, n, info)
                if form == "general":         # the gated dump behind the general form: the chunk count the selection derives from
                    assert sh["gmm"] == "fx2" and sh["n_chunks"] == n and sh["xcd_map"] == n, sh
                else:
                    assert sh["gmm"] is None, sh
                seen.add((form, info["chunks"]))
                assert np.array_equal(sel, sel_d), (form, n)
                assert np.array_equal(ivs.view(np.uint64), ivs_d.view(np.uint64)), (form, n)
    finally:
        e.close()
    assert seen == {(f, n) for f in ("wide", "general") for n in (1, 2, 4, 8)}
