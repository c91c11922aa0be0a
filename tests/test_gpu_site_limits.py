"""Sites at the engine's limits: 60 diagonal GMMs (fb_load_gmm refuses M > 60), 60 enrolled i-vector speakers
(fb_load_ivector refuses S > 60), 59 / 60 scores in the NES result block -- where the rest of the suite stops at 29 models
and 10 enrolled speakers.

1. k_gmm_fx2 (every single-group site above 28 models, every site with several variance groups) and k_gmm_bx3 at 30, 45
   and 60 models.  Both keep a [M][256] float pair of logsumexp state in dynamic LDS: 4 KB * NKF + 2 KB * M for fx2
   (143 360 bytes at D = 72, M = 60), 6 KB * NK + 2 KB * M for bx3 (153 600 bytes at D = 72, 159 744 at D = 78 .. 80) -- the
   largest launch of the suite before this file asked for 79 872.  Per-frame values against the float64 formula of
   tests/test_gpu_configs.py, utterance scores against the oracle, every model's column independent of its position.
2. The NES step behind a 60-model site, at the batch sizes where fb_gmm_finalize_loss_body changes its exchange protocol
   (B M against 512 / 1024) and fb_loss_body moves the scores from LDS to memory (B S against 768 / 2048), and at the largest
   batch whose update rides in the finalising launch: the launch chains bit for bit against one another and against their
   Philox replay, iteration 0 against the oracle.
3. i-vector sites with 11, 33 and 60 enrolled speakers: k_iv_backend's speaker loop, the solve kernels' tail with the scores
   in LDS (B S = 1980) and in memory (2100; 7740, the largest batch it takes), k_loss<false> at B S = 7860, k_loss_eot at
   S = 60.
4. The limits themselves.
Every case asserts the kernel or the launches it ran and prints its measured maximum errors."""
import os

import numpy as np
import pytest

from fakebob_amd import input_transform as T
from fakebob_amd._native import FB_E_ARG, NativeError
from fakebob_amd.engine import Engine, nes_params
from fakebob_amd.models import (DiagGmm, stack_models, synthetic_audio, synthetic_gmm_system, synthetic_ivector_system,
                                synthetic_ubm_moments)
from tests import nes_edges_ref as R
from tests.input_transform_noise_ref import NOISE, eot_mean, ref_noisy
from tests.test_gpu_configs import _frame_lls
from tests.test_gpu_input_transform import SCORE_TOL   # the bound between an NES batch's row and a scoring call

pytestmark = pytest.mark.gpu
GMM_TOL = 2e-5              # utterance scores, losses and NES rows of a GMM site against the oracle (tests/test_gpu_configs.py)
FUSION_ENV = ("FB_NO_FUSE", "FB_FUSE_UPD", "FB_FUSE_PARTS", "FB_FIN_COUNTER", "FB_FIN_TICKET", "FB_ATTACK_BATCH", "FB_VAD_WHOLE")
LENGTHS = (8000, 10777, 13554, 16000)   # 0.5 .. 1 s, ragged


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    """No kernel, fusion or i-vector knob of the caller's environment reaches a case."""
    for k in list(os.environ):
        if k.startswith(("FB_GMM_", "FB_IV_", "FB_GSEL_")) or k in FUSION_ENV:
            monkeypatch.delenv(k)
    return monkeypatch


def _wav(utt, n):
    return (synthetic_audio(utt, n) * 32768.0).astype(np.int16)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def _launches(eng):
    """fb_debug_nes_route of the last call, the kinds that ran only: {kind: launches}."""
    return {k: v for k, v in eng.debug_nes_route().items() if v}


def _assert_same_attack(a, b, what):
    """(int16 adv, flag, float64 adv, trace) twice: the same bits."""
    assert a[1] == b[1], what
    assert np.array_equal(a[0], b[0]), what
    assert np.array_equal(_bits(a[2]), _bits(b[2])), what
    assert a[3].shape == b[3].shape and np.array_equal(_bits(a[3]), _bits(b[3])), what


# ------------------------------------------------------------------ 1. the scoring kernels at 30, 45 and 60 models
KERNEL_ENV = {"fx2": {}, "bx3": {"FB_GMM_MODE": "bx3"}}


def _rows(ubm, n=300, seed=7):
    """n feature rows drawn from the UBM's components: two 128-frame strips and a ragged one of 44."""
    rng = np.random.default_rng(seed)
    var = 1.0 / ubm.inv_vars.astype(np.float64)
    mu = ubm.means_invvars.astype(np.float64) * var
    ks = rng.integers(0, var.shape[0], n)
    return (mu[ks] + np.sqrt(var[ks]) * rng.standard_normal((n, var.shape[1]))).astype(np.float32)


def _site(oracle, models, **fe):
    """A site with everything the float64 side says about it, computed once: per-frame values of 300 rows and the oracle's
    scores of four ragged utterances.  Every model's column stands for itself, so a site of the first M models reads the
    first M columns."""
    wavs = [_wav(u, n) for u, n in enumerate(LENGTHS)]
    rows = _rows(models[0])
    gc, miv, iv = stack_models(models)
    raw_o, tv_o = oracle.gmm_score_batch(oracle.default_cfg(**fe), wavs, gc, miv, iv, nthreads=8)
    return dict(models=models, fe=fe, wavs=wavs, rows=rows, want=_frame_lls(models, rows), raw_o=raw_o, tv_o=tv_o)


def _score_site(env, site, order, kernel):
    """The models site["models"][i] for i in `order` on a fresh engine: (per-frame values, raw scores, voiced counts), the
    kernel asserted from what fb_load_gmm chose and from what the two launches recorded."""
    e = Engine(0)
    try:
        for k, v in KERNEL_ENV[kernel].items():
            env.setenv(k, v)
        if site["fe"]:
            e.set_frontend(**site["fe"])
        e.load_gmm([site["models"][i] for i in order])
        assert e.gmm_kernel == kernel and e.gmm_kernel_variant == kernel, (e.gmm_kernel, e.gmm_kernel_variant)
        frames = e.debug_gmm_frames(site["rows"])
        sh = e.debug_launch_shape()
        assert sh["gmm"] == kernel and sh["strips"] == 3 and sh["passes"] == 1, sh
        raw, tv = e.score_raw(site["wavs"])
        sh = e.debug_launch_shape()
        assert sh["gmm"] == kernel and sh["passes"] == 1, sh
    finally:
        e.close()
        for k in KERNEL_ENV[kernel]:
            env.delenv(k, raising=False)
    return frames, raw, tv


def _check_site(env, site, M, kernel, label):
    """One kernel on the first M models of a site, against the float64 side and against itself with the models loaded in
    reversed order -> {figure: maximum error}."""
    order = list(range(M))
    frames, raw, tv = _score_site(env, site, order, kernel)
    want, raw_o = site["want"][:M], site["raw_o"][:, :M]
    assert frames.shape == want.shape and np.isfinite(frames).all() and np.isfinite(raw).all()
    rel = np.abs(frames - want) / np.maximum(1.0, np.abs(want))
    err = dict(frame=float(np.abs(frames - want).max()), frame_rel=float(rel.max()), score=float(np.abs(raw - raw_o).max()),
               score_sys=float(np.abs((raw[:, 1:] - raw[:, :1]) - (raw_o[:, 1:] - raw_o[:, :1])).max()))
    print("%s, %d models on k_gmm_%s: per frame |err| %.3g (relative %.3g), scores %.3g, scores minus model 0's %.3g"
          % (label, M, kernel, err["frame"], err["frame_rel"], err["score"], err["score_sys"]))
    # per frame: the bounds tests/test_gpu_configs.py and tests/test_gpu_launch_shapes.py hold these two kernels to
    assert rel[0].max() <= 2e-6 and rel.max() <= 2e-6, (label, M, kernel, rel.max())
    assert np.abs((frames[1:] - frames[:1]) - (want[1:] - want[:1])).max() <= 2e-3
    assert np.array_equal(tv, site["tv_o"])
    assert err["score"] <= GMM_TOL, (label, M, kernel, err)
    # a column belongs to its model and to nothing else: no two alike ...
    for u in range(raw.shape[0]):
        assert len(set(raw[u].tolist())) == M, (label, M, kernel, u)
    assert len({frames[m].tobytes() for m in range(M)}) == M
    # ... and the same bits wherever the model stands in the list: a model's item continues from the quadratic item of
    # its variance group and updates LDS state of its own; the load-time scalings are maxima over all models
    frames_r, raw_r, tv_r = _score_site(env, site, order[::-1], kernel)
    assert np.array_equal(tv_r, tv)
    assert np.array_equal(_bits(frames_r[::-1]), _bits(frames)), (label, M, kernel)
    assert np.array_equal(_bits(raw_r[:, ::-1]), _bits(raw)), (label, M, kernel)
    return err


@pytest.fixture(scope="module")
def site60(oracle):
    """UBM + 59 speakers that share its variances (one group: 1 + M items), C = 256, D = 72."""
    ubm, spk = synthetic_gmm_system(n_speakers=59, C=256, D=72, enrol_frames=2000.0)
    return _site(oracle, [ubm] + spk)


@pytest.mark.parametrize("M", [30, 45, 60])
def test_scoring_kernels_at_30_45_and_60_models(site60, clean_env, M):
    """k_gmm_fx2 asks for 20 480 + 2 048 M bytes of LDS at D = 72 (NKF = 5): 81 920, 112 640 and 143 360; k_gmm_bx3 for
    30 720 + 2 048 M (NK = 5): 92 160, 122 880 and 153 600.  The state of model m is [m][256] floats behind the two image
    slots: a wrong stride, or a launch that does not get its LDS, shows in the last models' columns first."""
    err = {k: _check_site(clean_env, site60, M, k, "one variance group") for k in ("fx2", "bx3")}
    # tests/test_gpu_parity.py's yardstick: the two-term f16 split gives up nothing against the exact bf16 one
    for fig in ("frame", "score", "score_sys"):
        assert err["fx2"][fig] <= 2.0 * err["bx3"][fig] + 2e-6, (fig, err)


def _scaled_variances(spk, w, factors):
    """Speaker i with its variances divided by factors[i % len(factors)] (the means kept): models with the same factor
    keep bitwise identical inv_vars and share a quadratic item."""
    out = []
    for i, m in enumerate(spk):
        f = np.float32(factors[i % len(factors)])
        out.append(m if f == 1.0 else DiagGmm.from_internal(w, m.means_invvars * f, m.inv_vars * f))
    return out


@pytest.mark.parametrize("groups", ["three", "one per model"])
def test_general_kernel_with_several_variance_groups_at_60_models(oracle, clean_env, groups):
    """Three groups interleaved over the speakers (63 items a tile: Q, 20 models, Q, 20 models, Q, 20 models, the models
    not in list order) and every model with variances of its own (120 items: Q, model, Q, model, ...).  The state row a
    model item updates comes from item_model[], not from the item's place."""
    ubm, spk = synthetic_gmm_system(n_speakers=59, C=256, D=72, enrol_frames=2000.0)
    w, _mu, _var = synthetic_ubm_moments(256, 72, 2001)
    factors = (1.0, 1.25, 0.8) if groups == "three" else [1.0 + 0.01 * (i + 1) for i in range(59)]
    models = [ubm] + _scaled_variances(spk, w, factors)
    n_groups = len({m.inv_vars.tobytes() for m in models})
    assert n_groups == (3 if groups == "three" else 60)
    _check_site(clean_env, _site(oracle, models), 60, "fx2", "%d variance groups" % n_groups)


def test_bf16_kernel_at_its_largest_lds_request(oracle, clean_env):
    """26 cepstra: D = 78, NK = 6 -- 36 864 bytes of image slots and 122 880 of state, 159 744 of the CU's 163 840."""
    fe = dict(num_ceps=26)
    ubm, spk = synthetic_gmm_system(n_speakers=59, C=256, D=78, enrol_frames=2000.0)
    _check_site(clean_env, _site(oracle, [ubm] + spk, **fe), 60, "bx3", "D = 78")


# ------------------------------------------------------------------ 2. the NES step behind a 60-model site
FUSE_MAX_HALF = 40                       # fb_kernels.h: FB_FUSE_MAX_HALF
FUSE_MAX_UPD_WG = 192                    # fb_kernels.h: FB_FUSE_MAX_UPD_WG
SMALL_MAX_SPD = 128                      # gmm_kernels.hip, nes_kernels.hip: the SMALL instantiations take B - 1 <= 128
XCH_MAX = {True: 512, False: 1024}       # k_gmm_finalize_loss_update: n_fin <= (SMALL ? 512 : 1024) ? u.xch : nullptr
FIN_SC_CAP = {True: 768, False: 2048}    # fb_gmm_finalize_loss_body: SC_CAP = SMALL ? 768 : FB_SC_LDS
SC_LDS = 2048                            # fb_nes_device.h: FB_SC_LDS (k_loss, the solve kernels' tail)


def _gmm_branches(spd, M, S, n):
    """What the source's constants say about a GMM site's NES batch: the instantiation, whether the update rides in the
    finalising launch (fb_engine.hip: fuses_update, attack_loop), whether that launch hands the scores over through its
    exchange slots (otherwise the arrival counter -- as k_gmm_finalize_loss always does), and whether fb_loss_body keeps the
    B S scores in LDS while it forms the losses."""
    half = spd // 2
    B = 2 * half + 1
    small = B - 1 <= SMALL_MAX_SPD
    rides = 0 < half <= FUSE_MAX_HALF and (n + 255) // 256 <= FUSE_MAX_UPD_WG
    return dict(B=B, BM=B * M, BS=B * S, small=small, rides=rides, slots=rides and B * M <= XCH_MAX[small],
                lds=B * S <= FIN_SC_CAP[small], lds_k_loss=B * S <= SC_LDS)


# (task, samples_per_draw) -> B M, B S, exchange slots, scores in LDS in the finalising launch, ... and in k_loss
NES_GMM = {
    ("OSI", 6): (420, 413, True, True, True),        # exchange slots, scores in LDS
    ("CSI", 6): (420, 420, True, True, True),
    ("OSI", 8): (540, 531, False, True, True),       # B M > 512: the arrival counter
    ("CSI", 8): (540, 540, False, True, True),
    ("OSI", 12): (780, 767, False, True, True),      # the last size with the scores in LDS (<= 768) ...
    ("CSI", 12): (780, 780, False, False, True),     # ... and the first in memory -- where k_loss still holds them in LDS
    ("OSI", 14): (900, 885, False, False, True),
    ("CSI", 14): (900, 900, False, False, True),
    ("OSI", 80): (4860, 4779, False, False, False),  # half = FB_FUSE_MAX_HALF: the largest batch whose update rides along
    ("CSI", 80): (4860, 4860, False, False, False),  # (B = 81: the loss body's rows in two waves, 4 860 arrivals)
    ("OSI", 130): (7860, 7729, False, False, False),  # not SMALL: no update in the finalising launch, counter, memory
    ("CSI", 130): (7860, 7860, False, False, False),
}
CHAINS = {"fused": (True, {}), "FB_FUSE_UPD=0": (True, {"FB_FUSE_UPD": "0"}), "FB_FIN_COUNTER=1": (True, {"FB_FIN_COUNTER": "1"}),
          "shared": (False, {}), "FB_NO_FUSE=1": (None, {"FB_NO_FUSE": "1"})}


def _gmm_routes(rides):
    """The launches of each chain per NES iteration (tests/test_gpu_nes_edges.py section d; fb_engine.hip: loop_knobs).  From
    half = 41 on the update is k_grad_update on the staged normals everywhere and FB_FUSE_UPD / FB_FIN_COUNTER have nothing
    to act on: the fused chain then runs k_gmm_finalize_loss."""
    if rides:
        return {"fused": ("fin_loss_update",), "FB_FUSE_UPD=0": ("fin_loss", "k_update_perturb"), "FB_FIN_COUNTER=1": ("fin_loss_update",),
                "shared": ("k_loss", "k_update_perturb"), "FB_NO_FUSE=1": ("k_loss", "k_grad_update")}
    return {"fused": ("fin_loss", "k_grad_update"), "shared": ("k_loss", "k_grad_update"), "FB_NO_FUSE=1": ("k_loss", "k_grad_update")}


@pytest.fixture(scope="module")
def nes_site():
    """UBM + 60 speakers, C = 128: OSI loads the UBM and the first 59 (S = 59), CSI the 60 speakers (S = 60)."""
    ubm, spk = synthetic_gmm_system(n_speakers=60, C=128, D=72, enrol_frames=2000.0)
    return ubm, spk


@pytest.mark.parametrize("task,spd", sorted(NES_GMM))
def test_nes_step_behind_a_60_model_site(oracle, nes_site, clean_env, task, spd):
    """An attack of four iterations (three at samples_per_draw = 130) on every launch chain the batch size has: the same
    bits, and the bits of the replay on the device's own normals.  At samples_per_draw = 12 and 14 -- B S on both sides of
    768 -- iteration 0 against the oracle, with a target above 31.  The two capacities guard LDS arrays of the loss body;
    a batch of up to 64 rows sits in one wave, which has read everything before it writes anything an overrun could reach
    (DESIGN.md section 4), so the cases that see a wrong capacity are the ones with two waves of rows: 80 and 130."""
    n, iters = 9000, (3 if spd == 130 else 4)
    ubm, spk = nes_site
    models = [ubm] + spk[:59] if task == "OSI" else spk
    zm, zs = np.linspace(-112.0, -96.0, 60), np.linspace(1.0, 3.0, 60)
    M, S = 60, (59 if task == "OSI" else 60)
    br = _gmm_branches(spd, M, S, n)
    assert (br["BM"], br["BS"], br["slots"], br["lds"], br["lds_k_loss"]) == NES_GMM[(task, spd)], br
    assert br["small"] == (spd != 130) and br["rides"] == (spd != 130)
    half = spd // 2
    audio = synthetic_audio(6, n)
    e = Engine(0)
    try:
        e.load_gmm(models)
        if task == "CSI":
            e.set_system("CSI", zm, zs)
        else:
            e.set_system("OSI")
        assert e.gmm_kernel_variant == "fx2" and e.n_speakers == S
        sc = e.system_scores(e.score_raw([(audio * 32768.0).astype(np.int16)])[0])[0]
        tgt = 32 + int(np.argmax(sc[32:]))
        # (the loss stays positive: the attack runs its iterations)
        kw = dict(samples_per_draw=spd, max_iter=iters, target=tgt)
        kw.update(dict(threshold=float(sc.max()) + 50.0) if task == "OSI" else dict(adver_thresh=1.0e3))
        p = nes_params(task, "targeted", seed=5, stream=0, **kw)
        routes = _gmm_routes(br["rides"])
        got = {}
        for name, kinds in routes.items():
            fused, env = CHAINS[name]
            for k, v in env.items():
                clean_env.setenv(k, v)
            e.set_fused_chain(fused)
            got[name] = e.attack(p, audio)
            assert _launches(e) == {k: iters for k in kinds}, (name, _launches(e))
            chain = e.debug_frontend_route()["chain"]
            assert (chain in ("split", "whole")) == (name != "FB_NO_FUSE=1"), (name, chain)
            for k in env:
                clean_env.delenv(k, raising=False)
        e.set_fused_chain(True)
        rep = e.attack(p, audio, noise_all=R.replay_noise(e, 5, 0, n, half, iters, oracle=oracle))
        assert _launches(e) == dict(fin_loss=iters, k_grad_update=iters)
        grad0 = e.get_grad(p, audio, it=0)
        assert _launches(e) == dict(k_loss=1, k_grad_update=1)
    finally:
        e.close()
    ref = got["fused"]
    assert ref[3].shape == (iters, 3 + S) and ref[1] == -1 and np.isfinite(ref[3]).all()
    assert np.any(ref[0] != (audio * 32768.0).astype(np.int16))
    for name, other in got.items():
        _assert_same_attack(ref, other, (task, spd, name))
    _assert_same_attack(ref, rep, (task, spd, "replay"))
    # get_grad's score0 holds all S scores: the ones of the attack's first row, and a scoring call's to SCORE_TOL
    flg, _gg, alg, scg = grad0
    row0 = ref[3][0]                                                   # [distance, adver_loss, lr, scores]
    assert scg.shape == (S,) and np.array_equal(_bits(scg), _bits(row0[3:])) and alg == row0[1]
    assert len(set(scg.tolist())) == S
    d_call = float(np.abs(scg - sc).max())
    line = "%s samples_per_draw %d (B M %d, B S %d): %s; row 0 against a scoring call %.3g" % (
        task, spd, br["BM"], br["BS"], ", ".join("%s = %s" % (k, "+".join(v)) for k, v in routes.items()), d_call)
    assert d_call <= SCORE_TOL
    if spd in (12, 14):
        gc, miv, iv = stack_models(models)
        ctx = oracle.GmmSystemCtx(oracle.default_cfg(), task, gc, miv, iv, z_mean=zm if task == "CSI" else None,
                                  z_std=zs if task == "CSI" else None, nthreads=8)
        assert ctx.S == S
        po = oracle.nes_params(task, "targeted", ctx.S, **kw)
        flo, _go, alo, sco = oracle.get_grad(po, ctx.fn, ctx.ctx, audio, seed=5, it=0, stream=0)
        d = (float(np.abs(row0[3:] - sco).max()), abs(row0[1] - alo), abs(flg - flo))
        line += "; against the oracle: scores %.3g adver_loss %.3g final_loss %.3g (target %d)" % (d + (tgt,))
        print(line)
        assert sco.shape == (S,) and max(d) <= GMM_TOL, d
    else:
        print(line)


# ------------------------------------------------------------------ 3. i-vector sites with 11, 33 and 60 speakers
@pytest.fixture(scope="module")
def iv60():
    sy = synthetic_ivector_system(C=96, D=72, R=48, L=24, n_speakers=60, seed=23)
    return sy.with_enrolled(sy.enrolled, z_mean=np.linspace(-40.0, -20.0, 60), z_std=np.linspace(4.0, 9.0, 60))


@pytest.fixture(scope="module")
def iv60_ctx(oracle, iv60):
    return oracle.IvSystemCtx(oracle.default_cfg(), iv60, nthreads=8)


def _first(iv60, S, reverse=False):
    idx = np.arange(S)[::-1] if reverse else np.arange(S)
    return iv60.with_enrolled(iv60.enrolled[idx], iv60.z_mean[idx], iv60.z_std[idx])


@pytest.mark.parametrize("S", [11, 33, 60])
def test_ivector_scoring_with_11_33_and_60_speakers(engine, oracle, iv60, iv60_ctx, S):
    """k_iv_backend's loop over the enrolled speakers: PLDA log-likelihood ratios of four ragged utterances and z-normed
    system scores against the oracle; no two columns alike; the speakers enrolled in reversed order give the reversed
    columns, bit for bit (the loop treats every speaker on its own)."""
    sy = _first(iv60, S)
    ctx = oracle.IvSystemCtx(oracle.default_cfg(), sy, nthreads=8, share=iv60_ctx)
    wavs = [_wav(u, n) for u, n in enumerate(LENGTHS)]
    engine.load_ivector(sy, "OSI")
    assert engine.n_speakers == S
    llr, tv = engine.score_raw(wavs)
    sc = engine.system_scores(llr)
    engine.load_ivector(_first(iv60, S, reverse=True), "OSI")
    llr_r, tv_r = engine.score_raw(wavs)
    sc_r = engine.system_scores(llr_r)
    llr_o, _ivs, tv_o = ctx.score_batch(wavs)
    audio = synthetic_audio(3, LENGTHS[3])
    sc_o = ctx.score(audio[:, None])[0]
    d_llr, d_sc = float(np.abs(llr - llr_o).max()), float(np.abs(sc[3] - sc_o).max())
    print("i-vector site with %d speakers (k_iv_backend): PLDA ratios %.3g, z-normed scores %.3g" % (S, d_llr, d_sc))
    assert llr.shape == (4, S) and np.array_equal(tv, tv_o) and np.array_equal(tv_r, tv)
    assert d_llr <= SCORE_TOL and d_sc <= SCORE_TOL
    assert np.allclose(sc, (llr - sy.z_mean) / sy.z_std, rtol=0, atol=1e-12)
    for u in range(4):
        assert len(set(llr[u].tolist())) == S and len(set(sc[u].tolist())) == S
    assert np.array_equal(_bits(llr_r[:, ::-1]), _bits(llr)) and np.array_equal(_bits(sc_r[:, ::-1]), _bits(sc))


IV_KINDS = {"OSI": ("targeted", dict(target=47)), "CSI": ("untargeted", dict(true=59, adver_thresh=1.0e3))}


def _iv_params(task, spd, s0, iters):
    kind, kw = IV_KINDS[task]
    kw = dict(kw, samples_per_draw=spd, max_iter=iters)
    if task == "OSI":
        kw["threshold"] = float(s0.max()) + 50.0
    return kind, kw


@pytest.mark.parametrize("task", ["OSI", "CSI"])
@pytest.mark.parametrize("spd", [32, 34, 128])
def test_ivector_tail_loss_with_60_speakers(oracle, iv60, iv60_ctx, clean_env, task, spd):
    """The solve kernels' tail runs fb_loss_body<true, true> with FB_SC_LDS = 2048 scores of LDS: B S = 33 x 60 = 1980 in
    LDS, 35 x 60 = 2100 in memory, and 129 x 60 = 7740 at samples_per_draw = 128, the largest batch the tail takes
    (fb_iv_tail_takes_loss: B - 1 <= 128).  As tests/test_gpu_nes_edges.py section e at S = 2: the fused chain, every launch on
    its own and the separate back-end and k_loss launches are the same bits and equal their Philox replay -- with half = 16
    / 17 <= FB_FUSE_MAX_HALF the update is k_update_perturb wherever the chain fuses it, with half = 64 k_grad_update on the
    staged normals everywhere.  Iteration 0 against the oracle."""
    n, half, iters = 8000, spd // 2, 3
    assert ((2 * half + 1) * 60 <= SC_LDS) == (spd == 32) and spd <= SMALL_MAX_SPD
    audio = synthetic_audio(6, n)
    e = Engine(0)
    try:
        e.load_ivector(iv60, task)
        s0 = e.system_scores(e.score_raw([(audio * 32768.0).astype(np.int16)])[0])[0]
        kind, kw = _iv_params(task, spd, s0, iters)
        p = nes_params(task, kind, seed=7, stream=1, **kw)
        got, seen = {}, {}
        for name, fused, env in (("fused", True, {}), ("FB_NO_FUSE=1", None, {"FB_NO_FUSE": "1"}),
                                 ("FB_IV_TAIL=split", True, {"FB_IV_TAIL": "split"})):
            for k, v in env.items():
                clean_env.setenv(k, v)
            e.set_fused_chain(fused)
            got[name] = e.attack(p, audio)
            seen[name] = _launches(e)
            want = {"k_loss" if name == "FB_IV_TAIL=split" else "iv_tail": iters,
                    "k_grad_update" if name == "FB_NO_FUSE=1" or half > FUSE_MAX_HALF else "k_update_perturb": iters}
            assert seen[name] == want, (name, seen[name])
            for k in env:
                clean_env.delenv(k, raising=False)
        e.set_fused_chain(True)
        rep = e.attack(p, audio, noise_all=R.replay_noise(e, 7, 1, n, half, iters, oracle=oracle))
        assert _launches(e) == dict(iv_tail=iters, k_grad_update=iters)
        flg, gg, alg, scg = e.get_grad(p, audio, it=0)
    finally:
        e.close()
    ref = got["fused"]
    assert ref[3].shape == (iters, 3 + 60) and ref[1] == -1 and np.isfinite(ref[3]).all()
    assert np.any(ref[0] != (audio * 32768.0).astype(np.int16))
    for name, other in got.items():
        _assert_same_attack(ref, other, (task, spd, name))
    _assert_same_attack(ref, rep, (task, spd, "replay"))
    assert scg.shape == (60,) and np.array_equal(_bits(scg), _bits(ref[3][0][3:])) and alg == ref[3][0][1]
    ctx = oracle.IvSystemCtx(oracle.default_cfg(), iv60, nthreads=8, share=iv60_ctx)
    po = oracle.nes_params(task, kind, ctx.S, **kw)
    flo, go, alo, sco = oracle.get_grad(po, ctx.fn, ctx.ctx, audio, seed=7, it=0, stream=1)
    d = (float(np.abs(scg - sco).max()), abs(alg - alo), abs(flg - flo), float(np.abs(gg - go).max()))
    print("i-vector %s, 60 speakers, samples_per_draw %d (B S %d): %s; against the oracle: scores %.3g adver_loss %.3g "
          "final_loss %.3g gradient %.3g (bound %.3g)" % (task, spd, (2 * half + 1) * 60, seen, d[0], d[1], d[2], d[3],
                                                          SCORE_TOL * 6.0 / p.sigma))
    assert max(d[:3]) <= SCORE_TOL, d
    assert d[3] <= SCORE_TOL * 6.0 / p.sigma, d


def test_ivector_loss_with_60_speakers_in_k_loss(iv60, clean_env):
    """samples_per_draw = 130: the tail hands the loss back to k_loss<false>, B S = 131 x 60 = 7860 scores in memory."""
    n, spd, iters = 8000, 130, 3
    audio = synthetic_audio(6, n)
    e = Engine(0)
    try:
        e.load_ivector(iv60, "OSI")
        s0 = e.system_scores(e.score_raw([(audio * 32768.0).astype(np.int16)])[0])[0]
        kind, kw = _iv_params("OSI", spd, s0, iters)
        p = nes_params("OSI", kind, seed=7, stream=1, **kw)
        got = {}
        for name, fused, env in (("fused", True, {}), ("FB_NO_FUSE=1", None, {"FB_NO_FUSE": "1"})):
            for k, v in env.items():
                clean_env.setenv(k, v)
            e.set_fused_chain(fused)
            got[name] = e.attack(p, audio)
            assert _launches(e) == dict(k_loss=iters, k_grad_update=iters), (name, _launches(e))
            for k in env:
                clean_env.delenv(k, raising=False)
        e.set_fused_chain(True)
        rep = e.attack(p, audio, noise_all=R.replay_noise(e, 7, 1, n, spd // 2, iters))
        assert _launches(e) == dict(k_loss=iters, k_grad_update=iters)
    finally:
        e.close()
    ref = got["fused"]
    assert ref[3].shape == (iters, 3 + 60) and ref[1] == -1 and np.isfinite(ref[3]).all()
    d_call = float(np.abs(ref[3][0][3:] - s0).max())
    print("i-vector OSI, 60 speakers, samples_per_draw 130 (B S 7860): k_loss + k_grad_update; row 0 against a scoring "
          "call %.3g" % d_call)
    assert d_call <= SCORE_TOL and len(set(ref[3][0][3:].tolist())) == 60
    _assert_same_attack(ref, got["FB_NO_FUSE=1"], "FB_NO_FUSE=1")
    _assert_same_attack(ref, rep, "replay")


def test_ivector_eot_loss_with_60_speakers(iv60):
    """fb_set_eot(2) at samples_per_draw = 34: k_loss_eot averages 2 x 35 rows of 60 scores.  As
    tests/test_gpu_eot.py's test_get_grad_averages_over_the_replicas: score0 and adver_loss against the numpy mean (the
    contract's order) of per-replica system scores and losses from scoring the restatement's replicas on a chain-less
    engine, at that file's bound."""
    r, it, seed, stream, n, tgt = 2, 4, 11, 6, 8000, 47
    chain = T.parse("at:20")
    audio = synthetic_audio(9, n)
    d, c = Engine(0), Engine(0)
    try:
        d.load_ivector(iv60, "OSI")
        c.load_ivector(iv60, "OSI")
        d.set_input_transform(chain)
        d.set_eot(r)
        thr, adv_thr = 0.1, 0.05
        p = nes_params("OSI", "targeted", samples_per_draw=34, threshold=thr, adver_thresh=adv_thr, seed=seed, stream=stream, target=tgt)
        fl, _g, al, sc0 = d.get_grad(p, audio, it=it)
        assert _launches(d) == dict(k_loss=1, k_grad_update=1)          # (k_loss_eot is counted as the k_loss launch)
        w = (np.asarray(audio, np.float64) * 32768.0).astype(np.int64).astype(np.int16)
        reps = []
        for j in range(r):
            normals = {s: d.debug_tf_noise(seed, stream, it, 0, j, s, 0, w.size) for s, st in enumerate(chain) if st.kind == NOISE}
            reps.append(ref_noisy(w, chain, normals))
        sc = c.system_scores(c.score_raw(reps)[0])
    finally:
        d.close()
        c.close()
    others = np.delete(sc, tgt, axis=1).max(axis=1)
    losses = (np.maximum(others, thr) + adv_thr) - sc[:, tgt]
    want_sc, want_al = eot_mean(sc.T), float(eot_mean(losses))
    print("i-vector OSI, 60 speakers, 2 replicas (k_loss_eot): score0 %.3g adver_loss %.3g"
          % (np.abs(sc0 - want_sc).max(), abs(al - want_al)))
    assert sc0.shape == (60,) and want_sc.shape == (60,)
    assert np.abs(sc0 - want_sc).max() <= 2 * SCORE_TOL
    assert abs(al - want_al) <= 2 * SCORE_TOL
    assert np.isfinite(fl)
    assert np.ptp(losses) > 10 * SCORE_TOL                          # the replicas do differ: the mean is not a formality


# ------------------------------------------------------------------ 4. the limits themselves
def test_61_models_are_refused_and_the_60_stay_loaded(nes_site):
    """fb_load_gmm takes 60 models and refuses 61 before it touches anything (include/fakebob_hip.h): the site loaded
    before scores the same bits afterwards, and a later load works."""
    ubm, spk = nes_site
    wavs = [_wav(1, 9000)]
    e = Engine(0)
    try:
        e.load_gmm([ubm] + spk[:59])
        before, tv = e.score_raw(wavs)
        with pytest.raises(NativeError) as ex:
            e.load_gmm([ubm] + spk)
        assert ex.value.code == FB_E_ARG and "at most 60 models per engine (got 61)" in str(ex.value)
        assert e.n_models == 60
        after, tv2 = e.score_raw(wavs)
        assert np.array_equal(_bits(after), _bits(before)) and np.array_equal(tv, tv2)
        e.load_gmm([ubm] + spk[:2])
        small, _ = e.score_raw(wavs)
        assert small.shape == (1, 3) and np.abs(small - before[:, :3]).max() <= GMM_TOL   # (k_gmm_fx2w now)
    finally:
        e.close()


def test_61_enrolled_speakers_are_refused_and_the_60_stay_loaded(iv60):
    wavs = [_wav(1, 9000)]
    extra = np.concatenate([iv60.enrolled, iv60.enrolled[:1] + 1.0])
    sy61 = iv60.with_enrolled(extra, np.append(iv60.z_mean, -30.0), np.append(iv60.z_std, 5.0))
    e = Engine(0)
    try:
        e.load_ivector(iv60, "CSI")
        before, tv = e.score_raw(wavs)
        with pytest.raises(NativeError) as ex:
            e.load_ivector(sy61, "CSI")
        assert ex.value.code == FB_E_ARG and "at most 60 enrolled speakers per engine" in str(ex.value)
        assert e.n_models == 60 and e.n_speakers == 60
        after, tv2 = e.score_raw(wavs)
        assert np.array_equal(_bits(after), _bits(before)) and np.array_equal(tv, tv2)
        e.load_ivector(_first(iv60, 3), "CSI")
        small, _ = e.score_raw(wavs)
        assert small.shape == (1, 3) and np.array_equal(_bits(small), _bits(before[:, :3]))
    finally:
        e.close()
