"""The attack loop on utterances longer than the CMVN window (real test utterances are longer than 3 s): every NES batch
then leaves the fused front end for k_vad -> k_deltas -> k_cmvn -> k_cmvn_sliding, the CompressedMatrix round trip for
the stand-alone k_feat_compress, and the GMM / gselect chunk counts change with the row count.  get_grad and attack
against the oracle, the chain variants bit for bit, route changes on one engine, and the window boundary.  Every case
asserts the route it ran (Engine.debug_frontend_route)."""
import numpy as np
import pytest

from fakebob_amd.engine import Engine, nes_params
from fakebob_amd.models import stack_models, synthetic_audio, synthetic_ivector_system

pytestmark = pytest.mark.gpu
SCORE_TOL = 1e-4
# 301 frames (one past the window), 500 (compression keys in registers), 800 (keys in LDS)
LENGTHS = [48160, 80000, 128000]
FRAMES = {48160: 301, 80000: 500, 128000: 800, 320000: 2000}


def _long_route(r, N, B):
    assert r["chain"] == "separate+sliding" and r["t_max"] == FRAMES[N] and r["B"] == B, r
    assert r["mfcc"] == "k_mfcc_r16<12,true>", r


@pytest.fixture(scope="module")
def small_iv():
    sy = synthetic_ivector_system(C=96, D=72, R=48, L=24, n_speakers=3, seed=11)
    return sy.with_enrolled(sy.enrolled, z_mean=[-30.0, -50.0, -20.0], z_std=[5.0, 8.0, 4.0])


def _gmm_models(small_system, task):
    ubm, spk = small_system
    return {"SV": [ubm, spk[0]], "CSI": spk}.get(task, [ubm] + spk)


def _gmm_ctx(oracle, task, models, cfg=None, zm=None, zs=None):
    gc, miv, iv = stack_models(models)
    return oracle.GmmSystemCtx(cfg or oracle.default_cfg(), task, gc, miv, iv, zm, zs, nthreads=8)


def _check_grad(g, o, sigma):
    flg, gg, alg, scg = g
    flo, go, alo, sco = o
    assert abs(alg - alo) <= SCORE_TOL and abs(flg - flo) <= SCORE_TOL
    assert np.abs(scg[:sco.size] - sco).max() <= SCORE_TOL
    assert np.abs(gg - go).max() <= SCORE_TOL * 6.0 / sigma


GMM_CASES = [("OSI", "targeted", dict(target=1, threshold=0.05)), ("CSI", "untargeted", dict(true=2)),
             ("SV", "targeted", dict(threshold=0.02))]


@pytest.mark.parametrize("N", LENGTHS)
@pytest.mark.parametrize("task,attack,kw", GMM_CASES, ids=[c[0] for c in GMM_CASES])
def test_gmm_get_grad_long(engine, oracle, small_system, N, task, attack, kw):
    models = _gmm_models(small_system, task)
    engine.load_gmm(models)
    zm = np.array([-60.0, -61.0, -59.0]) if task == "CSI" else None
    zs = np.array([2.0, 2.5, 3.0]) if task == "CSI" else None
    engine.set_system(task, zm, zs)
    ctx = _gmm_ctx(oracle, task, models, zm=zm, zs=zs)
    audio = synthetic_audio(4, N)
    pg = nes_params(task, attack, samples_per_draw=6, seed=99, stream=3, **kw)
    po = oracle.nes_params(task, attack, ctx.S, samples_per_draw=6, **kw)
    g = engine.get_grad(pg, audio, it=5)
    _long_route(engine.debug_frontend_route(), N, 7)
    _check_grad(g, oracle.get_grad(po, ctx.fn, ctx.ctx, audio, seed=99, it=5, stream=3), pg.sigma)


def test_gmm_get_grad_2000_frames(engine, oracle, small_system):
    models = _gmm_models(small_system, "OSI")
    engine.load_gmm(models)
    engine.set_system("OSI")
    ctx = _gmm_ctx(oracle, "OSI", models)
    audio = synthetic_audio(8, 320000)
    kw = dict(target=2, threshold=0.05)
    pg = nes_params("OSI", "targeted", samples_per_draw=4, seed=7, stream=1, **kw)
    po = oracle.nes_params("OSI", "targeted", ctx.S, samples_per_draw=4, **kw)
    g = engine.get_grad(pg, audio, it=2)
    _long_route(engine.debug_frontend_route(), 320000, 5)
    _check_grad(g, oracle.get_grad(po, ctx.fn, ctx.ctx, audio, seed=7, it=2, stream=1), pg.sigma)


@pytest.mark.parametrize("N", LENGTHS)
@pytest.mark.parametrize("task,attack,kw", [("OSI", "targeted", dict(target=1, threshold=0.5)),
                                            ("SV", "targeted", dict(threshold=0.1))], ids=["OSI", "SV"])
def test_ivector_get_grad_long(engine, oracle, small_iv, N, task, attack, kw):
    sy = small_iv if task != "SV" else small_iv.with_enrolled(small_iv.enrolled[:1], [-30.0], [5.0])
    engine.load_ivector(sy, task)
    ctx = oracle.IvSystemCtx(oracle.default_cfg(), sy, nthreads=8)
    audio = synthetic_audio(4, N)
    pg = nes_params(task, attack, samples_per_draw=6, seed=3, stream=1, **kw)
    po = oracle.nes_params(task, attack, ctx.S, samples_per_draw=6, **kw)
    g = engine.get_grad(pg, audio, it=2)
    _long_route(engine.debug_frontend_route(), N, 7)
    _check_grad(g, oracle.get_grad(po, ctx.fn, ctx.ctx, audio, seed=3, it=2, stream=1), pg.sigma)


def _attack_pair(e, oracle, ctx, audio, kw, seed=11):
    pg = nes_params("OSI", "targeted", seed=seed, stream=0, **kw)
    po = oracle.nes_params("OSI", "targeted", ctx.S, **kw)
    return e.attack(pg, audio), oracle.attack(po, ctx.fn, ctx.ctx, audio, seed=seed, stream=0)


def _same_trajectory(g, o):
    adv_g, flag_g, advf_g, tr_g = g
    adv_o, flag_o, advf_o, tr_o = o
    assert flag_g == flag_o and tr_g.shape == tr_o.shape
    assert np.abs(tr_g - tr_o).max() <= SCORE_TOL
    # the update is sign(momentum gradient): a flip needs a gradient entry within the 1e-4-scale score error of zero
    assert int(np.sum(adv_g != adv_o)) == 0


def _bits_equal(a, b):
    assert a[1] == b[1] and np.array_equal(a[0], b[0]) and np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])


ATTACK_KW = dict(samples_per_draw=6, max_iter=3, target=0, threshold=-1.0, epsilon=0.002)


def test_gmm_attack_trajectory_long(engine, oracle, small_system):
    models = _gmm_models(small_system, "OSI")
    engine.load_gmm(models)
    engine.set_system("OSI")
    g, o = _attack_pair(engine, oracle, _gmm_ctx(oracle, "OSI", models), synthetic_audio(6, 128000), ATTACK_KW)
    _long_route(engine.debug_frontend_route(), 128000, 7)
    _same_trajectory(g, o)


def test_ivector_attack_trajectory_long(engine, oracle, small_iv):
    engine.load_ivector(small_iv, "OSI")
    ctx = oracle.IvSystemCtx(oracle.default_cfg(), small_iv, nthreads=8)
    kw = dict(ATTACK_KW, threshold=-10.0)
    g, o = _attack_pair(engine, oracle, ctx, synthetic_audio(6, 80000), kw)
    _long_route(engine.debug_frontend_route(), 80000, 7)
    _same_trajectory(g, o)


@pytest.mark.parametrize("N", [48160, 128000])
def test_chain_variants_bit_for_bit_long(oracle, small_system, monkeypatch, N):
    """The NES chain fused (set_fused_chain(True)), split for a shared GPU (False), the library default and every launch
    on its own (FB_NO_FUSE=1): the same attack bit for bit."""
    models = _gmm_models(small_system, "OSI")
    audio = synthetic_audio(6, N)
    p = nes_params("OSI", "targeted", seed=11, stream=0, **ATTACK_KW)
    runs = {}
    for name, fused, env in (("default", None, {}), ("fused", True, {}), ("shared", False, {}), ("none", None, {"FB_NO_FUSE": "1"})):
        monkeypatch.delenv("FB_NO_FUSE", raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        e = Engine(0)
        try:
            e.load_gmm(models)
            e.set_system("OSI")
            e.set_fused_chain(fused)
            runs[name] = e.attack(p, audio)
            _long_route(e.debug_frontend_route(), N, 7)
        finally:
            e.close()
    monkeypatch.delenv("FB_NO_FUSE", raising=False)
    for name in runs:
        _bits_equal(runs[name], runs["default"])


@pytest.mark.parametrize("N,where", [(80000, "registers"), (128000, "lds")])
def test_compress_feats_attack_long(oracle, small_system, N, where):
    models = _gmm_models(small_system, "OSI")
    e = Engine(0)
    try:
        e.set_frontend(compress_feats=1)
        e.load_gmm(models)
        e.set_system("OSI")
        ctx = _gmm_ctx(oracle, "OSI", models, cfg=oracle.default_cfg(compress_feats=1))
        g, o = _attack_pair(e, oracle, ctx, synthetic_audio(6, N), ATTACK_KW)
        r = e.debug_frontend_route()
        _long_route(r, N, 7)
        assert r["compress"] == where
        _same_trajectory(g, o)
        e.debug_feats((synthetic_audio(1, 16000) * 32768).astype(np.int16))      # one inside the window: fused in
        r = e.debug_frontend_route()
        assert r["compress"] == "fused" and r["chain"] == "whole"
    finally:
        e.close()


def test_mfcc_f32_attack_long_equals_the_oracle_twin(oracle, small_system):
    models = _gmm_models(small_system, "OSI")
    e = Engine(0)
    try:
        e.set_frontend(mfcc_f32=1)
        e.load_gmm(models)
        e.set_system("OSI")
        ctx = _gmm_ctx(oracle, "OSI", models, cfg=oracle.default_cfg(mfcc_f32=1))
        g, o = _attack_pair(e, oracle, ctx, synthetic_audio(6, 128000), ATTACK_KW)
        r = e.debug_frontend_route()
        assert r["mfcc"] == "k_mfcc_f32<12>" and r["chain"] == "separate+sliding" and r["t_max"] == 800
        _same_trajectory(g, o)
    finally:
        e.close()


def test_route_changes_on_one_engine(oracle, small_system):
    """Short attack that stops early -> long attack -> long score_raw batch -> short attack -> long get_grad on one engine:
    each result equal bit for bit to the same call on a fresh engine (the counters, tickets, epochs and exchange slots the
    fused and the separate front-end kernels share survive every switch)."""
    models = _gmm_models(small_system, "OSI")
    short, long_ = synthetic_audio(6, 16000), synthetic_audio(5, 80000)
    gc, miv, iv = stack_models(models)
    ctx = _gmm_ctx(oracle, "OSI", models)
    s0 = ctx.score(short[:, None])[0]
    stop = nes_params("OSI", "targeted", seed=1, samples_per_draw=4, max_iter=3, target=int(np.argmax(s0)),
                      threshold=float(s0.min() - 5.0), adver_thresh=-1.0)
    p = nes_params("OSI", "targeted", seed=11, stream=0, **ATTACK_KW)
    pg = nes_params("OSI", "targeted", samples_per_draw=6, seed=99, stream=3, target=1, threshold=0.05)
    batch = [(long_ * 32768).astype(np.int16), (short * 32768).astype(np.int16), (synthetic_audio(2, 130000) * 32768).astype(np.int16)]
    steps = [("stop", lambda e: e.attack(stop, short), "split"),
             ("long attack", lambda e: e.attack(p, long_), "separate+sliding"),
             ("long batch", lambda e: e.score_raw(batch), "separate+sliding"),
             ("short attack", lambda e: e.attack(p, short), "split"),
             ("long get_grad", lambda e: e.get_grad(pg, long_, it=4), "separate+sliding")]

    def fresh(fn):
        e = Engine(0)
        try:
            e.load_gmm(models)
            e.set_system("OSI")
            return fn(e)
        finally:
            e.close()

    e = Engine(0)
    try:
        e.load_gmm(models)
        e.set_system("OSI")
        for name, fn, chain in steps:
            got = fn(e)
            assert e.debug_frontend_route()["chain"] == chain, name
            want = fresh(fn)
            for a, b in zip(got, want):
                if isinstance(a, np.ndarray):
                    assert np.array_equal(a, b), name
                else:
                    assert a == b, name
            if name == "stop":
                assert got[1] == 1 and got[3].shape[0] == 1       # stopped on the device at the first iteration
    finally:
        e.close()
    raw_o, _ = oracle.gmm_score_batch(oracle.default_cfg(), batch, gc, miv, iv, nthreads=8)
    assert np.abs(fresh(lambda e: e.score_raw(batch))[0] - raw_o).max() <= SCORE_TOL


def _boundary_route(W, T):
    if T > W:
        return "separate+sliding"
    # k_vad_delta_cmvn_p needs ~104 T + 4 KB of LDS at D = 72 (at most 64 KB: T <= 590); k_vad_delta_cmvn and
    # k_delta_cmvn ~388 T + 4 KB (at most 150 KB: T <= 385) -- beyond both, the separate chain's whole-utterance mean
    return "split" if T <= 590 else "separate"


@pytest.mark.parametrize("W", [300, 301, 100, 600])
def test_cmn_window_boundary(oracle, small_system, W):
    models = _gmm_models(small_system, "OSI")
    gc, miv, iv = stack_models(models)
    cfg = oracle.default_cfg(cmn_window=W)
    e = Engine(0)
    try:
        e.set_frontend(cmn_window=W)
        e.load_gmm(models)
        e.set_system("OSI")
        wavs = [(synthetic_audio(10 + T - W, 160 * T) * 32768).astype(np.int16) for T in (W - 1, W, W + 1)]
        wavs.append((synthetic_audio(3, 9000) * 32768).astype(np.int16))
        raw_g, tv_g = e.score_raw(wavs)
        r = e.debug_frontend_route()
        assert r["t_max"] == W + 1 and r["chain"] == "separate+sliding"
        raw_o, tv_o = oracle.gmm_score_batch(cfg, wavs, gc, miv, iv, nthreads=8)
        assert np.array_equal(tv_g, tv_o) and np.abs(raw_g - raw_o).max() <= SCORE_TOL
        ctx = _gmm_ctx(oracle, "OSI", models, cfg=cfg)
        kw = dict(target=1, threshold=0.05)
        pg = nes_params("OSI", "targeted", samples_per_draw=4, seed=9, stream=0, **kw)
        po = oracle.nes_params("OSI", "targeted", ctx.S, samples_per_draw=4, **kw)
        for T in (W - 1, W, W + 1):
            audio = synthetic_audio(20 + T - W, 160 * T)
            g = e.get_grad(pg, audio, it=1)
            r = e.debug_frontend_route()
            assert r["t_max"] == T and r["chain"] == _boundary_route(W, T), (W, T, r)
            _check_grad(g, oracle.get_grad(po, ctx.fn, ctx.ctx, audio, seed=9, it=1, stream=0), pg.sigma)
    finally:
        e.close()
