"""The attack loop that does not drain its stream between looks, and the launch chains of a GPU shared by several attacks.

Once three engines of the process on one device are set to the shared-GPU chain (Engine.set_fused_chain(False)), an attack
of any of them queues the next look's iterations before it waits for the control block of the last look (fb_engine.hip:
fb_shared_gpu, loop_knobs, attack_loop); FB_LOOK_AHEAD=1 | 0 forces either loop.  A lone engine keeps the drained looks.
The five-launch chain -- k_gmm_finalize_loss finalises the scores and runs the loss body, the update stays
k_update_perturb: FB_FUSE_PARTS=7 FB_FUSE_UPD=0, measured and left out of the default -- is compared
with the six launches of the shared GPU and the four of a lone attack.  Everything here compares bits between chains and loops; the attacks that stop are compared with the CPU
oracle at the bar of tests/test_gpu_parity.py (same flag, same number of trace rows, trace within 1e-4, identical int16
audio), and so are the twelve-iteration chain cases.

Small systems: UBM + 5 speakers, C = 64, D = 72, one second of audio.  samples_per_draw = 10 gives B M = 66 finalising
workgroups (the fused chain's exchange-slot form), 100 gives 606 (its arrival counter; the update no longer rides along).
The stop cases take their thresholds from the oracle's own trajectory of the best score, and the oracle run with each
threshold says where the stop falls."""
import numpy as np
import pytest

from fakebob_amd.engine import Engine, nes_params
from fakebob_amd.models import stack_models, synthetic_audio, synthetic_gmm_system

pytestmark = pytest.mark.gpu
SCORE_TOL = 1e-4   # tests/test_gpu_parity.py
N_AUDIO = 16000
LOOK = 4           # iterations queued per look (FB_ATTACK_BATCH's default)
CHAIN_ENV = ("FB_NO_FUSE", "FB_FUSE_UPD", "FB_FUSE_PARTS", "FB_FIN_COUNTER", "FB_FIN_TICKET", "FB_ATTACK_BATCH", "FB_LOOK_AHEAD",
             "FB_UP_THREADS", "FB_GMM_SUB", "FB_MFCC_CUS", "FB_VAD_WHOLE")


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    for k in CHAIN_ENV:
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


@pytest.fixture(scope="module")
def models():
    ubm, spk = synthetic_gmm_system(n_speakers=5, C=64, D=72)
    return [ubm] + spk


@pytest.fixture(scope="module")
def audio():
    return synthetic_audio(6, N_AUDIO)


@pytest.fixture(scope="module")
def trio(models):
    """The engine under test and as many idle engines on the shared-GPU chain as make three on the device."""
    e = Engine(0)
    e.load_gmm(models)
    e.set_system("OSI")
    others = []
    yield e, others
    for o in others:
        o.close()
    e.close()


def _share(trio, shared):
    """shared: the engine under test runs as one of three on the shared-GPU chain; otherwise it is on its own there."""
    e, others = trio
    e.set_fused_chain(False)
    while shared and e.debug_shared_chain_engines() < 3:
        o = Engine(0)
        o.set_fused_chain(False)
        others.append(o)
    if not shared:
        for o in others:
            o.set_fused_chain(None)
    else:
        for o in others:
            o.set_fused_chain(False)
    return e


def _ctx(oracle, task, models):
    gc, miv, iv = stack_models(models)
    return oracle.GmmSystemCtx(oracle.default_cfg(), task, gc, miv, iv, nthreads=8)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def _same(a, b, what):
    assert a[1] == b[1], what
    assert a[3].shape == b[3].shape and np.array_equal(_bits(a[3]), _bits(b[3])), what
    assert np.array_equal(a[0], b[0]), what
    assert np.array_equal(_bits(a[2]), _bits(b[2])), what


def _launches(e):
    return {k: v for k, v in e.debug_nes_route().items() if v}


def _against_oracle(got, ref, p, what):
    adv_g, flag_g, advf_g, tr_g = got
    adv_o, flag_o, advf_o, tr_o = ref
    assert flag_g == flag_o and tr_g.shape == tr_o.shape, (what, flag_g, flag_o, tr_g.shape, tr_o.shape)
    assert np.abs(tr_g - tr_o).max() <= SCORE_TOL, what
    assert int(np.sum(adv_g != adv_o)) == 0, what
    assert np.abs(advf_g - advf_o).max() <= 2 * p.max_lr * p.max_iter, what


# ------------------------------------------------------------------ which chain runs
def test_three_engines_on_the_shared_chain_look_ahead_and_a_lone_one_drains(trio, audio, stops):
    """The stop at iteration 2 of 12 (three rows): a loop that drains has queued one look of four iterations, a loop that
    looks ahead two."""
    thr, ref = stops[2]
    p = nes_params("OSI", "untargeted", max_iter=12, threshold=thr, seed=STOP_SEED, stream=2, **STOP_KW)
    e = _share(trio, False)
    count = e.debug_shared_chain_engines()   # (engines other tests left on the shared chain count as well)
    lone = e.attack(p, audio)
    assert lone[3].shape[0] == 3 and lone[1] == 1
    assert _launches(e) == dict(k_loss=8 if count >= 3 else 4, k_update_perturb=8 if count >= 3 else 4), (_launches(e), count)
    e = _share(trio, True)
    assert e.debug_shared_chain_engines() >= 3
    shared = e.attack(p, audio)
    assert _launches(e) == dict(k_loss=8, k_update_perturb=8), _launches(e)
    assert e.debug_launch_shape()["up_threads"] == 256
    _same(lone, shared, "lone / shared")
    e.set_fused_chain(True)    # the engine under test leaves the shared chain: its attack is a lone attack's again
    fused = e.attack(p, audio)
    assert _launches(e) == dict(fin_loss_update=4), _launches(e)
    _same(lone, fused, "lone / fused")
    _against_oracle(shared, ref, p, "shared")


# ------------------------------------------------------------------ five, six and four launches: the same bits
# (task, attack, samples_per_draw, Philox seed).  The seeds are such that the engine reproduces the oracle's int16 audio, as
# tests/test_gpu_parity.py requires of its attacks.  That is a property of the seed, not a matter of course: the engine's
# float32 scores agree with the oracle's to 6e-7, which is an error of up to 1e-3 in a sample's gradient estimate (times
# |z| / sigma), and over 12 iterations x 16 000 samples the smallest momentum gradient of the oracle's trajectory is some
# 1e-5 -- a sample that near zero can take the other sign.  At samples_per_draw = 10 seed 21 has one (sample 10 931,
# oracle's momentum gradient 7.6e-5, one step of max_lr in the int16 audio); seed 2 has none, nor has 21 in the other two cases.
CHAIN_CASES = [("OSI", "targeted", 10, 2), ("OSI", "targeted", 100, 21), ("CSI", "untargeted", 10, 21)]


@pytest.mark.parametrize("task,attack,spd,seed", CHAIN_CASES)
def test_five_six_and_four_launch_chains_are_bit_identical(oracle, trio, models, audio, clean_env, task, attack, spd, seed):
    e = _share(trio, True)
    e.set_system(task)
    try:
        if task == "OSI":   # never stops: the threshold is out of reach
            kw = dict(samples_per_draw=spd, max_iter=12, target=2, threshold=1e3)
        else:               # CSI untargeted never stops: s[true] + kappa - max(others) stays positive
            kw = dict(samples_per_draw=spd, max_iter=12, true=1, adver_thresh=1e3)
        p = nes_params(task, attack, seed=seed, stream=3, **kw)
        half = spd // 2
        upd = "k_update_perturb" if half <= 40 else "k_grad_update"   # FB_FUSE_MAX_HALF
        # (name, shared, fused, environment, the launches of the loss and of the update)
        five = {"FB_FUSE_PARTS": "7", "FB_FUSE_UPD": "0"}
        chains = [("five", True, False, five, ("fin_loss", upd)),
                  ("five, drained looks", True, False, dict(five, FB_LOOK_AHEAD="0"), ("fin_loss", upd)),
                  ("five, lone", False, False, five, ("fin_loss", upd)),
                  ("six", True, False, {}, ("k_loss", upd)),
                  ("six, drained looks", True, False, {"FB_LOOK_AHEAD": "0"}, ("k_loss", upd)),
                  ("fused", False, True, {}, ("fin_loss_update",) if half <= 40 else ("fin_loss", upd))]
        got, state = {}, {}
        for name, shared, fused, env, route in chains:
            _share(trio, shared)
            e.set_fused_chain(fused)
            for k, v in env.items():
                clean_env.setenv(k, v)
            got[name] = e.attack(p, audio)
            assert _launches(e) == {k: 12 for k in route}, (name, _launches(e))
            e.bench_nes(p, audio, 0, 12)   # the same twelve iterations: the whole batch's scores and losses of the last one
            state[name] = e.bench_nes_state(p, audio.size)
            for k in env:
                clean_env.delenv(k, raising=False)
        ref, st = got["five"], state["five"]
        assert ref[3].shape[0] == 12 and ref[1] == -1
        assert np.any(ref[0] != (audio * 32768.0).astype(np.int16))
        for name in got:
            _same(ref, got[name], (task, spd, name))
            for k in ("adver", "scores", "loss"):
                assert np.array_equal(_bits(st[k]), _bits(state[name][k])), (task, spd, name, k)
            assert _bits(np.array([st["final_loss"], st["adver_loss"], st["distance"]])).tolist() == \
                _bits(np.array([state[name]["final_loss"], state[name]["adver_loss"], state[name]["distance"]])).tolist()
        assert np.array_equal(_bits(st["adver"]), _bits(ref[2]))   # bench_nes ran the attack's own twelve iterations
        # ... and the oracle's attack: the flag, the rows, the trace and the int16 audio
        ctx = _ctx(oracle, task, models)
        po = oracle.nes_params(task, attack, ctx.S, **kw)
        _against_oracle(ref, oracle.attack(po, ctx.fn, ctx.ctx, audio, seed=seed, stream=3), p, (task, spd, seed))
    finally:
        e.set_system("OSI")


# ------------------------------------------------------------------ looks with and without the drain
STOP_KW = dict(samples_per_draw=50)
STOP_SEED = 7   # (of seeds 1 .. 8 the one whose oracle trajectory rises by at least 0.016 per iteration: 160 x SCORE_TOL)


@pytest.fixture(scope="module")
def stops(oracle, models, audio):
    """{k: (threshold, the oracle's attack with it)} for stops at iteration k = 2 .. 5 (k + 1 trace rows), from the oracle's
    trajectory of the best score in an untargeted OSI attack that cannot stop: loss[0] = threshold - max(scores)
    (FAKEBOB.py:269) first falls below zero at iteration k when the threshold lies between the best score of iteration k
    and every earlier one.  (Untargeted: the threshold only shifts the losses, so the trajectory does not depend on it.)"""
    ctx = _ctx(oracle, "OSI", models)

    def run(max_iter, thr):
        po = oracle.nes_params("OSI", "untargeted", ctx.S, max_iter=max_iter, threshold=thr, **STOP_KW)
        return oracle.attack(po, ctx.fn, ctx.ctx, audio, seed=STOP_SEED, stream=2)
    s = run(6, 1e3)[3][:, 3:].max(axis=1)
    out = {}
    for k in (2, 3, 4, 5):
        assert s[k] - s[:k].max() > 20 * SCORE_TOL, (k, s)   # the fixture's own premise: a stop the score tolerance cannot move
        thr = 0.5 * (s[:k].max() + s[k])
        ref = run(12, thr)
        assert ref[3].shape[0] == k + 1 and ref[1] == 1, (k, ref[3].shape, ref[1])
        out[k] = (thr, ref)
    out["never"] = (1e3, run(6, 1e3))
    out["one"] = (1e3, run(1, 1e3))
    return out


def _after(e, p, audio):
    """What the calls that follow an attack return: a gradient estimate and a scoring batch."""
    fl, grad, al, sc = e.get_grad(p, audio, it=0)
    raw, tv = e.score_raw([(audio * 32768.0).astype(np.int16), (audio[:9000] * 32768.0).astype(np.int16)])
    return fl, grad, al, sc, raw, tv


@pytest.mark.parametrize("chain", ["six", "five", "fused"])
@pytest.mark.parametrize("case", [2, 3, 4, 5, "never", "one"])
def test_looks_without_the_drain_equal_drained_looks(trio, audio, stops, clean_env, chain, case):
    thr, ref = stops[case]
    max_iter = {"never": 6, "one": 1}.get(case, 12)
    p = nes_params("OSI", "untargeted", max_iter=max_iter, threshold=thr, seed=STOP_SEED, stream=2, **STOP_KW)
    e = _share(trio, chain != "fused")
    e.set_fused_chain(chain == "fused")
    if chain == "five":
        clean_env.setenv("FB_FUSE_PARTS", "7")
        clean_env.setenv("FB_FUSE_UPD", "0")
    kind = dict(six="k_loss", five="fin_loss", fused="fin_loss_update")[chain]
    res = {}
    for ahead in ("0", "1"):
        clean_env.setenv("FB_LOOK_AHEAD", ahead)
        got = e.attack(p, audio)
        rows = got[3].shape[0]
        queued = min(LOOK * ((rows + LOOK - 1) // LOOK), max_iter)
        if ahead == "1" and got[1] == 1:   # the stop is seen with the next look already queued
            queued = min(queued + LOOK, max_iter)
        assert _launches(e)[kind] == queued, (chain, case, ahead, rows, _launches(e))
        secs = e.attack_iter_seconds(rows)
        assert secs.shape == (rows,) and np.all(np.isfinite(secs)) and np.all(secs > 0.0), (chain, case, ahead, secs)
        res[ahead] = (got, _after(e, p, audio))
        _against_oracle(got, ref, p, (chain, case, ahead))
    clean_env.delenv("FB_LOOK_AHEAD")
    if chain != "fused":   # three engines on the shared chain: the loop looks ahead without being told to
        got = e.attack(p, audio)
        _same(res["1"][0], got, (chain, case, "default"))
        rows = got[3].shape[0]
        queued = min(LOOK * ((rows + LOOK - 1) // LOOK) + (LOOK if got[1] == 1 else 0), max_iter)
        assert _launches(e)[kind] == queued, (chain, case, rows, _launches(e))
    (a, after_a), (b, after_b) = res["0"], res["1"]
    _same(a, b, (chain, case))
    for x, y in zip(after_a, after_b):   # nothing of the batch queued ahead leaks into the next call
        assert np.array_equal(_bits(np.asarray(x)), _bits(np.asarray(y))), (chain, case)
