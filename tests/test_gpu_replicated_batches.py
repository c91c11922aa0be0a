"""Replicated NES batches row by row at the recipe's batch size (fb_set_eot, fb_set_companions, dither and feature
compression inside fb_get_grad / fb_attack; include/fakebob_hip.h: "Row order", "Averaging").  tests/replicated_ref.py says
what the device must have computed for EVERY NES row b from paths that know nothing of replication; here the device's
loss[B] and scores[B][S] of iteration 0 -- read back with fb_bench_nes_state after one fb_bench_nes iteration, the batch
fb_get_grad(it = 0) builds -- are held against it at B = 51 .. 257, up to K * eot = 32 replicas and 1632 scored rows, on
GMM and i-vector systems, on the long-utterance front-end route and under FeCo and dither with companions.

Tolerances, each the one the suite already states for the same pair of paths:
  SCORE_TOL (tests/test_gpu_input_transform.py, from tests/test_gpu_properties.py): a row of an NES batch against a scoring
      call of the same utterance.  The contract's mean of R such rows keeps the bound, so scores and the linear SV loss take
      1 x SCORE_TOL; the OSI and CSI losses are a difference of two scores: 2 x SCORE_TOL, as in tests/test_gpu_eot.py and
      tests/test_gpu_companions.py.
  1e-4 (tests/test_gpu_feco.py): a score against the float64 mean of fb_debug_gmm_frames -- the FeCo
      case -- and the same 1e-4 tests/test_gpu_dither.py allows between fb_debug_feats_dither's features and a score -- the
      dither case.
The i-vector case (204 rows) and the z-normed CSI case had no bound of their own; both were measured against this reference
and sit inside SCORE_TOL (MEASURED below), which is therefore kept.

MEASURED on an MI355X, max over all rows b of |device - reference|, scores / loss (allowed):
  calibration    51 rows  0        / 0        (2e-6 / 4e-6)      large-B  514 rows  2.03e-7 / 1.53e-7 (2e-6 / 4e-6)
  recipe-eot    204 rows  0        / 0        (2e-6 / 4e-6)      ivector  204 rows  0       / 0       (2e-6 / 2e-6)
  full-replicas 1632 rows 1.05e-7  / 1.05e-7  (2e-6 / 4e-6)      long      28 rows  0       / 0       (2e-6 / 4e-6)
  below-256     255 rows  0        / 0        (2e-6 / 2e-6)      feco      28 rows  1.91e-6 / 1.91e-6 (1e-4 / 1e-4)
  above-256     265 rows  0        / 0        (2e-6 / 2e-6)      dither    28 rows  1.08e-6 / 1.08e-6 (1e-4 / 1e-4)
(0: on the float64 front end a row gets the same bits in a replicated batch as in a scoring call of 64 rows.)"""
import numpy as np
import pytest

from fakebob_amd import companions as CP, input_transform as T
from fakebob_amd._native import FB_E_NO_VOICED, NativeError
from fakebob_amd.engine import Engine, nes_params
from fakebob_amd.models import synthetic_audio, synthetic_gmm_system
from tests import replicated_ref as RR
from tests.test_gpu_eot import _gmm, _iv_sv, _same
from tests.test_gpu_input_transform import SCORE_TOL   # the bound between an NES batch's row and a scoring call

pytestmark = pytest.mark.gpu
FRAMES_TOL = 1e-4       # a score against the float64 mean of per-frame log-likelihoods (test_gpu_feco.py, test_gpu_dither.py)
Z_MEAN8 = np.array([-80.0, -75.0, -90.0, -85.0, -70.0, -78.0, -88.0, -82.0])
Z_STD8 = np.array([3.0, 2.0, 4.0, 2.5, 3.5, 2.0, 3.0, 4.0])


def _tolerances(case):
    """(scores, loss) allowed for a case: see the module docstring"""
    if case["mode"] in ("feco", "dither"):
        return FRAMES_TOL, FRAMES_TOL
    return SCORE_TOL, (1 if case["task"] == "SV" else 2) * SCORE_TOL


def _engine(case, small_system):
    if case["system"] == "ivector":
        return _iv_sv()
    if case["system"] == "gmm8":
        _ubm, spk = synthetic_gmm_system(n_speakers=8, C=256)
        e = Engine(0)
        e.load_gmm(spk)
        e.set_system("CSI", Z_MEAN8, Z_STD8)
        return e
    return _gmm(small_system, case["task"])


_RESULTS = {}


def _result(name, small_system, oracle):
    """One run per case, shared by the tests below: the reference, then the device's iteration 0 on an engine configured as
    the case says, fb_get_grad of the same batch, the composing launch and the row counters."""
    if name in _RESULTS:
        if isinstance(_RESULTS[name], BaseException):                   # (a case that failed is not run again for the next test)
            raise _RESULTS[name]
        return _RESULTS[name]
    try:
        _RESULTS[name] = _run_case(name, small_system, oracle)
    except BaseException as ex:
        _RESULTS[name] = ex
        raise
    return _RESULTS[name]


def _run_case(name, small_system, oracle):
    case = RR.CASES[name]
    audio, comp = RR.case_audio(case)
    p = RR.case_params(case)
    chain = T.parse(case["chain"])
    r, n = case["eot"], case["n"]
    bare, scorer, d = Engine(0), _engine(case, small_system), _engine(case, small_system)
    try:
        if case["mode"] == "dither":
            scorer.set_frontend(dither=RR.DITHER)
            d.set_frontend(dither=RR.DITHER)
        ref = RR.reference(oracle, bare, scorer, p, audio, RR.case_lossdef(case), comp=comp, chain=chain, r=r,
                           mode=case["mode"], feco_cfg=RR.FECO_CFG, it=RR.IT)
        d.set_input_transform(chain)
        d.set_eot(r)
        if comp is not None:
            d.set_companions(comp)
        if case["mode"] == "feco":
            d.set_feature_compression(*RR.FECO_CFG)
        composed = d.debug_compose(ref["q"], ref["q"][0], r, RR.SEED, RR.STREAM, RR.IT)
        s0 = d.stats()["scored_utts"]
        d.bench_nes(p, audio, 0, 1)                                     # iteration 0 of the attack: the batch of it = 0
        s1 = d.stats()["scored_utts"]
        state = d.bench_nes_state(p, n)
        fl, _g, al, sc0 = d.get_grad(p, audio, it=RR.IT, want_grad=False)
        s2 = d.stats()["scored_utts"]
        route = d.debug_frontend_route()
    finally:
        bare.close()
        scorer.close()
        d.close()
    S = ref["scores"].shape[1]
    out = dict(case=case, ref=ref, composed=composed, loss=state["loss"], scores=state["scores"][:, :S], fl=fl, al=al,
               sc0=np.asarray(sc0)[:S], counts=(s1 - s0, s2 - s1), route=route, p=p)
    return out


REPLICATED = [c for c in RR.CASES if c != "calibration"]


# ------------------------------------------------------------------------------------------------ calibration
def test_the_captured_rows_are_the_batch(small_system, oracle):
    """K = 1, eot = 1, no chain, B = 51: loss[b] and scores[b] of the state against per-row scoring calls of the rows
    captured from fb_get_grad_ext -- the captured rows ARE the rows the native batch holds, before any other case relies on it."""
    res = _result("calibration", small_system, oracle)
    ref = res["ref"]
    assert ref["rep_l"].shape == (51, 1) and res["loss"].shape == (51,)
    d_sc, d_l = np.abs(res["scores"] - ref["scores"]).max(), np.abs(res["loss"] - ref["loss"]).max()
    print("calibration: scores %.3g (allowed %.3g) loss %.3g (allowed %.3g)" % (d_sc, SCORE_TOL, d_l, 2 * SCORE_TOL))
    assert d_sc <= SCORE_TOL and d_l <= 2 * SCORE_TOL
    assert np.ptp(ref["loss"][1:]) > 10 * 2 * SCORE_TOL                 # the rows differ: another row's values would not pass
    assert np.array_equal(res["composed"][:, 0, 0], ref["q"])           # K = 1, r = 1, no chain: the copy
    assert res["counts"] == (51, 51)


# ------------------------------------------------------------------------------------------------ every case
@pytest.mark.parametrize("name", REPLICATED)
def test_composition_to_the_bit(small_system, oracle, name):
    res = _result(name, small_system, oracle)
    case, ref = res["case"], res["ref"]
    B = 2 * (case["spd"] // 2) + 1
    assert res["composed"].shape == (B, case["K"], case["eot"], case["n"]) == ref["rows"].shape
    assert np.array_equal(res["composed"], ref["rows"])


@pytest.mark.parametrize("name", REPLICATED)
def test_scores_and_losses_of_every_row(small_system, oracle, name):
    res = _result(name, small_system, oracle)
    case, ref = res["case"], res["ref"]
    tol_sc, tol_l = _tolerances(case)
    B = 2 * (case["spd"] // 2) + 1
    assert res["loss"].shape == (B,) and res["scores"].shape == ref["scores"].shape and ref["tv"].shape == (case["rows"],)
    assert np.all(ref["tv"] > 0)                                        # no row is skipped or masked
    e_sc = np.abs(res["scores"] - ref["scores"]).max(axis=1)
    e_l = np.abs(res["loss"] - ref["loss"])
    print("%s (%d rows, %s): scores max %.3g at b = %d (allowed %.3g), loss max %.3g at b = %d (allowed %.3g)"
          % (name, case["rows"], res["route"], e_sc.max(), e_sc.argmax(), tol_sc, e_l.max(), e_l.argmax(), tol_l))
    assert e_sc.max() <= tol_sc, (int(e_sc.argmax()), float(e_sc.max()))
    assert e_l.max() <= tol_l, (int(e_l.argmax()), float(e_l.max()))


@pytest.mark.parametrize("name", REPLICATED)
def test_get_grad_agrees_and_the_rows_are_counted(small_system, oracle, name):
    """fb_get_grad of the same (seed, stream, it): adver_loss and score0 are row 0 of the reference, final_loss the numpy mean
    of loss[1:] (FAKEBOB.py:243; a mean of values each within the loss bound); fb_stats counts exactly B * K * eot rows per
    batch, on the attack loop and on fb_get_grad."""
    res = _result(name, small_system, oracle)
    case, ref = res["case"], res["ref"]
    tol_sc, tol_l = _tolerances(case)
    want_fl = oracle.np_sum(ref["loss"][1:]) / float(case["spd"] // 2 * 2)
    print("%s: score0 %.3g adver_loss %.3g final_loss %.3g" % (name, np.abs(res["sc0"] - ref["scores"][0]).max(),
                                                                abs(res["al"] - ref["loss"][0]), abs(res["fl"] - want_fl)))
    assert np.abs(res["sc0"] - ref["scores"][0]).max() <= tol_sc
    assert abs(res["al"] - ref["loss"][0]) <= tol_l
    assert abs(res["fl"] - want_fl) <= tol_l
    assert res["counts"] == (case["rows"], case["rows"])


@pytest.mark.parametrize("name", REPLICATED)
def test_the_case_is_not_a_formality(small_system, oracle, name):
    """On the reference arrays alone: the replicas of some row differ by far more than the tolerance (the mean is a mean of
    different things), and a batch whose rows 1 and B - 1 were exchanged would fail the comparison."""
    res = _result(name, small_system, oracle)
    case, ref = res["case"], res["ref"]
    tol_sc, tol_l = _tolerances(case)
    B = ref["loss"].size
    assert np.ptp(ref["rep_l"], axis=1).max() > 10 * tol_l
    loss_x, scores_x = RR.swap_replicas(ref, 1, B - 1)
    assert abs(loss_x[1] - ref["loss"][1]) > tol_l and abs(loss_x[B - 1] - ref["loss"][B - 1]) > tol_l
    assert np.abs(scores_x[1] - ref["scores"][1]).max() > tol_sc
    assert np.array_equal(loss_x[2:B - 1], ref["loss"][2:B - 1]) and loss_x[0] == ref["loss"][0]


def test_routes_the_cases_were_chosen_for(small_system, oracle):
    """long: more frames than cmn_window (the other VAD / CMVN route); large-B: B - 1 > 128, B > 256 and B * S > 2048"""
    long_ = _result("long", small_system, oracle)
    assert long_["route"]["t_max"] > 300 and long_["route"]["B"] == 28
    assert -(-RR.CASES["long"]["n"] // 4096) == 12
    big = _result("large-B", small_system, oracle)
    B, S = big["ref"]["scores"].shape
    assert B == 257 and S == 8 and B * S > 2048 and B - 1 > 128
    assert _result("above-256", small_system, oracle)["case"]["rows"] > 256 > _result("below-256", small_system, oracle)["case"]["rows"]


# ------------------------------------------------------------------------------------------------ a replica without voiced frames
@pytest.mark.parametrize("kind", ["gmm", "ivector"])
def test_a_replica_without_voiced_frames_is_refused(small_system, kind):
    """One companion of digital silence: utterance 1 of NES row 0 is clip(0 + q_0 - a_0) = 0 everywhere, so that replica has
    no voiced frame.  fb_get_grad and fb_attack return FB_E_NO_VOICED (k_loss_eot's my_err path, behind the split i-vector
    tail too), and once the companions are cleared the engine runs a fresh engine's attack bit for bit."""
    n, spd = 4000, 6
    task, kw = ("OSI", dict(target=1)) if kind == "gmm" else ("SV", {})
    mk = (lambda: _gmm(small_system, "OSI")) if kind == "gmm" else _iv_sv
    p = nes_params(task, "targeted", samples_per_draw=spd, max_iter=5, epsilon=0.002, threshold=1e3, seed=5, stream=1, **kw)
    audio = synthetic_audio(9, n)
    silence = np.zeros((1, n), np.int16)
    a0 = CP.cast_i16(audio)
    assert not np.any(CP.compose(a0, a0, silence[0]))
    e, fresh = mk(), mk()
    try:
        base = fresh.attack(p, audio)
        assert base[3].shape[0] == 5 and np.all(np.isfinite(base[3]))
        e.set_companions(silence)
        for call in (lambda: e.get_grad(p, audio, it=0), lambda: e.attack(p, audio)):
            with pytest.raises(NativeError) as ex:
                call()
            assert ex.value.code == FB_E_NO_VOICED
        e.set_companions(None)
        assert _same(base, e.attack(p, audio))
    finally:
        e.close()
        fresh.close()


# ------------------------------------------------------------------------------------------------ launch chains at recipe size
def _recipe_attack(system, monkeypatch, batch=None, fused=None, no_fuse=False):
    case = RR.CASES["recipe-eot"]
    for k, v in (("FB_ATTACK_BATCH", batch), ("FB_NO_FUSE", "1" if no_fuse else None)):
        if v is None:
            monkeypatch.delenv(k, raising=False)
        else:
            monkeypatch.setenv(k, str(v))
    e = _gmm(system, "OSI")
    try:
        e.set_input_transform(case["chain"])
        e.set_eot(case["eot"])
        e.set_fused_chain(fused)
        p = nes_params("OSI", "targeted", samples_per_draw=case["spd"], max_iter=5, target=1, epsilon=0.002, threshold=1e3,
                       seed=5, stream=2)
        return e.attack(p, synthetic_audio(9, case["n"]))
    finally:
        e.close()
        monkeypatch.delenv("FB_ATTACK_BATCH", raising=False)
        monkeypatch.delenv("FB_NO_FUSE", raising=False)


def test_recipe_size_attack_is_the_same_on_every_launch_chain(small_system, monkeypatch):
    """B = 51, eot = 4, at:20, five iterations: a fresh engine, 1 and 4 iterations queued per host look, the 6-launch chain and
    every launch on its own give the same bits -- the small-batch property of tests/test_gpu_eot.py at 204 rows."""
    a = _recipe_attack(small_system, monkeypatch)
    assert a[3].shape[0] == 5 and np.all(np.isfinite(a[3]))
    assert _same(a, _recipe_attack(small_system, monkeypatch))
    assert _same(a, _recipe_attack(small_system, monkeypatch, batch=1))
    assert _same(a, _recipe_attack(small_system, monkeypatch, batch=4))
    assert _same(a, _recipe_attack(small_system, monkeypatch, fused=False))
    assert _same(a, _recipe_attack(small_system, monkeypatch, no_fuse=True))
