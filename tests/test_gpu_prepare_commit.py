"""fb_load_gmm prepares on the host and commits afterwards: what the engine reports after a load is the plan the
engine-free hook computes for the same arrays and environment, and a refused load leaves the engine scoring the system
it had, bit for bit."""
import numpy as np
import pytest

from fakebob_amd import prepare
from fakebob_amd._native import FB_E_ARG, NativeError
from fakebob_amd.engine import Engine
from fakebob_amd.models import stack_models, synthetic_audio, synthetic_gmm_system

pytestmark = pytest.mark.gpu
KNOBS = ("FB_GMM_MODE", "FB_GMM_NARROW", "FB_GMM_DELTA_P", "FB_GMM_DELTA_BUDGET", "FB_GMM_DELTA_F6")


def _system(M):
    ubm, spk = synthetic_gmm_system(n_speakers=M - 1, C=64, D=72)
    return stack_models([ubm] + spk)


@pytest.mark.parametrize("M", [3, 11])
def test_engine_reports_the_hooks_plan_and_a_refused_load_changes_nothing(M, monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    arrays = _system(M)
    plan, _ = prepare.gmm_plan(*arrays)
    n_tiles = plan["n_tiles"]
    eng = Engine(0)
    eng.load_gmm_arrays(*arrays)
    assert eng.gmm_kernel == {1: "bx3", 2: "fx2"}[plan["mode"]]
    assert plan["delta_p"] != 0 and eng.gmm_kernel_variant == "fx2w/%d" % plan["delta_p"]
    assert eng.gmm_shift_rms == plan["delta_rms"]
    assert eng.gmm_delta_tiles == (n_tiles - plan["t2"], plan["t2"] - plan["t6"], plan["t3"])
    assert eng.gmm_delta_tiles_f6 == plan["t6"] - plan["t3"]
    wavs = [(synthetic_audio(u, n) * 32768.0).astype(np.int16) for u, n in ((0, 16000), (1, 10777))]
    before, tv = eng.score_raw(wavs)
    assert np.all(np.isfinite(before)) and np.all(tv > 0)
    # a load the environment refuses: other arrays (the speakers in reverse order), FB_GMM_DELTA_P=7 for this call only
    other = [np.ascontiguousarray(a[[0] + list(range(M - 1, 0, -1))]) for a in arrays]
    monkeypatch.setenv("FB_GMM_DELTA_P", "7")
    with pytest.raises(NativeError) as ex:
        eng.load_gmm_arrays(*other)
    monkeypatch.delenv("FB_GMM_DELTA_P")
    assert ex.value.code == FB_E_ARG and "FB_GMM_DELTA_P must be 1, 2, 3 or 6 (got '7')" in str(ex.value)
    assert eng.gmm_kernel_variant == "fx2w/%d" % plan["delta_p"]
    after, tv2 = eng.score_raw(wavs)
    assert np.array_equal(before.view(np.uint64), after.view(np.uint64)) and np.array_equal(tv, tv2)
    # ... and the refused arrays load once the environment is right: the speakers' columns come out reversed
    eng.load_gmm_arrays(*other)
    swapped, _ = eng.score_raw(wavs)
    assert np.allclose(swapped, before[:, [0] + list(range(M - 1, 0, -1))], rtol=0, atol=2e-5)   # (tests/test_gpu_configs.py's bound)
    eng.close()
