"""No call-scoped state survives a call.  What a scoring call tells the engine about its batch -- the point of the RNG
contracts, the replica layout, the stop flag, the deferred finalisation, the requested loss tail -- belongs to that call
alone: after an NES call under every such setting at once, a plain scoring call on the same engine returns what a fresh
engine with the same settings returns, bit for bit."""
import numpy as np
import pytest

from fakebob_amd.engine import nes_params
from fakebob_amd.models import synthetic_audio
from tests.test_gpu_eot import _cast, _gmm, _iv_sv

pytestmark = pytest.mark.gpu
N = 16000
SEED = 77


def _configure(e):
    e.set_frontend(dither=1.0)
    e.set_input_transform("at:20")          # one SNR noise stage
    e.set_feature_compression(0.5, 4)
    e.set_dither_seed(SEED)


def _same_bits(a, b):
    return np.array_equal(a[0].view(np.uint64), b[0].view(np.uint64)) and np.array_equal(a[1], b[1])


@pytest.mark.parametrize("kind", ["gmm", "ivector"])
def test_a_scoring_call_after_an_nes_call_is_a_fresh_engines(small_system, kind):
    task, kw = ("OSI", dict(target=1)) if kind == "gmm" else ("SV", {})
    mk = (lambda: _gmm(small_system, "OSI")) if kind == "gmm" else _iv_sv
    p = nes_params(task, "targeted", samples_per_draw=6, max_iter=2, epsilon=0.002, threshold=1e3, seed=5, stream=3, **kw)
    audio = synthetic_audio(9, N)
    batch = [_cast(synthetic_audio(5, 12000)), _cast(synthetic_audio(6, 9000))]   # unequal lengths
    e, fresh = mk(), mk()
    try:
        _configure(fresh)
        want = fresh.score_raw(batch)
        assert np.all(np.isfinite(want[0])) and np.all(want[1] > 0)
        _configure(e)
        e.set_companions([synthetic_audio(3, N), synthetic_audio(4, N)])
        e.set_eot(2)
        fl, _g, al, _sc = e.get_grad(p, audio, it=2, want_grad=False)   # 3 utterances x 2 draws of every NES row
        assert np.isfinite(fl) and np.isfinite(al)
        e.set_companions(None)
        e.set_eot(1)
        e.set_dither_seed(SEED)             # the serial of scoring calls returns to 0
        assert _same_bits(want, e.score_raw(batch))
        # and behind an attack without replicas: the device-controlled loop's stop flag, the finalisation left to the fused
        # launch (GMM) and the loss body in the solve kernels' tail (i-vector)
        trace = e.attack(p, audio)[3]
        assert trace.shape[0] == 2 and np.all(np.isfinite(trace))
        e.set_dither_seed(SEED)
        assert _same_bits(want, e.score_raw(batch))
        fresh.set_dither_seed(SEED + 1)     # not a formality: the scoring call does depend on the point it stands at
        assert not _same_bits(want, fresh.score_raw(batch))
    finally:
        e.close()
        fresh.close()
