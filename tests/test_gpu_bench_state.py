"""fb_bench_nes_state: what bench.py --dump-outputs reads back after the timed steps.  The attack bench_nes leaves on
the device is the one attack() runs (early stop out of reach here), reading it back does not disturb it, and two
engines given the same inputs hold the same bits."""
import numpy as np
import pytest

from fakebob_amd.engine import Engine, nes_params
from fakebob_amd.models import synthetic_audio

pytestmark = pytest.mark.gpu


def test_bench_state_is_the_attack_and_reading_it_back_changes_nothing(engine, small_system):
    ubm, spk = small_system
    n_it, spd = 6, 6
    # adver_thresh far above any score gap: adver_loss never drops below zero, so attack() runs all max_iter iterations
    p = nes_params("OSI", "targeted", samples_per_draw=spd, target=1, threshold=0.05, adver_thresh=10.0, seed=42,
                   stream=3, max_iter=n_it)
    audio = synthetic_audio(7, 16000)
    engine.load_gmm([ubm] + spk)
    engine.set_system("OSI")
    adv, flag, advf, trace = engine.attack(p, audio)
    assert trace.shape[0] == n_it

    other = Engine(0)
    try:
        other.load_gmm([ubm] + spk)
        other.set_system("OSI")
        with pytest.raises(Exception):
            other.bench_nes_state(p, audio.size)                    # nothing resident yet: an error, not stale memory
        other.bench_nes(p, audio, 0, n_it // 2)
        mid = other.bench_nes_state(p, audio.size)
        assert mid["adver"].shape == audio.shape and mid["scores"].shape == (spd + 1, 3) and mid["loss"].shape == (spd + 1,)
        other.bench_nes(p, audio, -1, n_it - n_it // 2)             # continues the attack the read-back looked at
        st = other.bench_nes_state(p, audio.size)
        assert not np.array_equal(st["adver"], mid["adver"])
        again = other.bench_nes_state(p, audio.size)
        for k in st:
            assert np.array_equal(st[k], again[k]), k
    finally:
        other.close()

    assert np.array_equal(st["adver"], advf)                        # the adversarial audio after the last update
    assert st["distance"] == trace[-1, 0] and st["adver_loss"] == trace[-1, 1]
    assert np.array_equal(st["scores"][0], trace[-1, 3:])           # row 0: the unperturbed adversarial audio
    assert st["adver_loss"] == st["loss"][0]
    assert np.abs(st["adver"] - audio).max() <= 0.002 + 1e-12       # inside the epsilon ball
    assert np.isfinite(st["scores"]).all() and np.isfinite(st["loss"]).all()
