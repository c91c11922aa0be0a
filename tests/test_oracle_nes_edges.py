"""Pins the oracle's NES engine (oracle/fb_oracle.c) against the reference's own FAKEBOB.py at the parameter values
where the product's NES step switches kernels or paths (tests/golden/make_golden_nes_edges.py): samples_per_draw 8 ..
1030, 7 .. 62 speakers, plateau windows of 1, 8, 9 and 12 losses, utterances of 3, 255 and 257 samples.  Float64 /
integer arithmetic throughout, so the bar is bit-exact equality, as in test_oracle_nes.py."""
import numpy as np
import pytest

from tests import nes_edges_ref as R
from tests.golden.synth_model import SynthModel, synth_audio


@pytest.fixture(scope="module")
def g11():
    return R.load()


def test_g11_covers_the_switch_points(g11):
    z, meta = g11
    assert [c["spd"] for c in meta["get_grad"]] == [8, 14, 66, 80, 82, 126, 128, 130, 300, 302, 1030]
    assert all(c["N"] == (259 if c["spd"] == 1030 else 515) and c["n_spk"] == 5 for c in meta["get_grad"])
    at = meta["attack"]
    assert sorted(c["fbkw"]["plateau_length"] for c in at if c["name"].startswith("plateau")) == [1, 8, 9, 12]
    assert sorted(c["n_spk"] for c in at if c["fbkw"]["samples_per_draw"] == 130) == [7, 8, 9, 62]
    assert sorted(c["n_spk"] for c in at if c["name"].startswith("osi_untargeted_S")) == [7, 8, 9, 62]
    assert sorted(c["N"] for c in at if c["name"].startswith("osi_targeted_N")) == [3, 255, 257]
    for i, c in enumerate(at):
        lrs = z["lrs_%d" % i]
        if c["name"].startswith("plateau") and c["fbkw"]["plateau_length"] > 1:
            assert lrs.min() < lrs.max(), c["name"]               # the rate did drop


def test_g11_get_grad(oracle, g11):
    z, meta = g11
    for i, c in enumerate(meta["get_grad"]):
        model = SynthModel(c["task"], c["n_spk"], c["N"], seed=c["model_seed"])
        audio = synth_audio(c["N"], c["audio_seed"])
        half = c["spd"] // 2
        noise = R.noise_stream(c["noise_seed"], c["N"], half, 1)[0]
        p = oracle.nes_params(c["task"], c["attack"], model.S, adver_thresh=c["kappa"], samples_per_draw=c["spd"],
                              sigma=0.001, threshold=c["thr"], target=c["target"], true=c["true"])
        fl, grad, al, sc = oracle.get_grad(p, oracle.py_score_fn(model.score, model.S), None, audio, noise_pos=noise)
        assert fl == float(z["final_loss_%d" % i]), c
        assert al == float(z["adver_loss_%d" % i].reshape(-1)[0]), c
        assert np.array_equal(sc, z["score_%d" % i].reshape(-1)), c
        assert np.array_equal(grad, z["grad_%d" % i].reshape(-1)), c
        assert model.n_scored == 2 * half + 1


def test_g11_attack_trajectories(oracle, g11):
    z, meta = g11
    for i, c in enumerate(meta["attack"]):
        fb, at = c["fbkw"], c["atkw"]
        model = SynthModel(c["task"], c["n_spk"], c["N"], seed=c["model_seed"])
        audio, noise = R.attack_inputs(c)
        p = oracle.nes_params(c["task"], c["attack"], model.S, adver_thresh=fb["adver_thresh"],
                              epsilon=fb["epsilon"], max_iter=fb["max_iter"], max_lr=fb["max_lr"],
                              min_lr=fb["min_lr"], samples_per_draw=fb["samples_per_draw"], sigma=fb["sigma"],
                              momentum=fb["momentum"], plateau_length=fb["plateau_length"],
                              plateau_drop=fb["plateau_drop"], threshold=at.get("threshold", 0.0),
                              target=at.get("target"), true=at.get("true"))
        adv, flag, adv_f, trace = oracle.attack(p, oracle.py_score_fn(model.score, model.S), None, audio, noise_all=noise)
        want = z["trace_%d" % i]
        assert flag == c["flag"], c["name"]
        assert trace.shape[0] == c["n_rows"] == want.shape[0]
        assert model.n_calls == c["n_get_grad"]
        assert np.array_equal(trace[:, 0], want[:, 0]), c["name"]      # distance
        assert np.array_equal(trace[:, 1], want[:, 1]), c["name"]      # adver_loss
        assert np.array_equal(trace[:, 3:], want[:, 2:]), c["name"]    # score of the clean sample
        assert adv.dtype == np.int16 and np.array_equal(adv, R.adv_i16(z, i, audio)), c["name"]
        lrs = z["lrs_%d" % i]                                          # printed with %f
        assert lrs.shape[0] == c["n_rows"] and not c["last_time_is_zero"]
        assert np.abs(trace[:, 2] - lrs).max() <= 5.1e-7, c["name"]
