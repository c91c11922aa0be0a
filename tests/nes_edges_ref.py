"""Reads tests/golden/g11_* (make_golden_nes_edges.py: the reference's FAKEBOB.py at the NES step's switch points) for
tests/test_oracle_nes_edges.py and tests/test_gpu_nes_edges.py, and rebuilds what the generator did not store: the
np.random.normal tensors the reference drew and the int16 adversarial audio.  Not part of the product."""
import json
import os

import numpy as np

from tests.golden.synth_model import synth_audio

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load():
    """-> (the arrays of g11_nes_edges.npz as a dict, g11_meta.json)."""
    with open(os.path.join(G, "g11_meta.json")) as r:
        meta = json.load(r)
    with np.load(os.path.join(G, "g11_nes_edges.npz")) as z:
        return {k: z[k] for k in z.files}, meta


def noise_stream(seed, N, half, count):
    """The tensors np.random.normal(size=(N, half)) returned to the reference, call by call -> (count, N, half)."""
    rs = np.random.RandomState(seed)
    return np.stack([rs.normal(size=(N, half)) for _ in range(count)])


def attack_inputs(c):
    """-> (audio, noise_all) of an attack case."""
    audio = synth_audio(c["N"], c["audio_seed"])
    fb = c["fbkw"]
    return audio, noise_stream(c["noise_seed"], c["N"], fb["samples_per_draw"] // 2, fb["max_iter"])


def adv_i16(z, i, audio):
    """The reference's int16 adversarial audio of attack case i: stored as its difference to the cast of the clean one."""
    q = (audio * 32768.0).astype(np.int16)
    adv = q.astype(np.int32) + z["dadv_%d" % i].astype(np.int32)
    assert np.abs(adv).max() <= 32767
    return adv.astype(np.int16)


def replay_noise(engine, seed, stream, n, half, iters, oracle=None):
    """The device's Philox normals of iterations 0 .. iters - 1 as the noise_all an attack takes: float32 widened to
    float64, transposed to [N][half] (tests/test_gpu_plugin_api.py: test_philox_path_and_error_propagation).  With the
    oracle fixture handed in, the tensor must be the oracle generator's bit for bit: the replay then stands on the oracle,
    not on k_noise."""
    z = np.stack([engine.debug_noise(seed, it, stream, n, half) for it in range(iters)])
    if oracle is not None:
        assert np.array_equal(z.view(np.uint32), np.stack([oracle.noise(seed, it, stream, n, half) for it in range(iters)]).view(np.uint32))
    return np.ascontiguousarray(z.astype(np.float64).transpose(0, 2, 1))
