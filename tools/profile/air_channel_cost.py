"""What the over-the-air channel costs (fb_set_air_channel), at the headline size: UBM + 5 speakers, C = 2048, D = 72,
samples_per_draw 50, 3 s at 16 kHz -- 51 utterances of 48 000 samples per NES batch, k_mfcc_f32 route.  In the order run:
  1. the hooks, HOOK_REPS calls each: fb_debug_air_convolve over the 51 x 48 000 batch with L = 512, 2048, 4096 taps
     (k_air_conv alone), then fb_debug_input_transform of the same batch through one 511-tap FIR stage (k_input_transform:
     the yardstick).  Their kernels' own times come from a kernel trace (tools/profile/air_channel_cost.sh).
  2. Engine.bench_nes, one attack on the unfused chain: no channel at r = 1, the channel (L = 2048) at r = 1, no channel at
     eot 4 (the replicating copy), the channel at eot 4, and no channel at r = 1 again.
Prints one JSON line with the ms per NES step of each run."""
import json
import sys

import numpy as np

from fakebob_amd import input_transform as T
from fakebob_amd.engine import Engine, nes_params
from fakebob_amd.models import synthetic_audio, synthetic_gmm_system

HOOK_REPS = 5
HOOK_TAPS = (512, 2048, 4096)
ROWS, SAMPLES = 51, 48000
SPEC = "t60:200-600,drr:6,taps:2048,delay:32"
RUNS = [("none r=1", None, 1), ("air r=1", SPEC, 1), ("none r=4", None, 4), ("air r=4", SPEC, 4), ("none r=1 again", None, 1)]


def main(steps=100, warmup=10):
    ubm, spk = synthetic_gmm_system(n_speakers=5, C=2048, D=72)
    audio = synthetic_audio(0, SAMPLES)
    p = nes_params("OSI", "targeted", samples_per_draw=50, epsilon=0.002, sigma=0.001, max_lr=0.001, min_lr=1e-6,
                   momentum=0.9, max_iter=1000, target=1, threshold=1.0, seed=42)
    out = {"steps": steps, "warmup": warmup, "order": [r[0] for r in RUNS], "hook_reps": HOOK_REPS, "hook_taps": list(HOOK_TAPS),
           "rows": ROWS, "samples": SAMPLES}
    g = np.random.default_rng(0)
    batch = [g.integers(-3000, 3001, SAMPLES).astype(np.int16) for _ in range(ROWS)]
    e = Engine(0)
    try:
        for L in HOOK_TAPS:
            taps = g.integers(-2000, 2001, (ROWS, L)).astype(np.int16)
            for _ in range(HOOK_REPS):
                e.debug_air_convolve(batch, taps)
        e.set_input_transform([T.fir(np.full(511, 1.0 / 511))])
        for _ in range(HOOK_REPS):
            e.debug_input_transform(batch)
        e.set_input_transform(None)
        e.load_gmm([ubm] + spk)
        e.set_system("OSI")
        e.set_fused_chain(False)
        e.set_frontend(mfcc_f32=1)
        for name, spec, r in RUNS:
            e.set_air_channel(spec)
            e.set_eot(r)
            ms, _, rows = e.bench_nes(p, audio, warmup, steps)
            out[name] = dict(ms_per_step=ms / steps, its_per_s=1e3 * steps / ms, voiced_rows=rows)
    finally:
        e.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main(*(int(a) for a in sys.argv[1:3]))
