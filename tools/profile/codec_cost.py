"""What the telephone-line codec costs (fb_set_codec), at the headline size: UBM + 5 speakers, C = 2048, D = 72,
samples_per_draw 50, 3 s at 16 kHz -- 51 utterances of 48 000 samples per NES batch, k_mfcc_f32 route.  In the order run:
  1. the hook, HOOK_REPS calls each: fb_debug_codec over the 51 x 48 000 batch, then over 204 x 48 000 (the batch at eot 4),
     for mu-law, A-law and ADPCM (k_codec alone).  The kernels' own times come from a kernel trace
     (tools/profile/codec_cost.sh).
  2. Engine.bench_nes, one attack: no codec, each codec, and no codec again at r = 1; no codec and ADPCM at eot 4.
Prints one JSON line with the ms per NES step of each run."""
import json
import sys

import numpy as np

from fakebob_amd.engine import Engine, nes_params
from fakebob_amd.models import synthetic_audio, synthetic_gmm_system

HOOK_REPS = 5
KINDS = ("ulaw", "alaw", "adpcm")
HOOK_ROWS, SAMPLES = (51, 204), 48000
RUNS = [("none r=1", None, 1), ("ulaw r=1", "ulaw", 1), ("alaw r=1", "alaw", 1), ("adpcm r=1", "adpcm", 1),
        ("none r=4", None, 4), ("adpcm r=4", "adpcm", 4), ("none r=1 again", None, 1)]


def main(steps=100, warmup=10):
    ubm, spk = synthetic_gmm_system(n_speakers=5, C=2048, D=72)
    audio = synthetic_audio(0, SAMPLES)
    p = nes_params("OSI", "targeted", samples_per_draw=50, epsilon=0.002, sigma=0.001, max_lr=0.001, min_lr=1e-6,
                   momentum=0.9, max_iter=1000, target=1, threshold=1.0, seed=42)
    out = {"steps": steps, "warmup": warmup, "order": [r[0] for r in RUNS], "hook_reps": HOOK_REPS, "hook_kinds": list(KINDS),
           "hook_rows": list(HOOK_ROWS), "samples": SAMPLES}
    g = np.random.default_rng(0)
    e = Engine(0)
    try:
        for rows in HOOK_ROWS:
            batch = [g.integers(-3000, 3001, SAMPLES).astype(np.int16) for _ in range(rows)]
            for kind in KINDS:
                for _ in range(HOOK_REPS):
                    e.debug_codec(kind, batch)
        e.load_gmm([ubm] + spk)
        e.set_system("OSI")
        e.set_frontend(mfcc_f32=1)
        for name, codec, r in RUNS:
            e.set_codec(codec)
            e.set_eot(r)
            ms, _, rows = e.bench_nes(p, audio, warmup, steps)
            out[name] = dict(ms_per_step=ms / steps, its_per_s=1e3 * steps / ms, voiced_rows=rows)
    finally:
        e.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main(*(int(a) for a in sys.argv[1:3]))
