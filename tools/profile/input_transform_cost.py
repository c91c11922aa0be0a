"""What an input-transform chain costs: Engine.bench_nes at the headline size (UBM + 5 speakers, C = 2048, D = 72,
samples_per_draw 50, 3 s at 16 kHz: 51 utterances of 48 000 samples per NES batch, k_mfcc_f32 route, fused chain) with no
chain and with each of qt:512, ms:7, ms:31, a 101-tap FIR, a 511-tap FIR and ds:2.  Prints one JSON line with the ms per NES
step of each, in the order run; under a kernel trace (tools/profile/input_transform_cost.sh) the n-th group of k_input_transform
dispatches is the n-th chain's."""
import json
import sys

import numpy as np

from fakebob_amd import input_transform as T
from fakebob_amd.engine import Engine, nes_params
from fakebob_amd.models import synthetic_audio, synthetic_gmm_system

CHAINS = [("none", None), ("qt:512", "qt:512"), ("ms:7", "ms:7"), ("ms:31", "ms:31"), ("fir:101", "lpf:4000:101"),
          ("fir:511", "lpf:4000:511"), ("ds:2", "ds:2"), ("none again", None)]


def main(steps=200, warmup=20):
    ubm, spk = synthetic_gmm_system(n_speakers=5, C=2048, D=72)
    audio = synthetic_audio(0, 48000)
    p = nes_params("OSI", "targeted", samples_per_draw=50, epsilon=0.002, sigma=0.001, max_lr=0.001, min_lr=1e-6,
                   momentum=0.9, max_iter=1000, target=1, threshold=1.0, seed=42)
    out = {"steps": steps, "warmup": warmup, "order": [n for n, _ in CHAINS]}
    e = Engine(0)
    try:
        e.load_gmm([ubm] + spk)
        e.set_system("OSI")
        e.set_fused_chain(True)
        e.set_frontend(mfcc_f32=1)
        for name, spec in CHAINS:
            e.set_input_transform(spec)
            ms, _, rows = e.bench_nes(p, audio, warmup, steps)
            out[name] = dict(ms_per_step=ms / steps, stages=len(e.input_transform),
                             halo=int(np.sum([T.radius(s) for s in e.input_transform])), voiced_rows=rows)
    finally:
        e.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main(*(int(a) for a in sys.argv[1:3]))
