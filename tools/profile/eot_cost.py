"""What a randomised victim and expectation over transformation cost: Engine.bench_nes at the headline size (UBM + 5
speakers, C = 2048, D = 72, samples_per_draw 50, 3 s at 16 kHz: 51 utterances of 48 000 samples per NES batch, k_mfcc_f32
route).  One attack, in the order run: the unfused chain (fb_set_fused_chain(0)) with no chain and r = 1 -- the baseline
the r > 1 chains are compared against --, `noise:30` and `at:20` at r = 1, then `at:20` and dither 1.0 (no chain) at
r = 1, 2, 4, 8.  Prints one JSON line with the ms per NES step of each; under a kernel trace (tools/profile/eot_cost.sh)
the kernels' own times come from the trace."""
import json
import sys

from fakebob_amd.engine import Engine, nes_params
from fakebob_amd.models import synthetic_audio, synthetic_gmm_system

RUNS = [("none r=1", None, 0.0, 1), ("noise:30 r=1", "noise:30", 0.0, 1)] + \
       [("at:20 r=%d" % r, "at:20", 0.0, r) for r in (1, 2, 4, 8)] + \
       [("dither 1 r=%d" % r, None, 1.0, r) for r in (1, 2, 4, 8)] + [("none r=1 again", None, 0.0, 1)]


def main(steps=100, warmup=10):
    ubm, spk = synthetic_gmm_system(n_speakers=5, C=2048, D=72)
    audio = synthetic_audio(0, 48000)
    p = nes_params("OSI", "targeted", samples_per_draw=50, epsilon=0.002, sigma=0.001, max_lr=0.001, min_lr=1e-6,
                   momentum=0.9, max_iter=1000, target=1, threshold=1.0, seed=42)
    out = {"steps": steps, "warmup": warmup, "order": [r[0] for r in RUNS]}
    e = Engine(0)
    try:
        e.load_gmm([ubm] + spk)
        e.set_system("OSI")
        e.set_fused_chain(False)
        for name, spec, dither, r in RUNS:
            e.set_frontend(mfcc_f32=1, dither=dither)
            e.set_input_transform(spec)
            e.set_eot(r)
            ms, _, rows = e.bench_nes(p, audio, warmup, steps)
            out[name] = dict(ms_per_step=ms / steps, voiced_rows=rows)
    finally:
        e.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main(*(int(a) for a in sys.argv[1:3]))
