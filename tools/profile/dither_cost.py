"""What Kaldi's dither costs: Engine.bench_nes at the headline size (UBM + 5 speakers, C = 2048, D = 72, samples_per_draw
50, 3 s at 16 kHz: 51 utterances, 15 300 frames per NES batch) with dither 0 and 1 on both MFCC routes (k_mfcc_f32, the
bench / drop-in route; k_mfcc_r16, the library default).  Prints one JSON line with the ms per NES step of each of the four;
run it under a kernel-stats trace (tools/profile/dither_cost.sh) for the kernels' own times."""
import json
import sys

from fakebob_amd.engine import Engine, nes_params
from fakebob_amd.models import synthetic_audio, synthetic_gmm_system


def main(steps=200, warmup=20):
    ubm, spk = synthetic_gmm_system(n_speakers=5, C=2048, D=72)
    audio = synthetic_audio(0, 48000)
    p = nes_params("OSI", "targeted", samples_per_draw=50, epsilon=0.002, sigma=0.001, max_lr=0.001, min_lr=1e-6,
                   momentum=0.9, max_iter=1000, target=1, threshold=1.0, seed=42)
    out = {}
    e = Engine(0)
    try:
        e.load_gmm([ubm] + spk)
        e.set_system("OSI")
        e.set_fused_chain(True)
        for route, f32, dither in (("f32", 1, 0.0), ("f32", 1, 1.0), ("r16", 0, 0.0), ("r16", 0, 1.0)):
            e.set_frontend(mfcc_f32=f32, dither=dither)
            ms, _, rows = e.bench_nes(p, audio, warmup, steps)
            out["%s_dither%g" % (route, dither)] = dict(ms_per_step=ms / steps, mfcc=e.debug_frontend_route()["mfcc"],
                                                        voiced_rows=rows)
    finally:
        e.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main(*(int(a) for a in sys.argv[1:3]))
