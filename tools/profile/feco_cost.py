"""What feature compression costs: Engine.bench_nes at the headline size (UBM + 5 speakers, C = 2048, D = 72,
samples_per_draw 50, 3 s at 16 kHz: 51 utterances of 48 000 samples per NES batch, k_mfcc_f32 route).  One attack, in the
order run: no compression on the fused chain and on the unfused chain (what r > 1 runs on), ratio 0.2 and 0.5 at 10
iterations with r = 1 (fused) and r = 4, then the first run again.  Prints one JSON line with the ms per NES step of each;
under a kernel trace (tools/profile/feco_cost.sh) the kernel's own time comes from the trace."""
import json
import sys

from fakebob_amd.engine import Engine, nes_params
from fakebob_amd.models import synthetic_audio, synthetic_gmm_system

RUNS = [("none r=1", None, 1, True), ("none r=1 unfused", None, 1, False)] + \
       [("feco %s r=%d" % (ratio, r), ratio, r, r == 1) for ratio in (0.2, 0.5) for r in (1, 4)] + [("none r=1 again", None, 1, True)]


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
        e.set_frontend(mfcc_f32=1)
        for name, ratio, r, fused in RUNS:
            e.set_fused_chain(fused)
            e.set_feature_compression(ratio, 10)
            e.set_eot(r)
            ms, _, rows = e.bench_nes(p, audio, warmup, steps)
            out[name] = dict(ms_per_step=ms / steps, scored_rows=rows)
    finally:
        e.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main(*(int(a) for a in sys.argv[1:3]))
