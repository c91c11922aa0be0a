"""What companion utterances cost: Engine.bench_nes at the headline size (UBM + 5 speakers, C = 2048, D = 72,
samples_per_draw 50, 3 s at 16 kHz: 51 rows of 48 000 samples per NES batch, k_mfcc_f32 route).  One attack, in the order
run: the unfused chain (fb_set_fused_chain(0)) with K = 1 -- the baseline the K > 1 chains are compared against, and what the
parent commit runs --, then K = 2 and K = 4 utterances with no chain, with `ms:7` and with `at:20`, and K = 2 under
fb_set_eot(2).  Prints one JSON line with the ms per NES step of each; under a kernel trace
(tools/profile/companions_cost.sh) the kernels' own times come from the trace."""
import json
import sys

from fakebob_amd.companions import cast_i16
from fakebob_amd.engine import Engine, nes_params
from fakebob_amd.models import synthetic_audio, synthetic_gmm_system

RUNS = [("none K=1", None, 1, 1)] + [("none K=%d" % k, None, k, 1) for k in (2, 4)] + \
       [("ms:7 K=%d" % k, "ms:7", k, 1) for k in (1, 2, 4)] + [("at:20 K=%d" % k, "at:20", k, 1) for k in (1, 2, 4)] + \
       [("at:20 K=2 r=2", "at:20", 2, 2), ("none K=1 again", None, 1, 1)]


def main(steps=100, warmup=10):
    ubm, spk = synthetic_gmm_system(n_speakers=5, C=2048, D=72)
    audio = synthetic_audio(0, 48000)
    comp = [cast_i16(synthetic_audio(1 + u, 48000)) for u in range(3)]
    p = nes_params("OSI", "targeted", samples_per_draw=50, epsilon=0.002, sigma=0.001, max_lr=0.001, min_lr=1e-6,
                   momentum=0.9, max_iter=1000, target=1, threshold=1.0, seed=42)
    out = {"steps": steps, "warmup": warmup, "order": [r[0] for r in RUNS]}
    e = Engine(0)
    try:
        e.load_gmm([ubm] + spk)
        e.set_system("OSI")
        e.set_fused_chain(False)
        e.set_frontend(mfcc_f32=1)
        for name, spec, k, r in RUNS:
            e.set_input_transform(spec)
            e.set_companions(None)
            e.set_eot(r)
            e.set_companions(comp[:k - 1])
            ms, _, rows = e.bench_nes(p, audio, warmup, steps)
            out[name] = dict(ms_per_step=ms / steps, voiced_rows=rows)
    finally:
        e.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main(*(int(a) for a in sys.argv[1:3]))
