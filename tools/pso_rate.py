#!/usr/bin/env python
"""PSO iterations per second on the benchmark's GMM-UBM OSI system (bench.py's headline: 5 speakers + UBM, C = 2048,
D = 72, float32 MFCC, 3 s of audio): one engine, one attack in flight, the stop disabled by a large adver_thresh.

    python tools/pso_rate.py [--particles 25 51] [--iters 200]

Prints one JSON line per swarm size: iterations/s over the whole fb_attack_pso call (wall clock around it, after a short
warm-up attack), the mean and the median of the per-iteration host times (fb_attack_iter_seconds) and the best loss at both
ends.  A P = 51 iteration scores the batch an NES iteration at samples_per_draw = 50 scores, plus one look of the host: compare
with `bench.py --full`'s `single_attack` on the same machine in the same session.  k_pso_step's own time comes from a kernel trace of
this script (rocprofv3 --kernel-trace --stats -- python tools/pso_rate.py ...), not from here."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--particles", nargs="+", type=int, default=[25, 51])
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--samples", type=int, default=48000)
    args = ap.parse_args()
    from fakebob_amd.engine import Engine, nes_params, pso_params
    from fakebob_amd.models import synthetic_audio, synthetic_gmm_system
    ubm, spk = synthetic_gmm_system(5, 2048, 72)
    e = Engine(0)
    try:
        e.set_frontend(mfcc_f32=1)
        e.load_gmm([ubm] + list(spk))
        e.set_system("OSI")
        e.set_fused_chain(True)                 # what a lone attack runs
        audio = synthetic_audio(0, args.samples)
        for P in args.particles:
            kw = dict(epsilon=0.002, adver_thresh=1e6, target=0, threshold=0.2277, seed=42, stream=0)
            q = pso_params(particles=P, v_max=0.002)
            e.attack_pso(nes_params("OSI", "targeted", max_iter=5, **kw), q, audio)
            t0 = time.perf_counter()
            _adv, flag, _advf, trace, _losses = e.attack_pso(nes_params("OSI", "targeted", max_iter=args.iters, **kw), q, audio)
            dt = time.perf_counter() - t0
            secs = e.attack_iter_seconds(trace.shape[0])
            print(json.dumps(dict(particles=P, samples=args.samples, iterations=int(trace.shape[0]), flag=int(flag),
                                  iterations_per_s=trace.shape[0] / dt, ms_per_iteration=1e3 * dt / trace.shape[0],
                                  iter_ms_mean=1e3 * float(secs.mean()), iter_ms_median=1e3 * float(np.median(secs)),
                                  best_loss_first=float(trace[0, 0]), best_loss_last=float(trace[-1, 0]))))
    finally:
        e.close()


if __name__ == "__main__":
    main()
