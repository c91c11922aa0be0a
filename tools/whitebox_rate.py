#!/usr/bin/env python
"""White-box iterations per second on the benchmark's GMM-UBM OSI system (bench.py's headline: 5 speakers + UBM, C = 2048,
D = 72, float32 MFCC, 3 s of audio): one engine, one attack in flight, the stop disabled by a large adver_thresh.

    python tools/whitebox_rate.py [--iters 200] [--repeats 3]

Prints one JSON line per repeat: iterations/s of fb_attack_wb over the whole call (wall clock around it, after a short warm-up
attack) with the mean and the median of the device's per-iteration times (fb_attack_iter_seconds), and -- alternating with
it in the same process -- the same figures of fb_attack at samples_per_draw = 50.  A white-box iteration scores ONE row and
runs the backward; an NES iteration scores 51 rows.  The backward kernels' own times come from a kernel trace of this script
(rocprofv3 --kernel-trace --stats -- python tools/whitebox_rate.py --repeats 1), in a run of its own, not from here."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--samples", type=int, default=48000)
    args = ap.parse_args()
    from fakebob_amd.engine import Engine, nes_params
    from fakebob_amd.models import synthetic_audio, synthetic_gmm_system
    ubm, spk = synthetic_gmm_system(5, 2048, 72)
    e = Engine(0)
    try:
        e.set_frontend(mfcc_f32=1)
        e.load_gmm([ubm] + list(spk))
        e.set_system("OSI")
        e.set_fused_chain(True)                 # what a lone attack runs
        audio = synthetic_audio(0, args.samples)
        kw = dict(epsilon=0.002, adver_thresh=1e6, target=0, threshold=0.2277, seed=42, stream=0)
        runs = (("whitebox", lambda p: e.attack_wb(p, audio), dict(samples_per_draw=0)),
                ("nes_spd50", lambda p: e.attack(p, audio), dict(samples_per_draw=50)))
        for _name, fn, extra in runs:
            fn(nes_params("OSI", "targeted", max_iter=5, **dict(kw, **extra)))
        for rep in range(args.repeats):
            for name, fn, extra in runs:
                p = nes_params("OSI", "targeted", max_iter=args.iters, **dict(kw, **extra))
                t0 = time.perf_counter()
                _adv, flag, _advf, trace = fn(p)
                dt = time.perf_counter() - t0
                secs = e.attack_iter_seconds(trace.shape[0])
                print(json.dumps(dict(attack=name, repeat=rep, samples=args.samples, iterations=int(trace.shape[0]), flag=int(flag),
                                      iterations_per_s=trace.shape[0] / dt, ms_per_iteration=1e3 * dt / trace.shape[0],
                                      iter_ms_mean=1e3 * float(secs.mean()), iter_ms_median=1e3 * float(np.median(secs)),
                                      loss_first=float(trace[0, 1]), loss_last=float(trace[-1, 1]))))
    finally:
        e.close()


if __name__ == "__main__":
    main()
