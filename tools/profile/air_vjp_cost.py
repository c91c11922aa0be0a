"""What the white-box gradient through the over-the-air channel costs (fb_set_wb_air).  In the order run:
  1. the hooks, HOOK_REPS calls each, for rows in ROWS and L in HOOK_TAPS over rows x 48 000 samples: fb_debug_air_convolve
     (k_air_conv, the yardstick) and fb_debug_air_conv_t (k_air_conv_t) on the same taps; then, at L = 2048, the 8 rows as
     8 one-row launches of k_air_conv_t (the per-replica variant the engine does not run).  Their kernels' own times come
     from a kernel trace (tools/profile/air_vjp_cost.sh); FB_AIRT_PAD=16|17 in the environment times the other LDS layouts.
  2. (not with "hooks" as the first argument) Engine.attack_wb at the headline size -- UBM + 5 speakers, C = 2048, D = 72, 3 s
     at 16 kHz -- at eot 8 under fb_set_wb_bpda, without a channel and through a 2048-tap one: ms per iteration, wall clock
     over `steps` iterations after a warm-up attack.
Prints one JSON line."""
import json
import sys
import time

import numpy as np

from fakebob_amd.engine import Engine, nes_params
from fakebob_amd.models import synthetic_audio, synthetic_gmm_system

HOOK_REPS = 5
HOOK_TAPS = (512, 2048, 4096)
ROWS = (8, 32)
SAMPLES = 48000
SPEC = "t60:200-600,drr:6,taps:2048,delay:32"
RUNS = [("none eot=8", None), ("air eot=8", SPEC), ("none eot=8 again", None)]


def main(mode="all", steps=20, warmup=4):
    steps, warmup = int(steps), int(warmup)
    out = {"hook_reps": HOOK_REPS, "hook_taps": list(HOOK_TAPS), "rows": list(ROWS), "samples": SAMPLES, "order": [r[0] for r in RUNS],
           "steps": steps, "warmup": warmup}
    g = np.random.default_rng(0)
    e = Engine(0)
    try:
        for rows in ROWS:
            batch = [g.integers(-3000, 3001, SAMPLES).astype(np.int16) for _ in range(rows)]
            cot = g.normal(size=(rows, SAMPLES))
            for L in HOOK_TAPS:
                taps = g.integers(-2000, 2001, (rows, L)).astype(np.int16)
                for _ in range(HOOK_REPS):
                    e.debug_air_convolve(batch, taps)
                for _ in range(HOOK_REPS):
                    e.debug_air_conv_t(taps, cot)
        taps = g.integers(-2000, 2001, (8, 2048)).astype(np.int16)
        cot = g.normal(size=(8, SAMPLES))
        for _ in range(HOOK_REPS):
            for j in range(8):
                e.debug_air_conv_t(taps[j], cot[j])
        if mode != "hooks":
            ubm, spk = synthetic_gmm_system(n_speakers=5, C=2048, D=72)
            audio = synthetic_audio(0, SAMPLES)
            e.load_gmm([ubm] + spk)
            e.set_system("OSI")
            e.set_frontend(mfcc_f32=1)
            e.set_eot(8)
            e.set_wb_bpda(True)
            e.set_wb_air(True)
            for name, spec in RUNS:
                e.set_air_channel(spec)
                p = nes_params("OSI", "targeted", epsilon=0.002, max_lr=0.001, min_lr=1e-6, momentum=0.9, target=1, threshold=1e3,
                               adver_thresh=1e6, seed=42, max_iter=warmup)     # (adver_thresh: never stops early)
                e.attack_wb(p, audio)
                p.max_iter = steps
                t0 = time.perf_counter()
                _adv, _flag, _f, trace = e.attack_wb(p, audio)
                dt = time.perf_counter() - t0
                out[name] = dict(ms_per_iter=1e3 * dt / trace.shape[0], iters=int(trace.shape[0]), air_launches=e.debug_wb_air_route())
    finally:
        e.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main(*sys.argv[1:4])
