#!/usr/bin/env python
"""White-box iterations through the i-vector-PLDA victim (fb_set_wb_ivector) on the benchmark's i-vector SV system (bench.py
--arch iv, BASELINE.json configs[2]: C = 2048, D = 72, R = 400, LDA 200, one enrolled speaker, float32 MFCC, 3 s of audio):
one engine, one attack in flight.

    python tools/wb_iv_rate.py [--iters 100] [--repeats 2] [--out profiles/wb_iv_rate.jsonl] [--trace-only]

Writes one JSON line per measurement (and prints it):
  rate      iterations/s of fb_attack_wb with the stop disabled, the mean and median of the device's per-iteration times, the
            launches of the last call, the active components and the bytes k_wb_iv_stats_t streams for them,
            n_active * (R (R + 1) / 2 + D R) * 8
  cosine    between fb_get_grad's NES estimate at samples_per_draw = 1030 and the exact gradient, three seeds
  crossing  iterations fb_attack_wb (PGD, the attack's defaults) and fb_attack (NES, samples_per_draw = 50) need to reach
            adver_loss < 0 on the same utterance at a threshold `--margin` above the clean score
The time of each new launch comes from a kernel trace of this script in a run of its own, the program after the `--`:
    rocprofv3 --kernel-trace --stats -- python tools/wb_iv_rate.py --trace-only
(--trace-only: the warm-up and one attack of --iters iterations, nothing else).  k_wb_iv_stats_t's time against
bytes / HBM bandwidth is the achieved fraction DESIGN.md section 6 records."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--samples", type=int, default=48000)
    ap.add_argument("--margin", type=float, default=0.5, help="crossing: the threshold above the clean score (z-normalised units)")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "wb_iv_rate.jsonl"))
    ap.add_argument("--trace-only", action="store_true")
    args = ap.parse_args()
    from fakebob_amd.engine import Engine, nes_params
    from fakebob_amd.models import synthetic_audio, synthetic_ivector_system
    C_, D_, R_, L_ = 2048, 72, 400, 200
    sy = synthetic_ivector_system(C=C_, D=D_, R=R_, L=L_, n_speakers=1)
    sy = sy.with_enrolled(sy.enrolled, [-40.0], [10.0])
    lines = []

    def emit(**rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
    e = Engine(0)
    try:
        e.set_frontend(mfcc_f32=1)
        e.load_ivector(sy, "SV")
        e.set_fused_chain(True)                 # what a lone attack runs
        e.set_wb_ivector(True)
        audio = synthetic_audio(0, args.samples)
        never = dict(epsilon=0.002, adver_thresh=1e6, threshold=1.0)
        e.attack_wb(nes_params("SV", "targeted", max_iter=5, **never), audio)
        for rep in range(1 if args.trace_only else args.repeats):
            p = nes_params("SV", "targeted", max_iter=args.iters, **never)
            t0 = time.perf_counter()
            _adv, flag, _advf, trace = e.attack_wb(p, audio)
            dt = time.perf_counter() - t0
            secs = e.attack_iter_seconds(trace.shape[0])
            n_active = e.debug_iv_active()
            emit(what="rate", repeat=rep, samples=args.samples, iterations=int(trace.shape[0]), flag=int(flag),
                 iterations_per_s=trace.shape[0] / dt, ms_per_iteration=1e3 * dt / trace.shape[0],
                 iter_ms_mean=1e3 * float(secs.mean()), iter_ms_median=1e3 * float(np.median(secs)), launches=e.debug_wb_route(),
                 n_active=int(n_active), stats_t_bytes=int(n_active) * (R_ * (R_ + 1) // 2 + D_ * R_) * 8,
                 loss_first=float(trace[0, 1]), loss_last=float(trace[-1, 1]))
        if not args.trace_only:
            g, al, sc = e.get_grad_wb(nes_params("SV", "targeted", threshold=1.0), audio)
            for seed in (1, 2, 3):
                p = nes_params("SV", "targeted", threshold=1.0, samples_per_draw=1030, sigma=0.001, seed=seed)
                _fl, est, _al, _sc = e.get_grad(p, audio)
                est = np.asarray(est, np.float64).reshape(-1)
                emit(what="cosine", seed=seed, samples_per_draw=1030, sigma=0.001,
                     cosine=float(est @ g / (np.linalg.norm(est) * np.linalg.norm(g))), adver_loss=float(al))
            thr = float(sc[0]) + args.margin
            pgd = nes_params("SV", "targeted", threshold=thr, epsilon=0.002, max_iter=1000)
            _adv, flag_w, _advf, trace_w = e.attack_wb(pgd, audio)
            nes = nes_params("SV", "targeted", threshold=thr, epsilon=0.002, max_iter=1000, samples_per_draw=50, sigma=0.001, seed=42)
            _adv, flag_n, _advf, trace_n = e.attack(nes, audio)
            emit(what="crossing", clean_score=float(sc[0]), threshold=thr, pgd_iterations=int(trace_w.shape[0]), pgd_flag=int(flag_w),
                 nes_iterations=int(trace_n.shape[0]), nes_flag=int(flag_n), nes_samples_per_draw=50)
    finally:
        e.close()
    if not args.trace_only:
        with open(args.out, "w") as w:
            w.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
