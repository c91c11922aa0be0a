#!/usr/bin/env python
"""What the white-box gradient through an x-vector victim costs (fb_set_wb_xvector): the stock TDNN (24 -> 512 x 4 -> 1500, R 512)
on 3 s of audio.

    python tools/xvector_wb_rate.py --what kernels|attack|cosine|race [--samples 48000] [--reps 10] [--repeat 5] [--iters 30]

One step per process, so that a caller can give every step a time limit of its own.  Prints JSON lines (one engine, nothing else
of this process on the GPU):
  kernels  at 1 and 8 utterances of 298 rows: median over --repeat of the milliseconds per launch (device events around --reps
           launches after one to warm up; fb_bench_xv_backward, fb_bench_xvector) of every kernel of the backward and, beside
           them, the forward's; k_wb_xv_affine_t's FLOP (2 * rows * K * dout per layer, the padding not counted) and TFLOP/s.
  attack   milliseconds per fb_attack_wb iteration (host clock around --iters iterations that never stop, after a warm-up
           call) at r = 1 and at eot = 8 behind noise:8 with BPDA, beside a forward-only scoring call of the same rows.
  cosine   the cosine between NES estimates at samples_per_draw = 1030 (three seeds) and the analytic gradient.
  race     iterations of fb_attack_wb and of fb_attack (NES, samples_per_draw = 50) to the same margin, same step rule."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
T_FRAMES = 298          # frames of 3 s at 10 ms (snip-edges)


def emit(**kw):
    print(json.dumps(kw))
    sys.stdout.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", required=True, choices=("kernels", "attack", "cosine", "race"))
    ap.add_argument("--samples", type=int, default=48000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--iters", type=int, default=30)
    args = ap.parse_args()
    from fakebob_amd import companions as CP
    from fakebob_amd.engine import Engine, nes_params
    from fakebob_amd.models import synthetic_audio, synthetic_xvector_system
    n = args.samples
    e = Engine(0)
    try:
        e.set_frontend(delta_order=0, mfcc_f32=1)
        sy = synthetic_xvector_system(e.feat_dim)
        sy = sy.with_enrolled(sy.enrolled, [-40.0], [10.0])
        e.load_xvector(sy, "SV")
        e.set_wb_xvector(True)
        nl = len(sy.layers)
        audio = synthetic_audio(0, n)
        if args.what == "kernels":
            flop_per_row = [2.0 * ly["W"].shape[0] * ly["W"].shape[1] for ly in sy.layers]
            for B in (1, 8):
                bw = [e.bench_xv_backward(B, T_FRAMES, reps=args.reps) for _ in range(args.repeat)]
                fw = [e.bench_xvector(B, T_FRAMES, reps=args.reps) for _ in range(args.repeat)]
                med = lambda runs, f: float(np.median([f(r) for r in runs]))   # noqa: E731
                per = lambda runs, key: [med(runs, lambda r, l=l: r[key][l]) for l in range(nl)]   # noqa: E731
                rows = B * T_FRAMES
                aff_t, aff = per(bw, "affine_t"), per(fw, "affine")
                flop = rows * sum(flop_per_row)
                backward = dict(k_wb_xv_segment_t=med(bw, lambda r: r["segment_t"]), k_wb_xv_pool_t=med(bw, lambda r: r["pool_t"]),
                                k_wb_xv_act_t=per(bw, "act_t"), k_wb_xv_affine_t=aff_t, k_wb_xv_unsplice=per(bw, "unsplice"))
                total = backward["k_wb_xv_segment_t"] + backward["k_wb_xv_pool_t"] + sum(backward["k_wb_xv_act_t"]) + sum(aff_t) + sum(backward["k_wb_xv_unsplice"])
                emit(what="kernels", utterances=B, rows=rows, backward_solo_launch_ms=backward, backward_ms=total,
                     forward_solo_launch_ms=dict(k_xv_affine=aff, k_xv_rowmax=per(fw, "rowmax"), k_xv_pool=med(fw, lambda r: r["pool"]),
                                                 k_xv_segment=med(fw, lambda r: r["segment"])),
                     k_wb_xv_affine_t_ms=sum(aff_t), k_wb_xv_affine_t_TFLOPs=flop / (sum(aff_t) * 1e-3) / 1e12,
                     k_wb_xv_affine_t_TFLOPs_per_layer=[rows * f / (t * 1e-3) / 1e12 for f, t in zip(flop_per_row, aff_t)],
                     k_xv_affine_ms=sum(aff), k_xv_affine_TFLOPs=flop / (sum(aff) * 1e-3) / 1e12, repeat=args.repeat, reps=args.reps)
        elif args.what == "attack":
            wav = CP.cast_i16(audio, 16)
            for r, chain in ((1, None), (8, "noise:8")):
                e.set_input_transform(chain)
                e.set_eot(r)
                e.set_wb_bpda(r > 1)
                p = nes_params("SV", "targeted", adver_thresh=1e6, threshold=0.0, samples_per_draw=0, seed=3, max_iter=args.iters)
                e.attack_wb(p, audio)
                times = []
                for _ in range(args.repeat):
                    t0 = time.perf_counter()
                    trace = e.attack_wb(p, audio)[3]
                    times.append((time.perf_counter() - t0) / trace.shape[0])
                xr = e.debug_wb_xv_route()
                e.set_eot(1)            # the forward alone: a scoring call of the same r rows (the chain draws per row)
                e.score_raw([wav] * r)
                t0 = time.perf_counter()
                for _ in range(args.iters):
                    e.score_raw([wav] * r)
                fwd = (time.perf_counter() - t0) / args.iters
                emit(what="attack", eot=r, chain=chain, iters=int(trace.shape[0]), attack_wb_ms_per_iter=1e3 * float(np.median(times)),
                     scoring_call_ms=1e3 * fwd, launches_of_the_last_call=xr, repeat=args.repeat)
            e.set_input_transform(None)
            e.set_wb_bpda(False)
        elif args.what == "cosine":
            pw = nes_params("SV", "targeted", threshold=0.0, samples_per_draw=0)
            g, al, _sc = e.get_grad_wb(pw, audio)
            cos = []
            for seed in (3, 4, 5):
                pn = nes_params("SV", "targeted", threshold=0.0, samples_per_draw=1030, seed=seed)
                _fl, gn, _al, _s = e.get_grad(pn, audio, it=0)
                gn = np.asarray(gn, np.float64).reshape(-1)
                cos.append(float(gn @ g / (np.linalg.norm(gn) * np.linalg.norm(g))))
            emit(what="cosine", samples_per_draw=1030, cosines=cos, adver_loss=al)
        else:
            s0 = float(e.system_scores(e.score_raw([CP.cast_i16(audio, 16)])[0])[0][0])
            for margin in (0.05, 0.2):
                kw = dict(threshold=s0 + margin, epsilon=0.002, max_lr=0.001, max_iter=400, seed=3)
                tw = e.attack_wb(nes_params("SV", "targeted", samples_per_draw=0, **kw), audio)
                tn = e.attack(nes_params("SV", "targeted", samples_per_draw=50, **kw), audio)
                emit(what="race", margin=margin, score0=s0, attack_wb_iters=int(tw[3].shape[0]), attack_wb_flag=int(tw[1]),
                     nes_iters=int(tn[3].shape[0]), nes_flag=int(tn[1]))
    finally:
        e.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
