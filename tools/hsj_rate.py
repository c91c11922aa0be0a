#!/usr/bin/env python
"""What HopSkipJump costs and reaches on the benchmark's GMM-UBM OSI system (bench.py's headline: 5 speakers + UBM, C = 2048,
D = 72, float32 MFCC, 3 s of audio).

    python tools/hsj_rate.py [--samples 48000] [--reps 20] [--iters 30] [--snr 65.5]

Prints JSON lines:
  what=kernels   for B = 50 and B = 1024: milliseconds per launch of every HopSkipJump kernel alone (device events around
                 --reps launches; fb_bench_hsj_kernels) next to the NES batch launch (k_perturb) of 2 ceil(B / 2) + 1 rows in
                 the same process, and the per-row ratios probes / NES batch and direction / NES batch.  probes_keep and
                 dir_kept are the pair that hands the normals over as float32 [B][N] instead of drawing them twice.
  what=host      the host's median seconds per iteration of an attack (fb_attack_iter_seconds) next to a plain scoring call
                 (fb_score_i16) of as many rows as an iteration of it scores.
  what=result    the attack itself: audio 0, the target is the clean runner-up and the threshold its clean score (the
                 setting of tools/cw2_rate.py), the start the first synthetic voice the system decides as that speaker or,
                 when there is none, the white-box attack's first success at a large epsilon: the queries and iterations until
                 the returned row reaches --snr dB (CW2's figure on this audio and target), and where it stands after --iters
                 iterations."""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def emit(**kw):
    print(json.dumps(kw))
    sys.stdout.flush()


def snr_db(x0, adv):
    d = adv.astype(np.float64) - x0.astype(np.float64)
    n = float(np.sum(d * d))
    return float("inf") if n == 0.0 else 10.0 * math.log10(float(np.sum(x0.astype(np.float64) ** 2)) / n)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=48000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--snr", type=float, default=65.5)
    ap.add_argument("--score-reps", dest="score_reps", type=int, default=10)
    args = ap.parse_args()
    from fakebob_amd import companions as CP
    from fakebob_amd.engine import Engine, hsj_params, nes_params
    from fakebob_amd.models import synthetic_audio, synthetic_gmm_system
    ubm, spk = synthetic_gmm_system(5, 2048, 72)
    n = args.samples
    e = Engine(0)
    try:
        e.set_frontend(mfcc_f32=1)
        e.load_gmm([ubm] + list(spk))
        e.set_system("OSI")
        e.set_fused_chain(True)                 # what a lone attack runs
        audio = synthetic_audio(0, n)
        x0 = CP.cast_i16(audio, 16)
        other = synthetic_audio(1, n)
        for B in (50, 1024):
            ms = e.bench_hsj_kernels(audio, other, B, G=15, reps=args.reps)
            nes_rows = 2 * ((B + 1) // 2) + 1
            per_row = ms["nes_batch"] / nes_rows
            emit(what="kernels", samples=n, B=B, nes_rows=nes_rows, **dict(
                {k + "_ms": v for k, v in ms.items()}, probes_per_nes_row=(ms["probes"] / B) / per_row,
                dir_draw_per_nes_row=(ms["dir_draw"] / B) / per_row, keep_pair_ms=ms["probes_keep"] + ms["dir_kept"],
                draw_pair_ms=ms["probes"] + ms["dir_draw"]))
        # the setting of tools/cw2_rate.py: the clean runner-up is the target, its clean score the threshold
        sc = e.system_scores(e.score_raw([x0])[0])[0]
        order = np.argsort(sc)
        target, thr = int(order[-2]), float(sc[order[-2]])
        start, where = None, None
        for seed in (1234, 99, 7, 2024):
            for u in range(1, 25):
                cand = synthetic_audio(u, n, seed)
                s = e.system_scores(e.score_raw([CP.cast_i16(cand, 16)])[0])[0]
                if start is None and int(np.argmax(s)) == target and s[target] >= thr:
                    start, where = cand, "synthetic_audio(%d, seed %d)" % (u, seed)
        # no synthetic voice is the target's own: the start is then MADE, by the white-box attack at a budget far above the one
        # it needs (the first successful iterate of fb_attack_wb at epsilon = 0.05, 0.02, 0.002) -- not what a decision-only
        # attacker has, but an audio that is decided as the target and lies far from the attacked one, which is all the walk asks
        for eps in (0.05, 0.02, 0.002):
            if start is None:
                _adv, flag, adv_f, _tr = e.attack_wb(nes_params("OSI", "targeted", max_iter=200, epsilon=eps, max_lr=eps / 2,
                                                                 target=target, threshold=thr, adver_thresh=0.01), audio)
                if flag == 1:
                    start, where = adv_f, "fb_attack_wb at epsilon %g" % eps
        if start is None:
            emit(what="result", target=target, threshold=thr, error="no start is decided as the target")
            return
        start_snr = snr_db(x0, CP.cast_i16(start, 16))
        p = lambda it: nes_params("OSI", "targeted", max_iter=it, target=target, threshold=thr, seed=42, stream=0)   # noqa: E731
        e.attack_hsj(p(2), hsj_params(), audio, start)                           # warm up: buffers, batch layouts
        res = e.attack_hsj(p(args.iters), hsj_params(), audio, start, keep_x=False)
        secs = e.attack_iter_seconds(res["trace"].shape[0])
        tr = res["trace"]
        rows_per_iter = np.diff(tr[:, 6])
        rows_mid = int(np.median(rows_per_iter)) if rows_per_iter.size else 0
        batch = [CP.cast_i16(synthetic_audio(2 + (j % 7), n), 16) for j in range(max(rows_mid, 1))]
        e.score_raw(batch)
        ts = []
        for _ in range(args.score_reps):
            t0 = time.perf_counter()
            e.score_raw(batch)
            ts.append(time.perf_counter() - t0)
        emit(what="host", iter_ms_median=1e3 * float(np.median(secs[1:])) if secs.size > 1 else None,
             start_search_ms=1e3 * float(secs[0]), rows_per_iter_median=rows_mid, score_call_same_rows_ms=1e3 * float(np.median(ts)),
             batches_per_iter_median=float(np.median(2 + tr[1:, 5])) if tr.shape[0] > 1 else None)
        # the distance is the float64 boundary point's; the SNR that counts is the returned int16 row's, so the attack is run
        # again with max_iter = t for the t at which the boundary point first passes --snr (an attack of t iterations is the
        # first t iterations of a longer one)
        sig = float(np.sum((x0.astype(np.float64) / 32768.0) ** 2))
        x_snr = [10.0 * math.log10(sig / d2) if d2 > 0 else float("inf") for d2 in tr[:, 0]]
        reach = next((t for t, v in enumerate(x_snr) if v >= args.snr), None)
        at = None
        if reach is not None:
            for t in range(reach, tr.shape[0]):
                r = e.attack_hsj(p(t), hsj_params(), audio, start)
                if snr_db(x0, r["adv"]) >= args.snr:
                    at = dict(iters=t, queries=int(r["n_queries"]), snr_db=snr_db(x0, r["adv"]),
                              linf_lsb=int(np.abs(r["adv"].astype(np.int32) - x0.astype(np.int32)).max()))
                    break
        emit(what="result", target=target, threshold=thr, start=where, start_snr_db=start_snr, first_boundary_dist=math.sqrt(tr[0, 0]),
             reaches_snr=at, iters=int(res["n_iters"]), queries=int(res["n_queries"]), stalls=int((tr[1:, 4] < 0).sum()),
             final_dist=math.sqrt(res["dist2"]), final_snr_db=snr_db(x0, res["adv"]),
             final_linf_lsb=int(np.abs(res["adv"].astype(np.int32) - x0.astype(np.int32)).max()),
             boundary_point_snr_db=[float("%.2f" % v) for v in x_snr])
    finally:
        e.close()


if __name__ == "__main__":
    main()
