#!/usr/bin/env python
"""What voted decisions cost on the benchmark's GMM-UBM OSI system (bench.py's headline: 5 speakers + UBM, C = 2048, D = 72,
float32 MFCC, 3 s of audio) behind a randomised victim (the noise stage at:20).

    python tools/query_eot_rate.py [--samples 48000] [--reps 50] [--iters 6]

Prints JSON lines:
  what=k_vote    milliseconds per launch of k_vote alone at 1024 candidate rows x 8 replicas (device events around --reps
                 launches; fb_bench_vote), on raw scores of the system's own width.
  what=hsj       the host's median seconds per HopSkipJump iteration (fb_attack_iter_seconds) at r' = 1 (the switch off) and
                 at r' = 8 (fb_set_eot(8), majority quorum), with the victim queries per iteration: the ratio is what a vote of
                 eight costs.  The attack is untargeted from a voice the system accepts towards one it rejects.
  what=pso       the same for an iteration of a swarm of 25 particles."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def emit(**kw):
    print(json.dumps(kw))
    sys.stdout.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=48000)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--iters", type=int, default=6)
    args = ap.parse_args()
    from fakebob_amd import companions as CP
    from fakebob_amd.engine import Engine, hsj_params, nes_params, pso_params
    from fakebob_amd.models import synthetic_audio, synthetic_gmm_system
    ubm, spk = synthetic_gmm_system(5, 2048, 72)
    n = args.samples
    e = Engine(0)
    try:
        e.set_frontend(mfcc_f32=1)
        e.load_gmm([ubm] + list(spk))
        e.set_system("OSI")
        e.set_fused_chain(True)                 # what a lone attack runs
        e.set_input_transform("at:20")
        S = e.n_speakers
        # k_vote alone: 1024 x 8 replica rows of plausible raw scores, a threshold in their middle
        rng = np.random.RandomState(1)
        raw = rng.normal(-80.0, 3.0, (1024, 8, S + 1))
        tv = np.full(1024 * 8, 200, np.int32)
        ms = e.bench_vote(raw, tv, "OSI", 0.0, "untargeted", -1, reps=args.reps)
        emit(what="k_vote", rows=1024, replicas=8, speakers=S, ms=ms)
        # the two voices whose best scores lie furthest apart, the threshold half way: the lower one is rejected and attacked
        voices = [synthetic_audio(u, n) for u in range(8)]
        sc = e.system_scores(e.score_raw([CP.cast_i16(v, 16) for v in voices])[0])
        best = sc.max(axis=1)
        lo, hi = int(np.argmin(best)), int(np.argmax(best))
        thr = 0.5 * float(best[lo] + best[hi])
        audio, init = voices[lo], voices[hi]
        for name in ("hsj", "pso"):
            out = {}
            for eot in (1, 8):
                e.set_query_eot("majority" if eot > 1 else None)
                e.set_eot(eot)
                try:
                    for it in (1, args.iters):       # the first run warms up: buffers, batch layouts
                        if name == "hsj":
                            p = nes_params("OSI", "untargeted", max_iter=it, true=-1, threshold=thr, seed=42, stream=0)
                            res = e.attack_hsj(p, hsj_params(), audio, init)
                            rows, queries = res["trace"].shape[0], res["n_queries"]
                        else:
                            p = nes_params("OSI", "untargeted", max_iter=it, threshold=thr, adver_thresh=1e3, seed=42, stream=0)
                            trace = e.attack_pso(p, pso_params(25), audio)[3]
                            rows, queries = trace.shape[0], 25 * eot * trace.shape[0]
                    secs = e.attack_iter_seconds(rows)
                    skip = 1 if name == "hsj" and rows > 1 else 0       # (HopSkipJump's entry 0 is the start search)
                    out[eot] = dict(iter_ms_median=1e3 * float(np.median(secs[skip:])), iters=int(rows - skip), queries=int(queries))
                finally:
                    e.set_eot(1)
                    e.set_query_eot(None)
            emit(what=name, samples=n, r1=out[1], r8=out[8], ratio=out[8]["iter_ms_median"] / out[1]["iter_ms_median"])
    finally:
        e.close()


if __name__ == "__main__":
    main()
