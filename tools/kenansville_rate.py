#!/usr/bin/env python
"""What a round of the decision-only attack costs on the benchmark's GMM-UBM OSI system (bench.py's headline: 5 speakers +
UBM, C = 2048, D = 72, float32 MFCC, 3 s of audio) at the default search: W = 100, G = 15.

    python tools/kenansville_rate.py [--samples 48000] [--window 100] [--grid 15] [--reps 200]

Prints one JSON line with three times, in milliseconds:
  analyse_ms      one k_kv_analyse launch (once per attack): device events around --reps launches
  candidates_ms   one k_kv_candidates launch of G rows (once per round): likewise
  score_ms        a scoring call of the same G rows (fb_score_i16: the copy of the rows, the front end, the GMM, one
                  synchronisation): host clock, median of --score-reps calls after a warm-up
and, for the whole thing, the host's median time per round of an attack that runs --rounds rounds (fb_attack_iter_seconds:
candidates, scoring, k_loss and the look)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=48000)
    ap.add_argument("--window", type=int, default=100)
    ap.add_argument("--grid", type=int, default=15)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--score-reps", dest="score_reps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=8)
    args = ap.parse_args()
    from fakebob_amd import companions as CP
    from fakebob_amd import kenansville as KV
    from fakebob_amd.engine import Engine, kv_params, nes_params
    from fakebob_amd.models import synthetic_audio, synthetic_gmm_system
    ubm, spk = synthetic_gmm_system(5, 2048, 72)
    e = Engine(0)
    try:
        e.set_frontend(mfcc_f32=1)
        e.load_gmm([ubm] + list(spk))
        e.set_system("OSI")
        e.set_fused_chain(True)                 # what a lone attack runs
        audio = synthetic_audio(0, args.samples)
        x = CP.cast_i16(audio, 16)
        G, W = args.grid, args.window
        qs = [((j + 1) * 32768) // G for j in range(G)]                # up to half of every window's energy: all rows voiced
        analyse_ms, cand_ms = e.bench_kv_kernels(x, W, qs, reps=args.reps)
        rows = list(e.debug_kv_candidates(x, W, qs))
        assert np.array_equal(rows[-1], KV.remove(x, W, qs[-1]))       # what is timed is what the contract says
        e.score_raw(rows)
        ts = []
        for _ in range(args.score_reps):
            t0 = time.perf_counter()
            e.score_raw(rows)
            ts.append(time.perf_counter() - t0)
        # one round in which nothing succeeds: no voice is accepted under this threshold, so none is decided to be speaker 0
        p = nes_params("OSI", "targeted", target=0, threshold=1e9, seed=42, stream=0)
        e.attack_kenansville(p, kv_params(W, G, 32768, 1), audio)
        t0 = time.perf_counter()
        res = e.attack_kenansville(p, kv_params(W, G, 32768, 1), audio)
        one = time.perf_counter() - t0
        # a search that goes on: the goal is rejection itself, which every candidate meets, so the bracket narrows towards 1
        p = nes_params("OSI", "targeted", target=-1, threshold=1e9, seed=42, stream=0)
        res = e.attack_kenansville(p, kv_params(W, G, 32768, args.rounds), audio)
        secs = e.attack_iter_seconds(res["trace"].shape[0])
        print(json.dumps(dict(samples=args.samples, window=W, grid=G, analyse_ms=analyse_ms, candidates_ms=cand_ms,
                              score_ms=1e3 * float(np.median(ts)), score_ms_min=1e3 * float(min(ts)),
                              one_round_attack_ms=1e3 * one, rounds=int(res["trace"].shape[0]),
                              round_ms_median=1e3 * float(np.median(secs)), queries=int(res["n_queries"]))))
    finally:
        e.close()


if __name__ == "__main__":
    main()
