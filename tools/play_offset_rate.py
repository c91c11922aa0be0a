#!/usr/bin/env python
"""What the play offset costs and what it buys, on the benchmark's GMM-UBM OSI system (bench.py's headline: 5 speakers + UBM,
C = 2048, D = 72, float32 MFCC, 3 s of audio).

    python tools/play_offset_rate.py [--samples 48000] [--reps 20] [--iters 8] [--steps 30] [--nes-iters 200]

Prints JSON lines:
  what=k_play_compose  milliseconds per launch of k_play_compose alone (device events around --reps launches;
                       fb_bench_play_compose) for a 1031-row batch at r' = 1, 8 and 32 (K = 1) and at K = 4, eot = 8 (three
                       companions), and the write bandwidth it reaches (B * r' * N * 2 bytes per launch).
  what=nes             the median seconds per iteration of fb_attack (fb_attack_iter_seconds; samples_per_draw 50, eot 8) with
                       S = N - 1 against S = 0, the same engine, the same process.
  what=pgd             the same for fb_attack_wb (fb_set_wb_universal, fb_set_wb_bpda, eot 8).
  what=buys            --steps PGD sign steps at eot 8, once trained with S = N - 1 and once with S = 0, both judged by the mean
                       loss over 16 held-out epochs of offsets (S = N - 1, eot 8: 128 offsets each): what training under the
                       offset buys when the playback timing is unknown.  Also the loss of the unperturbed audio.
  what=per_offset      one NES attack (FakeBob, --nes-iters iterations, eot 8) trained with the offset and one trained without
                       it: of the 16 offsets of play_offset.offset_grid(N - 1), how many still succeed (the system's ordinary
                       make_decisions on the composed audio).  The attack is untargeted on the voice the system rejects by the
                       widest margin, the threshold a quarter of the way towards the best-accepted voice."""
import argparse
import json
import os
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def emit(**kw):
    print(json.dumps(kw))
    sys.stdout.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=48000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--iters", type=int, default=8)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--nes-iters", dest="nes_iters", type=int, default=200)
    args = ap.parse_args()
    from fakebob_amd import companions as CP, play_offset as PO
    from fakebob_amd.attack import FakeBob
    from fakebob_amd.engine import nes_params
    from fakebob_amd.models import synthetic_audio, synthetic_gmm_system
    from fakebob_amd.systems import gmm_OSI
    ubm, spk = synthetic_gmm_system(5, 2048, 72)
    n = args.samples
    tmp = tempfile.mkdtemp(prefix="play_offset_rate_")
    ml = [["spk%d" % i, "utt%d" % i, g, 0.0, 1.0] for i, g in enumerate(spk)]
    model = gmm_OSI(os.path.join(tmp, "osi"), ml, ubm, pre_model_dir=tmp, threshold=0.0, mfcc_f32=1)
    e = model.engine
    try:
        e.set_fused_chain(True)                 # what a lone attack runs
        for K, eot in ((1, 1), (1, 8), (1, 32), (4, 8)):      # (the last: three companions re-read by every row, out of L2)
            ms = e.bench_play_compose(1031, n, eot, reps=args.reps, K=K)
            emit(what="k_play_compose", rows=1031, utterances=K, eot=eot, replicas=K * eot, samples=n, ms=ms,
                 write_GBps=1031 * K * eot * n * 2 / (ms * 1e-3) / 1e9)
        voices = [synthetic_audio(u, n) for u in range(8)]
        sc = e.system_scores(e.score_raw([CP.cast_i16(v, 16) for v in voices])[0])
        best = sc.max(axis=1)
        lo, hi = int(np.argmin(best)), int(np.argmax(best))
        thr = float(best[lo] + 0.25 * (best[hi] - best[lo]))
        audio = voices[lo]
        S = n - 1
        e.set_eot(8)
        # the cost of an iteration: no early stop (adver_thresh 1e3)
        for name in ("nes", "pgd"):
            out = {}
            e.set_wb_universal(name == "pgd")
            e.set_wb_bpda(name == "pgd")
            for s in (0, S, 0, S):              # (twice each: the first pair warms up buffers and batch layouts)
                e.set_play_offset(s)
                p = nes_params("OSI", "untargeted", samples_per_draw=50 if name == "nes" else 0, max_iter=args.iters, threshold=thr,
                               adver_thresh=1e3, seed=42, stream=0)
                rows = (e.attack(p, audio) if name == "nes" else e.attack_wb(p, audio))[3].shape[0]
                out[s] = dict(iter_ms_median=1e3 * float(np.median(e.attack_iter_seconds(rows))), iters=int(rows))
            e.set_play_offset(0)
            emit(what=name, samples=n, eot=8, S0=out[0], Smax=out[S], ratio=out[S]["iter_ms_median"] / out[0]["iter_ms_median"])
        # what it buys: PGD sign steps, judged over held-out offsets
        e.set_wb_universal(True)
        e.set_wb_bpda(True)
        judged = {}
        p = nes_params("OSI", "untargeted", samples_per_draw=0, max_iter=args.steps, threshold=thr, adver_thresh=1e3, seed=42, stream=0)
        pj = nes_params("OSI", "untargeted", samples_per_draw=0, threshold=thr, adver_thresh=0.0, seed=4242, stream=9)

        def held_out(x):
            e.set_play_offset(S)
            try:
                return float(np.mean([e.get_grad_wb_from(pj, x, audio, 1000 + k, want_grad=False)[1] for k in range(16)]))
            finally:
                e.set_play_offset(0)
        for s in (S, 0):
            e.set_play_offset(s)
            adv_f = e.attack_wb(p, audio)[2]
            e.set_play_offset(0)
            judged[s] = held_out(adv_f)
        emit(what="buys", samples=n, eot=8, steps=args.steps, threshold=thr, clean_loss=held_out(audio), trained_with_offset=judged[S],
             trained_without=judged[0])
        e.set_wb_universal(False)
        e.set_wb_bpda(False)
        # per_offset of one NES attack trained either way
        model.threshold = thr
        grid = PO.offset_grid(S)
        counts = {}
        for s in (S, 0):
            fb = FakeBob("OSI", "untargeted", model, samples_per_draw=50, max_iter=args.nes_iters, seed=42, verbose=False, eot_size=8,
                         play_offset=s if s else None)
            res = fb.attack(audio, None, threshold=thr)
            if s:
                ok = res.per_offset[0]["successes"]
            else:
                ok = [CP.succeeded("OSI", "untargeted", model.make_decisions(PO.compose(CP.cast_i16(audio), res.perturbation_i16, t))[0]) for t in grid]
            counts[s] = dict(flag=int(res[1]), n_success=int(sum(ok)), successes=[int(b) for b in ok])
        emit(what="per_offset", samples=n, eot=8, nes_iters=args.nes_iters, grid=grid, trained_with_offset=counts[S], trained_without=counts[0])
    finally:
        e.close()
        import shutil
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
