#!/usr/bin/env python
"""What fb_attack_psy costs and what it buys, on the benchmark's GMM-UBM OSI system (bench.py's headline: 5 speakers + UBM,
C = 2048, D = 72, float32 MFCC, 3 s of audio): one engine, one attack in flight.

    python tools/psy_rate.py [--iters 100] [--windows 5] [--search-iters 200] [--window 2048] [--l2-weight 0] [--trace-only]

Prints one JSON line per measurement:
  rate      the median over --windows attacks of the median device time per iteration (fb_attack_iter_seconds) of
            fb_attack_psy -- one search step of --iters iterations, the abort rule off -- and of fb_attack_cw2 with the same
            parameters, in the same process, one after the other in every window
  result    same audio, same target (the clean runner-up), same threshold (its clean score), same search: for CW2's best iterate
            and for this attack's the masking distortion D, the share n_over / (F K) of bins above the threshold (both by
            fakebob_amd.masking.masking_loss on adver_f64 - audio), |delta|^2 in float audio units and the SNR of the int16
            perturbation
The time of k_psy_frames, k_psy_ctl and k_psy_step alone comes from a kernel trace of this script in a run of its own, the
program after the `--`:
    rocprofv3 --kernel-trace --stats -- python tools/psy_rate.py --trace-only
(--trace-only: a warm-up and one attack of --iters iterations, nothing else)."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--samples", type=int, default=48000)
    ap.add_argument("--search-iters", dest="search_iters", type=int, default=200)
    ap.add_argument("--window", type=int, default=2048)
    ap.add_argument("--l2-weight", dest="l2_weight", type=float, default=0.0)
    ap.add_argument("--trace-only", action="store_true")
    args = ap.parse_args()
    from fakebob_amd.cw2 import snr_db
    from fakebob_amd.companions import cast_i16
    from fakebob_amd.engine import Engine, cw2_params, nes_params, psy_params
    from fakebob_amd.masking import masking_loss, masking_threshold
    from fakebob_amd.models import synthetic_audio, synthetic_gmm_system

    def emit(**rec):
        print(json.dumps(rec), flush=True)

    audio = synthetic_audio(0, args.samples)
    a0 = cast_i16(audio, 16)
    one_step = cw2_params(search_steps=1, abort_every=0)
    ubm, spk = synthetic_gmm_system(5, 2048, 72)
    e = Engine(0)
    try:
        e.set_frontend(mfcc_f32=1)
        e.load_gmm([ubm] + list(spk))
        e.set_system("OSI")
        e.set_fused_chain(True)                 # what a lone attack runs
        theta, psd_max = masking_threshold(audio, float(e.cfg.sample_freq), args.window)
        m = psy_params(theta, psd_max, args.window, args.l2_weight)
        never = dict(adver_thresh=1e6, threshold=1.0)
        p = nes_params("OSI", "targeted", max_iter=args.iters, samples_per_draw=0, **never)
        warm = nes_params("OSI", "targeted", max_iter=5, samples_per_draw=0, **never)
        e.attack_psy(warm, one_step, m, audio)
        e.attack_cw2(warm, one_step, audio)
        if args.trace_only:
            e.attack_psy(p, one_step, m, audio)
            return
        ps, cw = [], []
        for _ in range(args.windows):
            res = e.attack_psy(p, one_step, m, audio)
            ps.append(1e3 * float(np.median(e.attack_iter_seconds(res["trace"].shape[0]))))
            res = e.attack_cw2(p, one_step, audio)
            cw.append(1e3 * float(np.median(e.attack_iter_seconds(res["trace"].shape[0]))))
        emit(what="rate", system="gmm_ubm_osi", samples=args.samples, window=args.window, frames=int(theta.shape[0]),
             iterations=args.iters, windows=args.windows, psy_iter_ms=float(np.median(ps)), psy_iter_ms_windows=ps,
             cw2_iter_ms=float(np.median(cw)), cw2_iter_ms_windows=cw, added_us=1e3 * (float(np.median(ps)) - float(np.median(cw))))
        _g, _al, sc = e.get_grad_wb(nes_params("OSI", "targeted", target=0, samples_per_draw=0), audio)
        order = np.argsort(sc[:5])
        target, thr = int(order[-2]), float(sc[order[-2]])
        goal = nes_params("OSI", "targeted", max_iter=args.search_iters, samples_per_draw=0, target=target, threshold=thr)
        fk = float(theta.size)
        for name, res in (("cw2", e.attack_cw2(goal, cw2_params(), audio)), ("psy", e.attack_psy(goal, cw2_params(), m, audio))):
            d = res["adv"].astype(np.int32) - a0
            D, n_over, _P = masking_loss(res["adver_f64"] - audio, theta, psd_max, args.window)
            emit(what="result", attack=name, target=target, threshold=thr, search_iters=args.search_iters,
                 rows_per_step=[int(v) for v in res["rows_per_step"]], success=int(res["success"]), D=D, n_over=n_over,
                 over_share=n_over / fk, l2=float(np.sum((res["adver_f64"] - audio) ** 2)), snr_db=snr_db(a0, d),
                 linf_lsb=int(np.abs(d).max()), const=float(res["const"]))
    finally:
        e.close()


if __name__ == "__main__":
    main()
