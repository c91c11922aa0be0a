#!/usr/bin/env python
"""What fb_attack_cw2 costs and what it buys, on the benchmark's GMM-UBM OSI system (bench.py's headline: 5 speakers + UBM,
C = 2048, D = 72, float32 MFCC, 3 s of audio) and on its i-vector SV system (C = 2048, D = 72, R = 400, LDA 200, one enrolled
speaker, under fb_set_wb_ivector): one engine, one attack in flight.

    python tools/cw2_rate.py [--iters 100] [--windows 5] [--search-iters 200] [--trace-only]

Prints one JSON line per measurement:
  rate      per system: the median over --windows attacks of the median device time per iteration (fb_attack_iter_seconds: the
            device's constant-rate clock, stamped by the control launch of every iteration) of fb_attack_cw2 -- one search step of
            --iters iterations, the abort rule off -- and of fb_attack_wb with its stop out of reach, in the same process, one
            after the other in every window
  result    on the GMM-UBM system: the squared L2 distance (float audio units) and the SNR of the int16 perturbation of CW2's
            result at its defaults with max_iter = --search-iters per search step, and of PGD's first successful iterate
            (fb_attack_wb at its defaults) from the same audio; the target is the clean runner-up, the threshold its clean score
The time of k_cw2_step and k_cw2_ctl alone comes from a kernel trace of this script in a run of its own, the program after
the `--`:
    rocprofv3 --kernel-trace --stats -- python tools/cw2_rate.py --trace-only
(--trace-only: a warm-up and one GMM-UBM attack of --iters iterations, nothing else)."""
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
    ap.add_argument("--trace-only", action="store_true")
    args = ap.parse_args()
    from fakebob_amd.cw2 import snr_db
    from fakebob_amd.companions import cast_i16
    from fakebob_amd.engine import Engine, cw2_params, nes_params
    from fakebob_amd.models import synthetic_audio, synthetic_gmm_system, synthetic_ivector_system

    def emit(**rec):
        print(json.dumps(rec), flush=True)

    audio = synthetic_audio(0, args.samples)
    a0 = cast_i16(audio, 16)
    one_step = cw2_params(search_steps=1, abort_every=0)

    def rate(e, name, task, kind):
        never = dict(adver_thresh=1e6, threshold=1.0)
        p = nes_params(task, "targeted", max_iter=args.iters, samples_per_draw=0, **never)
        e.attack_cw2(nes_params(task, "targeted", max_iter=5, samples_per_draw=0, **never), one_step, audio)
        e.attack_wb(nes_params(task, "targeted", max_iter=5, **never), audio)
        if args.trace_only:
            e.attack_cw2(p, one_step, audio)
            return
        cw, wb = [], []
        for _ in range(args.windows):
            res = e.attack_cw2(p, one_step, audio)
            cw.append(1e3 * float(np.median(e.attack_iter_seconds(res["trace"].shape[0]))))
            launches = e.debug_wb_route()
            trace = e.attack_wb(p, audio)[3]
            wb.append(1e3 * float(np.median(e.attack_iter_seconds(trace.shape[0]))))
        emit(what="rate", system=name, samples=args.samples, iterations=args.iters, windows=args.windows,
             cw2_iter_ms=float(np.median(cw)), cw2_iter_ms_windows=cw, wb_iter_ms=float(np.median(wb)), wb_iter_ms_windows=wb,
             added_us=1e3 * (float(np.median(cw)) - float(np.median(wb))), launches=launches)

    ubm, spk = synthetic_gmm_system(5, 2048, 72)
    e = Engine(0)
    try:
        e.set_frontend(mfcc_f32=1)
        e.load_gmm([ubm] + list(spk))
        e.set_system("OSI")
        e.set_fused_chain(True)                 # what a lone attack runs
        rate(e, "gmm_ubm_osi", "OSI", "gmm")
        if not args.trace_only:
            _g, _al, sc = e.get_grad_wb(nes_params("OSI", "targeted", target=0, samples_per_draw=0), audio)
            order = np.argsort(sc[:5])
            target, thr = int(order[-2]), float(sc[order[-2]])
            goal = dict(target=target, threshold=thr)
            res = e.attack_cw2(nes_params("OSI", "targeted", max_iter=args.search_iters, samples_per_draw=0, **goal), cw2_params(), audio)
            d = res["adv"].astype(np.int32) - a0
            ok = res["trace"][:, 1] < 0
            emit(what="result", attack="cw2", target=target, threshold=thr, clean_scores=[float(v) for v in sc[:5]],
                 search_iters=args.search_iters, rows_per_step=[int(v) for v in res["rows_per_step"]], success=int(res["success"]),
                 l2=float(res["best_l2"]), snr_db=snr_db(a0, d), linf_lsb=int(np.abs(d).max()), const=float(res["const"]),
                 successful_rows=int(ok.sum()), rows=int(ok.size))
            adv, flag, adv_f, trace = e.attack_wb(nes_params("OSI", "targeted", max_iter=1000, **goal), audio)
            d = adv.astype(np.int32) - a0
            emit(what="result", attack="pgd_first_success", success=int(flag), iterations=int(trace.shape[0]),
                 l2=float(np.sum((adv_f - audio) ** 2)), snr_db=snr_db(a0, d), linf_lsb=int(np.abs(d).max()))
    finally:
        e.close()
    if args.trace_only:
        return
    sy = synthetic_ivector_system(C=2048, D=72, R=400, L=200, n_speakers=1)
    sy = sy.with_enrolled(sy.enrolled, [-40.0], [10.0])
    e = Engine(0)
    try:
        e.set_frontend(mfcc_f32=1)
        e.load_ivector(sy, "SV")
        e.set_fused_chain(True)
        e.set_wb_ivector(True)
        rate(e, "ivector_sv", "SV", "iv")
    finally:
        e.close()


if __name__ == "__main__":
    main()
