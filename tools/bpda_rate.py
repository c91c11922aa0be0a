#!/usr/bin/env python
"""White-box iterations per second through a defended victim (fb_set_wb_bpda) on the benchmark's GMM-UBM OSI system (bench.py's
headline: 5 speakers + UBM, C = 2048, D = 72, float32 MFCC, 3 s of audio): one engine, one attack in flight, the stop
disabled by a large adver_thresh.

    python tools/bpda_rate.py [--iters 100] [--repeats 2]

Prints one JSON line per (repeat, case): iterations/s of fb_attack_wb over the whole call (wall clock around it, after a short
warm-up attack) with the mean and the median of the device's per-iteration times (fb_attack_iter_seconds).  Cases: the switch
off and on with no defence (the same launches: tools/whitebox_rate.py's figure), then with the switch on ms:7,qt:512, ds:2,
the ulaw codec alone, and noise:40 at EOT 1 and 4.  k_wb_chain_t's own time comes from a kernel trace of this script
(rocprofv3 --kernel-trace --stats -- python tools/bpda_rate.py --repeats 1), in a run of its own, not from here."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

#        name              switch  chain           codec   eot
CASES = [("undefended_off", False, None, None, 1),
         ("undefended_on", True, None, None, 1),
         ("ms7_qt512", True, "ms:7,qt:512", None, 1),
         ("ds2", True, "ds:2", None, 1),
         ("ulaw", True, None, "ulaw", 1),
         ("noise40_eot1", True, "noise:40", None, 1),
         ("noise40_eot4", True, "noise:40", None, 4)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=2)
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
        kw = dict(epsilon=0.002, adver_thresh=1e6, target=0, threshold=0.2277, seed=42, stream=0, samples_per_draw=0)

        def setup(on, chain, codec, eot):
            e.set_input_transform(chain)
            e.set_codec(codec)
            e.set_eot(eot)
            e.set_wb_bpda(on)
        for _name, on, chain, codec, eot in CASES:
            setup(on, chain, codec, eot)
            e.attack_wb(nes_params("OSI", "targeted", max_iter=5, **kw), audio)
        for rep in range(args.repeats):
            for name, on, chain, codec, eot in CASES:
                setup(on, chain, codec, eot)
                p = nes_params("OSI", "targeted", max_iter=args.iters, **kw)
                t0 = time.perf_counter()
                _adv, flag, _advf, trace = e.attack_wb(p, audio)
                dt = time.perf_counter() - t0
                secs = e.attack_iter_seconds(trace.shape[0])
                print(json.dumps(dict(case=name, repeat=rep, samples=args.samples, eot=eot, iterations=int(trace.shape[0]), flag=int(flag),
                                      iterations_per_s=trace.shape[0] / dt, ms_per_iteration=1e3 * dt / trace.shape[0],
                                      iter_ms_mean=1e3 * float(secs.mean()), iter_ms_median=1e3 * float(np.median(secs)),
                                      launches=e.debug_wb_route(), loss_first=float(trace[0, 1]), loss_last=float(trace[-1, 1]))))
    finally:
        e.close()


if __name__ == "__main__":
    main()
