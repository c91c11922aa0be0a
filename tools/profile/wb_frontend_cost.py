"""What the white-box gradient through feature compression and dither costs (fb_set_wb_frontend): ms per fb_attack_wb iteration,
wall clock around the call (it ends in a device synchronise) after a warm-up attack of the same shape, the stop disabled.
  gmm   the headline GMM-UBM OSI system -- UBM + 5 speakers, C = 2048, D = 72, k_mfcc_f32, 3 s at 16 kHz -- under fb_set_wb_bpda at
        EOT 1 and 8: no stage, FeCo 0.5:10, dither 1.0, no stage again (the spread)
  iv    the benchmark's i-vector SV system (C = 2048, R = 400, LDA 200, one speaker) at r = 1: no stage, FeCo 0.5:10, no stage again
  trace (for a kernel trace, tools/profile/wb_frontend_cost.sh) the GMM system at r = 1 only: no stage, dither 1.0, FeCo 0.5:10,
        `steps` iterations each after `warmup`
Prints one JSON line."""
import json
import sys
import time

from fakebob_amd.engine import Engine, nes_params
from fakebob_amd.models import synthetic_audio, synthetic_gmm_system, synthetic_ivector_system

SAMPLES = 48000
STAGES = [("none", None, 0.0), ("feco 0.5:10", 0.5, 0.0), ("dither 1.0", None, 1.0), ("none again", None, 0.0)]


def _time(e, task, r, ratio, dither, steps, warmup, audio, **kw):
    e.set_eot(r)
    e.set_feature_compression(ratio, 10) if ratio else e.set_feature_compression(None)
    e.set_frontend(dither=dither)
    p = nes_params(task, "targeted", epsilon=0.002, max_lr=0.001, min_lr=1e-6, momentum=0.9, threshold=1e3, adver_thresh=1e6,
                   seed=42, max_iter=warmup, **kw)     # (adver_thresh: never stops early)
    e.attack_wb(p, audio)
    p.max_iter = steps
    t0 = time.perf_counter()
    _adv, _flag, _f, trace = e.attack_wb(p, audio)
    dt = time.perf_counter() - t0
    return dict(ms_per_iter=1e3 * dt / trace.shape[0], iters=int(trace.shape[0]), feco_launches=e.debug_wb_feco_route())


def main(mode="all", steps=100, warmup=4):
    steps, warmup = int(steps), int(warmup)
    out = {"mode": mode, "steps": steps, "warmup": warmup, "samples": SAMPLES}
    audio = synthetic_audio(0, SAMPLES)
    e = Engine(0)
    try:
        e.set_frontend(mfcc_f32=1)
        e.set_wb_bpda(True)
        e.set_wb_ivector(True)
        e.set_wb_frontend(True)
        if mode in ("all", "gmm", "trace"):
            ubm, spk = synthetic_gmm_system(n_speakers=5, C=2048, D=72)
            e.load_gmm([ubm] + spk)
            e.set_system("OSI")
            if mode == "trace":
                for name, ratio, dither in (STAGES[0], STAGES[2], STAGES[1]):
                    out["gmm eot=1 " + name] = _time(e, "OSI", 1, ratio, dither, steps, warmup, audio, target=1)
            else:
                for r in (1, 8):
                    for name, ratio, dither in STAGES:
                        out["gmm eot=%d %s" % (r, name)] = _time(e, "OSI", r, ratio, dither, max(steps // r, 10), warmup, audio, target=1)
        if mode in ("all", "iv"):
            sy = synthetic_ivector_system(C=2048, D=72, R=400, L=200, n_speakers=1)
            sy = sy.with_enrolled(sy.enrolled, [-40.0], [10.0])
            e.load_ivector(sy, "SV")
            e.set_fused_chain(True)             # what a lone attack runs
            for name, ratio, dither in (STAGES[0], STAGES[1], STAGES[3]):
                out["iv eot=1 " + name] = _time(e, "SV", 1, ratio, dither, steps, warmup, audio)
    finally:
        e.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main(*sys.argv[1:4])
