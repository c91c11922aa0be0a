"""What the white-box gradient of a universal perturbation costs (fb_set_wb_universal): ms per fb_attack_wb iteration, wall clock
around the call (it ends in a device synchronise) after a warm-up attack of the same shape, the stop disabled.
  gmm   the headline GMM-UBM OSI system -- UBM + 5 speakers, C = 2048, D = 72, k_mfcc_f32, 3 s at 16 kHz -- under fb_set_wb_bpda:
        the single row (K = 1, eot 1), K = 4 at eot 1 and 8, the single row again (the spread)
  iv    the benchmark's i-vector SV system (C = 2048, R = 400, LDA 200, one speaker): the single row, K = 4, the single row again
  hook  (for a kernel trace, tools/profile/wb_universal_cost.sh) k_wb_compose_t alone through fb_debug_wb_compose_t at N = 48 000:
        R = 8 (K = 4, eot 2) and R = 32 (K = 32, eot 1), `steps` launches each
Prints one JSON line."""
import json
import sys
import time

import numpy as np

from fakebob_amd.engine import Engine, nes_params
from fakebob_amd.models import synthetic_audio, synthetic_gmm_system, synthetic_ivector_system

SAMPLES = 48000


def _time(e, task, K1, r, steps, warmup, audio, **kw):
    e.set_companions(None)
    e.set_eot(r)
    e.set_companions([synthetic_audio(u, SAMPLES) for u in range(1, K1 + 1)] if K1 else None)
    p = nes_params(task, "targeted", epsilon=0.002, max_lr=0.001, min_lr=1e-6, momentum=0.9, threshold=1e3, adver_thresh=1e6,
                   seed=42, max_iter=warmup, **kw)     # (adver_thresh: never stops early)
    e.attack_wb(p, audio)
    p.max_iter = steps
    t0 = time.perf_counter()
    _adv, _flag, _f, trace = e.attack_wb(p, audio)
    dt = time.perf_counter() - t0
    return dict(ms_per_iter=1e3 * dt / trace.shape[0], iters=int(trace.shape[0]), replicas=(K1 + 1) * r,
                compose_t_launches=e.debug_wb_universal_route())


def main(mode="all", steps=100, warmup=4):
    steps, warmup = int(steps), int(warmup)
    out = {"mode": mode, "steps": steps, "warmup": warmup, "samples": SAMPLES}
    audio = synthetic_audio(0, SAMPLES)
    e = Engine(0)
    try:
        if mode == "hook":
            rng = np.random.RandomState(1)
            q = (audio * 32768.0).astype(np.int16)
            for K, eot in ((4, 2), (32, 1)):
                cot = rng.standard_normal((K * eot, SAMPLES))
                comp = rng.randint(-32768, 32768, (K - 1, SAMPLES)).astype(np.int16)
                for _ in range(steps):
                    e.debug_wb_compose_t(cot, q, q, comp, eot)
            print(json.dumps(out))
            return
        e.set_frontend(mfcc_f32=1)
        e.set_wb_bpda(True)
        e.set_wb_ivector(True)
        e.set_wb_universal(True)
        if mode in ("all", "gmm"):
            ubm, spk = synthetic_gmm_system(n_speakers=5, C=2048, D=72)
            e.load_gmm([ubm] + spk)
            e.set_system("OSI")
            for name, K1, r in (("K=1 eot=1", 0, 1), ("K=4 eot=1", 3, 1), ("K=4 eot=8", 3, 8), ("K=1 eot=1 again", 0, 1)):
                out["gmm " + name] = _time(e, "OSI", K1, r, max(steps // ((K1 + 1) * r), 10), warmup, audio, target=1)
        if mode in ("all", "iv"):
            sy = synthetic_ivector_system(C=2048, D=72, R=400, L=200, n_speakers=1)
            sy = sy.with_enrolled(sy.enrolled, [-40.0], [10.0])
            e.load_ivector(sy, "SV")
            e.set_fused_chain(True)             # what a lone attack runs
            for name, K1 in (("K=1", 0), ("K=4", 3), ("K=1 again", 0)):
                out["iv eot=1 " + name] = _time(e, "SV", K1, 1, max(steps // (K1 + 1), 10), warmup, audio)
    finally:
        e.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main(*sys.argv[1:4])
