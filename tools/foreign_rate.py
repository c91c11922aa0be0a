#!/usr/bin/env python
"""What a foreign victim adds to the swarm and the decision-only attacks (fb_attack_*_foreign), on the benchmark's shape: 3 s
of audio, batches of up to 1024 rows.

    python tools/foreign_rate.py [--samples 48000] [--rows 1024] [--reps 20] [--iters 30] [--repeat 3]

Prints JSON lines:
  what=kernels   --repeat times: milliseconds per launch (device events around --reps launches after one to warm up;
                 fb_bench_foreign_rows) and bytes per second of k_rows_to_model<float> (2 bytes read, 4 written per sample)
                 and k_rows_to_model<double> (2 read, 8 written), k_decide_foreign on rows x 5 scores, and, as the yardstick
                 of a pass that writes int16 rows, k_play_compose on the same rows (2 read, 2 written; fb_bench_play_compose)
                 in the same process.
  what=host_copy --repeat times: the two ways a host victim can get its rows, on the host's clock (one copy each after one
                 to warm up): the float64 rows copied device -> host (8 bytes per sample over the bus), and the int16 rows
                 copied (2 bytes per sample) and widened by one host thread.
  what=host      the host's median seconds per HopSkipJump iteration (fb_attack_iter_seconds) of fb_attack_hsj_foreign in
                 device mode around tests/foreign_models.TorchSynthModel (5 speakers, float32 batch), next to fb_attack_hsj
                 on the benchmark's GMM-UBM OSI system in the same process (tools/hsj_rate.py's setting), with the rows an
                 iteration scores and the model's own time per iteration (its score_device on as many rows, timed alone)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def emit(**kw):
    print(json.dumps(kw))
    sys.stdout.flush()


def native_hsj(e, n, iters):
    """tools/hsj_rate.py's attack on the benchmark system -> (median ms per iteration, median rows per iteration) or None"""
    from fakebob_amd import companions as CP
    from fakebob_amd.engine import hsj_params, nes_params
    from fakebob_amd.models import synthetic_audio
    audio = synthetic_audio(0, n)
    sc = e.system_scores(e.score_raw([CP.cast_i16(audio, 16)])[0])[0]
    order = np.argsort(sc)
    target, thr = int(order[-2]), float(sc[order[-2]])
    start = None
    for seed in (1234, 99, 7, 2024):
        for u in range(1, 25):
            cand = synthetic_audio(u, n, seed)
            s = e.system_scores(e.score_raw([CP.cast_i16(cand, 16)])[0])[0]
            if start is None and int(np.argmax(s)) == target and s[target] >= thr:
                start = cand
    for eps in (0.05, 0.02, 0.002):
        if start is None:
            _adv, flag, adv_f, _tr = e.attack_wb(nes_params("OSI", "targeted", max_iter=200, epsilon=eps, max_lr=eps / 2, target=target,
                                                             threshold=thr, adver_thresh=0.01), audio)
            if flag == 1:
                start = adv_f
    if start is None:
        return None
    p = lambda it: nes_params("OSI", "targeted", max_iter=it, target=target, threshold=thr, seed=42, stream=0)   # noqa: E731
    e.attack_hsj(p(2), hsj_params(), audio, start)                               # warm up: buffers, batch layouts
    res = e.attack_hsj(p(iters), hsj_params(), audio, start)
    secs = e.attack_iter_seconds(res["trace"].shape[0])
    return 1e3 * float(np.median(secs[1:])), float(np.median(np.diff(res["trace"][:, 6])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=48000)
    ap.add_argument("--rows", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--repeat", type=int, default=3)
    args = ap.parse_args()
    from fakebob_amd import _native
    torch = _native.torch_first()                                               # the model on the GPU and the engine share one HIP runtime
    from fakebob_amd import foreign as FG
    from fakebob_amd.engine import Engine, hsj_params, nes_params
    from fakebob_amd.models import synthetic_gmm_system
    from tests.foreign_models import TorchSynthModel
    from tests.golden.synth_model import synth_audio
    n, rows = args.samples, args.rows
    total = float(rows) * n
    e = Engine(0)
    try:
        for _ in range(args.repeat):
            ms = e.bench_foreign_rows(rows, n, S=5, reps=args.reps)
            play = e.bench_play_compose(rows, n, 1, reps=args.reps)
            emit(what="kernels", samples=n, rows=rows, rows_f32_ms=ms["rows_f32"], rows_f32_TBps=6.0 * total / ms["rows_f32"] * 1e-9,
                 rows_f32_write_TBps=4.0 * total / ms["rows_f32"] * 1e-9, rows_f64_ms=ms["rows_f64"],
                 rows_f64_TBps=10.0 * total / ms["rows_f64"] * 1e-9, rows_f64_write_TBps=8.0 * total / ms["rows_f64"] * 1e-9,
                 decide_ms=ms["decide"], play_compose_ms=play, play_compose_TBps=4.0 * total / play * 1e-9,
                 play_compose_write_TBps=2.0 * total / play * 1e-9)
            emit(what="host_copy", samples=n, rows=rows, d2h_f64_ms=ms["d2h_f64"], d2h_i16_widen_ms=ms["d2h_i16_widen"])
        # HopSkipJump in device mode around a torch model
        m = TorchSynthModel("OSI", 5, n, seed=2, device="cuda:0", device_dtype=torch.float32)
        a, i = synth_audio(n, 3), synth_audio(n, 4)
        sa, si = float(np.max(m.score(a))), float(np.max(m.score(i)))
        if si < sa:
            a, i, sa, si = i, a, si, sa
        thr = 0.5 * (sa + si)
        vic = FG.Victim("foreign_rate", "OSI", m, True)
        vic._engine = e
        spec = vic.spec(256, n, None, 16000, 16, 1, False)
        p = lambda it: nes_params("OSI", "untargeted", max_iter=it, true=-1, threshold=thr, seed=42, stream=0)   # noqa: E731
        e.attack_hsj_foreign(p(2), hsj_params(), spec, a, i)                     # warm up
        res = e.attack_hsj_foreign(p(args.iters), hsj_params(), spec, a, i)
        secs = e.attack_iter_seconds(res["trace"].shape[0])
        rows_mid = int(np.median(np.diff(res["trace"][:, 6]))) if res["trace"].shape[0] > 1 else 0
        batches = float(np.median(2 + res["trace"][1:, 5])) if res["trace"].shape[0] > 1 else 0.0
        x = spec["x"][:max(rows_mid, 1)]
        m.score_device(x)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(10):
            m.score_device(x)
        torch.cuda.synchronize()
        model_ms = 1e3 * (time.perf_counter() - t0) / 10
        foreign = dict(iter_ms_median=1e3 * float(np.median(secs[1:])) if secs.size > 1 else None, rows_per_iter_median=rows_mid,
                       batches_per_iter_median=batches, model_same_rows_one_call_ms=model_ms, success=int(res["success"]),
                       iters=int(res["n_iters"]), path=e.debug_foreign_path())
    finally:
        e.close()
    ubm, spk = synthetic_gmm_system(5, 2048, 72)
    e = Engine(0)
    try:
        e.set_frontend(mfcc_f32=1)
        e.load_gmm([ubm] + list(spk))
        e.set_system("OSI")
        e.set_fused_chain(True)                 # what a lone attack runs
        nat = native_hsj(e, n, args.iters)
    finally:
        e.close()
    emit(what="host", samples=n, foreign_device=foreign, native_iter_ms_median=None if nat is None else nat[0],
         native_rows_per_iter_median=None if nat is None else nat[1])


if __name__ == "__main__":
    main()
