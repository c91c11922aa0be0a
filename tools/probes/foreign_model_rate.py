"""NES iterations/s of the plugin API with a float32 model on the GPU: the host path (fb_attack_ext: the batch copied to
the host, the model's score on a numpy batch, the scores copied back) against the device path (fb_attack_dev:
batch and scores stay in device memory) at look_every = 1 and 4.

The model is tests/foreign_models.py's FrameModel (framing by unfold, matmul, log, mean), samples_per_draw = 50, 3 s of
16 kHz audio, OSI untargeted with a loss that never turns negative (every iteration runs).  Each leg runs in a child
process of its own under `timeout -k 10`.

    python tools/probes/foreign_model_rate.py [--iters 200] [--warmup 20] [--timeout 300]

Prints one JSON line per leg and a summary line."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
LEGS = (("host", 0), ("device", 1), ("device", 4))


def leg(path, look_every, iters, warmup):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch  # noqa: F401  (before the library: one HIP runtime)
    from fakebob_amd.attack import FakeBob
    from fakebob_amd.engine import nes_params
    from tests.foreign_models import FrameModel, ScoreOnly
    from tests.golden.synth_model import synth_audio

    n, spd, S = 48000, 50, 8
    model = FrameModel("OSI", S, "cuda:0", seed=1)
    host = ScoreOnly(model)
    audio = synth_audio(n, 1)
    fb = FakeBob("OSI", "untargeted", model if path == "device" else host, samples_per_draw=spd, verbose=False)
    eng = fb._engine()

    def run(k):
        p = nes_params("OSI", "untargeted", adver_thresh=1e6, max_iter=k, samples_per_draw=spd, threshold=0.0, seed=3)
        if path == "device":
            x, sc = fb._device_buffers(n, S)
            r = eng.attack_dev(p, S, model.score_device, x, sc, audio, look_every=look_every)
        else:
            r = eng.attack_ext(p, S, fb._score_fn(16000, 16, 1, False), audio)
        return r[3].shape[0]

    run(warmup)
    t0 = time.perf_counter()
    rows = run(iters)
    dt = time.perf_counter() - t0
    info = eng.debug_foreign_path()
    return dict(path=path, look_every=look_every if path == "device" else None, iters=rows, seconds=dt,
                it_per_s=rows / dt, ms_per_iter=1e3 * dt / rows, launches_per_iter=info["launches_per_iter"],
                batch_bytes_d2h_per_iter=info["batch_bytes_d2h"] // max(info["model_calls"], 1),
                score_bytes_h2d_per_iter=info["score_bytes_h2d"] // max(info["model_calls"], 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--timeout", type=int, default=300, help="seconds per leg")
    ap.add_argument("--leg", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.leg:
        path, le = a.leg.split(":")
        print(json.dumps(leg(path, int(le), a.iters, a.warmup)))
        return 0
    res = []
    for path, le in LEGS:
        cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--leg", "%s:%d" % (path, le),
               "--iters", str(a.iters), "--warmup", str(a.warmup)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, cwd=ROOT)
        line = [s for s in r.stdout.splitlines() if s.startswith("{")]
        if r.returncode != 0 or not line:
            print("leg %s:%d failed (exit %d):\n%s" % (path, le, r.returncode, r.stdout[-3000:]), file=sys.stderr)
            return 1   # nothing more on the GPU after a failed leg
        print(line[-1])
        res.append(json.loads(line[-1]))
    h = res[0]["it_per_s"]
    print(json.dumps({"summary": {"host_it_per_s": h, "device_le1_it_per_s": res[1]["it_per_s"],
                                  "device_le4_it_per_s": res[2]["it_per_s"],
                                  "speedup_le1": res[1]["it_per_s"] / h, "speedup_le4": res[2]["it_per_s"] / h}}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
