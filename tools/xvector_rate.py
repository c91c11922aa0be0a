#!/usr/bin/env python
"""What an x-vector victim costs: the stock TDNN (24 -> 512 x 4 -> 1500, R 512, L 150) on 3 s of audio, NES batches of 51 rows
(samples_per_draw = 50) and 1 031 rows (1 030).

    python tools/xvector_rate.py [--samples 48000] [--reps 10] [--repeat 5] [--iters 30] [--warmup 5] [--no-torch]

Prints JSON lines (one engine, nothing else of this process on the GPU: "solo" launches):
  what=kernels  per batch size: median over --repeat of the milliseconds per launch (device events around --reps launches after
                one to warm up; fb_bench_xvector) of k_xv_rowmax and k_xv_affine per frame layer, k_xv_pool, k_xv_segment and
                k_iv_backend, on rows x 298 seeded feature rows; k_xv_affine's FLOP (2 * rows * K * dout per layer, the padded
                K steps not counted), its achieved TFLOP/s and that as a fraction of one third of the 2.5 PFLOP/s f16 peak
                (three f16 products per f32-equivalent one).
  what=nes      per batch size: NES iterations per second of one attack on the native system (fb_bench_nes: device events
                around --iters iterations after --warmup), the chain's own milliseconds per iteration (events around
                run_xvector) and the voiced rows of a batch.
  what=torch    the same weights as a float32 PyTorch module attacked through fb_attack_dev in this process: iterations per
                second on the host's clock around --iters iterations that end in the call's own synchronise, and the
                module's milliseconds per batch alone.  Its front end is tests/foreign_models.FrameModel's (framing, one
                seeded projection, log): no MFCC, no VAD, no CMVN -- far less work than the engine's front end, so the
                comparison favours this route."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
PEAK_F16_TFLOPS = 2500.0
T_FRAMES = 298          # frames of 3 s at 10 ms (snip-edges)


def emit(**kw):
    print(json.dumps(kw))
    sys.stdout.flush()


def torch_model(torch, sy, device):
    """models.XvectorSystem -> an object with score_device(x [B, N]) -> [B] float32 LLR-like scores (SV)"""
    from tests.foreign_models import FrameModel

    class TorchXvector(FrameModel):
        def __init__(self):
            FrameModel.__init__(self, "SV", 1, device, seed=1, n_feat=sy.D)
            t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(device)   # noqa: E731
            self.layers = [(list(ly["ctx"]), t(ly["W"]).T.contiguous(), t(ly["bias"]), t(ly["bn_scale"]), t(ly["bn_offset"]))
                           for ly in sy.layers]
            self.segW, self.segb = t(sy.seg_W).T.contiguous(), t(sy.seg_bias)
            self.lda = t(sy.lda[:, :sy.R]).T.contiguous()
            self.psi = t(sy.plda_psi)
            from tests import xvector_ref as ref
            self.train = t(ref.backend_transform(sy, sy.enrolled[0]))

        @torch.no_grad()
        def score_device(self, x):
            self.n_calls += 1
            x = x.float()
            B = x.shape[0]
            fr = x.unfold(1, self.frame, self.hop)
            T = fr.shape[1]
            h = torch.log((fr.reshape(B * T, self.frame) @ self.P) ** 2 + 1e-4).reshape(B, T, -1)
            h = h - h.mean(dim=1, keepdim=True)
            ar = torch.arange(T, device=x.device)
            for ctx, W, b, sc, of in self.layers:
                sp = torch.cat([h[:, torch.clamp(ar + c, 0, T - 1)] for c in ctx], dim=2)
                h = sc * torch.relu(sp @ W + b) + of
            mean = h.mean(dim=1)
            std = torch.sqrt(torch.clamp((h * h).mean(dim=1) - mean * mean, min=1e-10))
            emb = torch.cat([mean, std], dim=1) @ self.segW + self.segb
            z = emb @ self.lda
            y = z * (z.shape[1] ** 0.5) / z.norm(dim=1, keepdim=True)
            psi = self.psi
            d = y - psi / (psi + 1.0) * self.train
            var = 1.0 + psi / (psi + 1.0)
            return -0.5 * ((d * d / var).sum(dim=1) + torch.log(var).sum()) + 0.5 * ((y * y / (psi + 1.0)).sum(dim=1) + torch.log(psi + 1.0).sum())

    return TorchXvector()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=48000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--batches", default="51,1031")
    args = ap.parse_args()
    from fakebob_amd import _native
    torch = _native.torch_first()
    from fakebob_amd.attack import FakeBob
    from fakebob_amd.engine import Engine, nes_params
    from fakebob_amd.models import synthetic_audio, synthetic_xvector_system
    n = args.samples
    batches = [int(b) for b in args.batches.split(",")]
    e = Engine(0)
    try:
        e.set_frontend(delta_order=0, mfcc_f32=1)
        sy = synthetic_xvector_system(e.feat_dim)
        sy = sy.with_enrolled(sy.enrolled, [-40.0], [10.0])
        e.load_xvector(sy, "SV")
        flop_per_row = [2.0 * ly["W"].shape[0] * ly["W"].shape[1] for ly in sy.layers]
        for B in batches:
            runs = [e.bench_xvector(B, T_FRAMES, reps=args.reps) for _ in range(args.repeat)]
            med = lambda f: float(np.median([f(r) for r in runs]))   # noqa: E731
            rows = B * T_FRAMES
            affine = [med(lambda r, l=l: r["affine"][l]) for l in range(len(sy.layers))]
            rowmax = [med(lambda r, l=l: r["rowmax"][l]) for l in range(len(sy.layers))]
            flop = rows * sum(flop_per_row)
            tf = flop / (sum(affine) * 1e-3) / 1e12
            emit(what="kernels", batch=B, rows=rows, solo_launch_ms=dict(k_xv_affine=affine, k_xv_rowmax=rowmax, k_xv_pool=med(lambda r: r["pool"]),
                 k_xv_segment=med(lambda r: r["segment"]), k_iv_backend=med(lambda r: r["backend"])),
                 k_xv_affine_ms=sum(affine), k_xv_affine_GFLOP=flop * 1e-9, k_xv_affine_TFLOPs=tf,
                 k_xv_affine_frac_of_third_f16_peak=tf / (PEAK_F16_TFLOPS / 3.0), repeat=args.repeat, reps=args.reps)
        audio = synthetic_audio(0, n)
        for B in batches:
            p = nes_params("SV", "targeted", adver_thresh=1e6, threshold=0.0, samples_per_draw=B - 1, seed=3, max_iter=args.iters)
            ms, chain_ms, rows = e.bench_nes(p, audio, args.warmup, args.iters, time_gmm=True)
            emit(what="nes", batch=B, iters=args.iters, it_per_s=args.iters / (ms * 1e-3), ms_per_iter=ms / args.iters,
                 xvector_chain_ms_per_iter=chain_ms / args.iters, voiced_rows=int(rows))
    finally:
        e.close()
    if args.no_torch:
        return 0
    model = torch_model(torch, sy, "cuda:0")
    for B in batches:
        fb = FakeBob("SV", "targeted", model, samples_per_draw=B - 1, verbose=False)
        eng = fb._engine()

        def run(k):
            p = nes_params("SV", "targeted", adver_thresh=1e6, max_iter=k, samples_per_draw=B - 1, threshold=0.0, seed=3)
            x, sc = fb._device_buffers(n, 1)
            return eng.attack_dev(p, 1, model.score_device, x, sc, audio, look_every=0)[3].shape[0]

        run(args.warmup)
        t0 = time.perf_counter()
        done = run(args.iters)
        dt = time.perf_counter() - t0
        x, _sc = fb._device_buffers(n, 1)
        model.score_device(x)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        for _ in range(5):
            model.score_device(x)
        torch.cuda.synchronize()
        emit(what="torch", batch=B, iters=done, it_per_s=done / dt, ms_per_iter=1e3 * dt / done,
             module_ms_per_batch=1e3 * (time.perf_counter() - t1) / 5)
    return 0


if __name__ == "__main__":
    sys.exit(main())
