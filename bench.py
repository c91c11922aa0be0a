#!/usr/bin/env python
"""bench.py -- NES iterations/s of the FAKEBOB hot path on MI355X.

Workload (BASELINE.json configs[1]): GMM-UBM OSI targeted attack, 5 enrolled speakers + UBM
(C=2048 diagonal Gaussians, D=72), samples_per_draw=50 -> 51 utterances of 3 s @ 16 kHz scored
per NES iteration.  One "step" = one full NES iteration exactly as FakeBob.attack runs it
(FAKEBOB.py:168-214): Philox noise -> perturb -> int16 -> MFCC/VAD/deltas/CMVN -> GMM
log-likelihoods of all 6 models -> scores -> loss -> gradient estimate -> momentum sign step +
clip, with the early-stop *test* evaluated but not taken so that exactly K steps are timed.
Synthetic audio and seeded synthetic models: no dataset / Kaldi models exist
offline.

Attacks in flight: attacks on different utterances are independent (attackMain.py:324-409), so each
GPU runs --streams K of them concurrently, one engine (= HIP stream + device state) each, driven from K
host threads (ctypes releases the GIL).  Kernels of different attacks then overlap on the chip --
the float64 VALU front-end of one attack runs beside the MFMA GMM kernel of another -- which is what
fills the gaps a single launch chain leaves.  One "step" = one NES iteration of each of the K attacks
in flight; `value` counts all of them.

Multi-GPU: utterances are independent (attackMain.py:324-409), so each rank attacks its own
utterance ("weak" scaling, no data-path collective); RCCL is used only for the barrier, the
max-over-ranks time and the final counter reduction.

A plain run does what the headline figure needs and no more: set-up, precondition and warm-up, the timed windows,
--dump-outputs, the line.  `--full` adds everything else to the same line, unchanged: the dominant kernel with the chip
to itself (roofline.solo_*, whole_chip_grid), `single_attack`, `secondary` (other configurations, whole attacks with
the early stop on, the i-vector systems), `cpu_baseline`; --no-single / --no-secondary / --no-cpu-baseline take parts
of it away again.

Prints ONE JSON line on rank 0.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

S_SPK, C_GAUSS, D_FEAT, SPD, N_SAMPLES = 5, 2048, 72, 50, 48000
PEAK_F16_MFMA_TFLOPS = 2500.0  # MI355X_MICROARCH.md: dense f16/bf16 MFMA peak (32x32x16)
PEAK_F64_MFMA_TFLOPS = 78.6
PEAK_HBM_GBPS = 8000.0
README_GMM_ITS = 0.20         # reference README.md:113 (~5 s / iteration, unspecified CPU)


class Workers(object):
    """K persistent host threads, one per attack in flight (ctypes releases the GIL).  The threads exist before
    the timed region starts: `run` only releases them, so no thread creation / start-up is timed."""

    def __init__(self, K, fn):
        import threading
        self.K, self.fn = K, fn
        self.go = threading.Barrier(K + 1)
        self.done = threading.Barrier(K + 1)
        self.job = None
        self.err = [None] * K
        self.threads = [threading.Thread(target=self._loop, args=(k,), daemon=True) for k in range(K)]
        for t in self.threads:
            t.start()

    def _loop(self, k):
        while True:
            self.go.wait()
            if self.job is None:
                return
            try:
                self.fn(k, *self.job)
            except BaseException as ex:  # noqa: BLE001 -- re-raised on the main thread
                self.err[k] = ex
            self.done.wait()

    def run(self, *job):
        self.job = job
        self.go.wait()
        self.done.wait()
        for ex in self.err:
            if ex is not None:
                raise ex

    def close(self):
        self.job = None
        self.go.wait()
        for t in self.threads:
            t.join()


def emit(out):
    """ONE JSON line, last on stdout: C-level stdio (RCCL / gloo banners) is flushed first."""
    try:
        import ctypes
        ctypes.CDLL(None).fflush(None)
    except Exception:  # noqa: BLE001
        pass
    sys.stdout.flush()
    print(json.dumps(out))
    sys.stdout.flush()


def self_launch(args):
    """`python bench.py --gpus N` outside torchrun: re-exec under torch.distributed.run with one rank per GPU
    (the contract's launch line), so the plain command measures N GPUs and prints n_gpus = N."""
    if args.gpus <= 1 or "RANK" in os.environ or "WORLD_SIZE" in os.environ:
        return
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=%d" % args.gpus,
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    os.environ.setdefault("OMP_NUM_THREADS", "8")
    sys.stdout.flush()
    os.execv(sys.executable, cmd)


def cpu_baseline(audio, models, params_kw, faithful=False, mfcc_f32=0):
    """Times the CPU oracle (the build's C restatement of the identical computation; Kaldi itself
    cannot be installed offline) on one full NES iteration of the same workload, 1 thread --
    the reference's default n_jobs=1 (attackMain.sh:34)."""
    from oracle import oracle as O
    from fakebob_amd.models import stack_models
    gc, miv, iv = stack_models(models)
    ocfg = O.default_cfg(compress_feats=1, text_scores=1, mfcc_f32=mfcc_f32) if faithful else O.default_cfg(mfcc_f32=mfcc_f32)
    ctx = O.GmmSystemCtx(ocfg, "OSI", gc, miv, iv, nthreads=1)
    po = O.nes_params("OSI", "targeted", ctx.S, **params_kw)
    t0 = time.perf_counter()
    O.get_grad(po, ctx.fn, ctx.ctx, audio, seed=42, it=0, stream=0)
    dt = time.perf_counter() - t0
    out = {"value": 1.0 / dt, "unit": "NES iterations/s", "cores": 1, "kind": "port",
           "sample": "1 full NES iteration (51 utterances x 3 s, 6 models) of the same workload, "
                     "CPU oracle single thread, %.1f s" % dt}
    # the same iteration with the oracle's utterance-parallel scoring on every host core (report
    # the single-thread and the all-cores restatement separately; the reference's own default is n_jobs=1)
    try:
        nthr = max(1, len(os.sched_getaffinity(0)))
        if nthr > 1:
            ctx = O.GmmSystemCtx(ocfg, "OSI", gc, miv, iv, nthreads=nthr)
            O.get_grad(po, ctx.fn, ctx.ctx, audio, seed=42, it=0, stream=0)        # warm the thread pool / caches
            t0 = time.perf_counter()
            n = 0
            while n < 3 and time.perf_counter() - t0 < 10.0:
                O.get_grad(po, ctx.fn, ctx.ctx, audio, seed=42, it=n + 1, stream=0)
                n += 1
            dta = (time.perf_counter() - t0) / n
            out["all_cores"] = {"value": 1.0 / dta, "unit": "NES iterations/s", "cores": nthr, "kind": "port",
                                "sample": "%d NES iterations, oracle with %d threads (utterances in parallel), "
                                          "%.2f s each" % (n, nthr, dta)}
    except Exception as ex:  # noqa: BLE001 -- the single-thread number above is the contract
        out["all_cores"] = {"error": str(ex)[:200]}
    return out


def dist_setup(args, torch):
    """(rank, world, device index, dist module or None).  One process per GPU under torchrun; RCCL only carries
    the barrier, the max-over-ranks time and the final counter reduction."""
    from fakebob_amd import parallel
    rank, local_rank, world = parallel.dist_env()
    dev_index = 0 if args.same_device else local_rank
    if world > 1 and not args.same_device and dev_index >= torch.cuda.device_count():
        raise SystemExit("rank %d: --gpus %d but only %d GPUs are visible" % (rank, world, torch.cuda.device_count()))
    dist = None
    if world > 1 or args.force_dist:
        if args.force_dist and world == 1:
            os.environ.setdefault("RANK", "0")
            os.environ.setdefault("WORLD_SIZE", "1")
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            os.environ.setdefault("MASTER_PORT", "29541")
            import torch.distributed as dist
            if args.dist_backend == "nccl":
                torch.cuda.set_device(dev_index)
            dist.init_process_group(args.dist_backend, rank=0, world_size=1)
        else:
            if args.dist_backend == "nccl":
                torch.cuda.set_device(dev_index)
            dist = parallel.init_process_group(args.dist_backend)
    if world > 1 and args.gpus != world:
        print("bench.py: --gpus %d but WORLD_SIZE=%d; reporting n_gpus=%d" % (args.gpus, world, world), file=sys.stderr)
    return rank, world, dev_index, dist


def timed_region(args, torch, dist, workers, K, after_window=None):
    """W untimed warm-up steps, then --repeats consecutive windows of EXACTLY --steps steps of every attack in flight,
    each between two (barrier + device synchronize) pairs, each the max over ranks.  Returns the list of window times in
    seconds; the line reports their MEDIAN as `value` / `ms_per_step` and all of them as `config.windows_ms` (a single
    20-step window is 5.6 ms of GPU time and was seen 7 - 8 %% off the 200-step value: VERDICT r4)."""
    def barrier():
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    if args.warmup > 0:
        workers.run(args.warmup, False)
    barrier()
    barrier()                                               # the first collective of a communicator pays its lazy set-up
    dts = []
    for _ in range(max(1, args.repeats)):
        t0 = time.perf_counter()
        workers.run(args.steps, True)
        barrier()
        dt = time.perf_counter() - t0
        if dist is not None:
            tdev = "cuda" if args.dist_backend == "nccl" else "cpu"
            t = torch.tensor([dt], dtype=torch.float64, device=tdev)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            dt = float(t.item())
        dts.append(dt)
        if after_window is not None:
            after_window()
    return dts


def windows_fields(dts):
    """the timed windows in the forms a record keeps: the list, a short string (a parser that drops lists keeps it), min / max"""
    ms = [1e3 * x for x in dts]
    return {"repeats": len(ms), "windows_ms": ms, "windows_ms_str": " ".join("%.3f" % x for x in ms),
            "windows_ms_min": min(ms), "windows_ms_max": max(ms)}


def median(xs):
    ys = sorted(xs)
    n = len(ys)
    return ys[n // 2] if n % 2 else 0.5 * (ys[n // 2 - 1] + ys[n // 2])


DUMP_MAX_BYTES = 64 << 20


def dump_outputs(out_dir, engs, prms, n, rank=0, world=1):
    """--dump-outputs: what the timed path computed in its last step, one .npy per array (float64), for comparing two
    builds output for output.  Per attack in flight (axis 0): adver_audio (K, n) the adversarial audio after the step,
    scores (K, B, S) and loss (K, B) of the step's NES batch (row 0 = the unperturbed adversarial audio), final_loss /
    adver_loss / distance (K,).  Above DUMP_MAX_BYTES the audio is a fixed, seeded sample of its columns (adver_index).
    With several ranks each writes under out_dir/rank<r>/."""
    import numpy as np
    d = out_dir if world == 1 else os.path.join(out_dir, "rank%d" % rank)
    os.makedirs(d, exist_ok=True)
    st = [e.bench_nes_state(p, n) for e, p in zip(engs, prms)]
    arrs = {"adver_audio": np.stack([x["adver"] for x in st]), "scores": np.stack([x["scores"] for x in st]),
            "loss": np.stack([x["loss"] for x in st])}
    for k in ("final_loss", "adver_loss", "distance"):
        arrs[k] = np.array([x[k] for x in st], np.float64)
    rest = sum(a.nbytes for k, a in arrs.items() if k != "adver_audio") + 4096   # (+ the .npy headers)
    if arrs["adver_audio"].nbytes + rest > DUMP_MAX_BYTES:
        keep = max(1, (DUMP_MAX_BYTES - rest) // (8 * (len(st) + 1)))     # the audio columns and their indices
        idx = np.sort(np.random.RandomState(0).choice(n, size=min(n, keep), replace=False))
        arrs["adver_audio"] = np.ascontiguousarray(arrs["adver_audio"][:, idx])
        arrs["adver_index"] = idx.astype(np.float64)
    for k, a in arrs.items():
        np.save(os.path.join(d, k + ".npy"), a)
    return d


def iv_rooflines(B, n_active, con_ms, solve_ms, R=400):
    """(contraction, solve) roofline objects of an i-vector NES batch of B utterances: the T-matrix contraction against
    HBM (and its float64-MFMA utilisation), the posterior solve against the float64 MFMA peak."""
    tri = R * (R + 1) // 2
    n_bgroups = (B + 63) // 64                                          # utterance groups of 64 -> passes over the rows
    # ALGORITHMIC bytes of the T-matrix contraction: the float64 rows of Sigma^-1 M and U of every component with
    # posterior mass, read once per launch pair -- Kaldi's own loop skips gamma == 0 components
    # (IvectorExtractor::GetIvectorDistMean/Prior); the kernels stream exactly these rows once per
    # 64-utterance group
    bytes_alg = 8.0 * n_active * (D_FEAT * R + tri)
    bytes_all = 8.0 * (C_GAUSS * D_FEAT * R + C_GAUSS * tri)
    bytes_exec = bytes_alg * n_bgroups
    flops_alg = 2.0 * B * n_active * (D_FEAT * R + tri)
    flops_exec = 2.0 * 64 * n_bgroups * n_active * (D_FEAT * R + tri)   # 64-row MFMA tiles
    gbps = bytes_alg / (con_ms * 1e-3) / 1e9 if con_ms else 0.0
    contraction = {"kernel": "k_iv_contract_both = k_iv_contract_dma<lin> + <quad> in one launch (T-matrix contraction: LDS-DMA ring, float64 MFMA "
                             "v_mfma_f64_16x16x4, rows of components with posterior mass only)", "bound": "hbm",
                   "achieved": gbps, "peak": PEAK_HBM_GBPS, "unit": "GB/s", "frac": gbps / PEAK_HBM_GBPS,
                   "traffic": None, "avg_launch_ms": con_ms, "algorithmic_bytes_per_launch": bytes_alg,
                   "active_components": n_active, "executed_bytes_per_launch": bytes_exec,
                   "executed_gbps": bytes_exec / (con_ms * 1e-3) / 1e9 if con_ms else 0.0,
                   "all_components_bytes": bytes_all,
                   "note": "algorithmic bytes = float64 rows of Sigma^-1 M and U of the components with posterior "
                           "mass (the reference's Kaldi loop skips gamma == 0 components too); launch time = the "
                           "contraction launch, HIP events on the attack's stream (with several attacks in flight "
                           "it includes time shared with other attacks' kernels)",
                   "mfma_f64": {"algorithmic_flops_per_launch": flops_alg, "executed_flops_per_launch": flops_exec,
                                "executed_tflops": flops_exec / (con_ms * 1e-3) / 1e12 if con_ms else 0.0,
                                "peak_tflops": PEAK_F64_MFMA_TFLOPS,
                                "frac": flops_exec / (con_ms * 1e-3) / 1e12 / PEAK_F64_MFMA_TFLOPS if con_ms else 0.0}}
    # the posterior solve: B Cholesky factorisations + two triangular solves of R x R (R^3/3 + 2 R^2
    # flops per utterance) on the float64 matrix cores
    solve_flops = B * (R ** 3 / 3.0 + 2.0 * R * R)
    solve_tf = solve_flops / (solve_ms * 1e-3) / 1e12 if solve_ms else 0.0
    solve = {"kernel": "k_iv_solve_rw / k_iv_solve_ll (batched blocked Cholesky + substitutions of the R x R posterior "
                       "precision, v_mfma_f64_16x16x4; the launch includes the back-end and the loss body)", "bound": "mfma", "achieved": solve_tf,
             "peak": PEAK_F64_MFMA_TFLOPS, "unit": "TFLOP/s", "frac": solve_tf / PEAK_F64_MFMA_TFLOPS,
             "traffic": None, "avg_launch_ms": solve_ms, "algorithmic_flops_per_launch": solve_flops,
             "note": "HIP events around every launch of an extra one-attack pass of the same step count"}
    return contraction, solve


def bench_ivector(args, torch):
    """BASELINE.json configs[2] (default: i-vector-PLDA SV targeted, spd=50) and the single-GPU half of configs[4]
    (--task OSI --speakers 10 --spd 200 -> 201 utterances per NES batch), C=2048, D=72, R=400, LDA 200.  Not the
    headline metric: run with --arch iv."""
    from fakebob_amd import parallel
    from fakebob_amd.engine import Engine, nes_params
    from fakebob_amd.models import synthetic_audio, synthetic_ivector_system
    rank, world, dev_index, dist = dist_setup(args, torch)
    t0 = time.perf_counter()
    task, spd = args.task, args.spd
    n_spk = args.speakers if args.speakers is not None else (1 if task == "SV" else 10)
    if task == "SV":
        n_spk = 1
    B = 2 * (spd // 2) + 1
    sy = synthetic_ivector_system(C=C_GAUSS, D=D_FEAT, R=400, L=200, n_speakers=n_spk)
    sy = sy.with_enrolled(sy.enrolled, [-40.0] * n_spk, [10.0] * n_spk)
    K = max(1, args.streams)
    fused = (K < 3) if args.chain == "auto" else (args.chain == "fused")
    engs = []
    for k in range(K):
        e = Engine(dev_index)
        e.set_frontend(mfcc_f32=int(args.frontend == "f32"))
        e.load_ivector(sy, task)
        e.set_fused_chain(fused)
        engs.append(e)
    eng = engs[0]
    t_load = time.perf_counter() - t0
    kw = dict(samples_per_draw=spd, epsilon=0.002, sigma=0.001, max_iter=1000, threshold=1.0)
    if task != "SV":
        kw["target"] = 0
    auds = [synthetic_audio(rank * K + k, N_SAMPLES) for k in range(K)]
    prms = [nes_params(task, "targeted", seed=42, stream=rank * K + k, **kw) for k in range(K)]
    res = [None] * K

    started = [False] * K

    def run(k, n, timed):   # first call: upload + reset; later calls continue the resident attack (see the GMM path)
        res[k] = engs[k].bench_nes(prms[k], auds[k], 0 if not started[k] else -1, n, time_gmm=1 if timed else 0)
        started[k] = True

    workers = Workers(K, run)
    workers.run(max(2, args.precondition // 3), False)     # module load, first-touch allocations, clock ramp: outside everything
    con_acc = []
    dts = timed_region(args, torch, dist, workers, K, after_window=lambda: con_acc.append(sum(r[1] for r in res) / K))
    dt = median(dts)
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, engs, prms, N_SAMPLES, rank, world)
    ms_con = sum(con_acc) / len(con_acc)
    rows = res[0][2]
    total_steps = args.steps * K
    if dist is not None:
        total_steps = parallel.reduce_counters([total_steps], dist)[0]
        assert total_steps == world * args.steps * K
    its = total_steps / dt
    single = None
    solve_ms = None
    if rank == 0 and args.full:
        # one attack in flight, same step count: the latency view, and the pass that times k_iv_solve_ll
        # (HIP events around each of its launches on the attack's stream); without --full roofline_solve has no time
        eng.set_fused_chain(True if args.chain == "auto" else fused)
        d1s = []
        for _ in range(3):   # (median of three passes)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            r1 = eng.bench_nes(prms[0], auds[0], -1, args.steps, time_gmm=2)
            torch.cuda.synchronize()
            d1s.append((time.perf_counter() - t1, r1[1]))
        d1, s1 = sorted(d1s)[1]
        solve_ms = s1 / args.steps
        if os.environ.get("FB_BENCH_VERBOSE"):
            print("bench.py: one-attack pass %.3f ms/step (solve launches %.3f ms)" % (1e3 * d1 / args.steps, solve_ms), file=sys.stderr)
        if K > 1 and not args.no_single:
            single = {"value": args.steps / d1, "unit": "NES iterations/s", "ms_per_step": 1e3 * d1 / args.steps,
                      "note": "one attack in flight (a single launch chain), same workload"}
    workers.close()
    if rank == 0:
        n_active = eng.debug_iv_active()
        con_ms = ms_con / args.steps
        contraction, solve = iv_rooflines(B, n_active, con_ms, solve_ms)
        tr, prov = committed_traffic("k_iv_contract_dma<lin>+<quad>")   # HBM bytes per launch (both kernels), PMC passes
        contraction["traffic"] = tr
        contraction.update(prov)
        if tr and con_ms:   # the PMC bytes (FETCH_SIZE x 2 + WRITE_SIZE, committed profile) over this run's launch time
            contraction["traffic_gbps"] = tr / (con_ms * 1e-3) / 1e9
            contraction["traffic_frac_of_hbm_peak"] = contraction["traffic_gbps"] / PEAK_HBM_GBPS
        dominant = solve if (solve_ms or 0.0) >= con_ms else contraction
        out = {"metric": "NES iterations/sec (i-vector-PLDA %s, samples_per_draw=%d, 3 s@16 kHz)" % (task, spd), "value": its,
               "unit": "NES iterations/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
               "ms_per_step": 1e3 * dt / args.steps, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
               "dtype": "f64 (extractor/PLDA), f32 (gselect: two-term f16 split on MFMA)", "data": "synthetic",
               "vs_readme_nominal": its / 0.083 if (task == "SV" and spd == SPD) else None,
               "single_attack": single,
               "config": {"workload": "i-vector-PLDA %s targeted, %d enrolled, C=2048, D=72, R=400, LDA=200, spd=%d (%d "
                                      "utterances per NES batch), N=48000, %d attacks in flight per GPU"
                                      % (task, n_spk, spd, B, K), "attacks_in_flight_per_gpu": K,
                          "voiced_rows_per_iter": rows, "model_load_s": t_load,
                          "launch_chain": "fused" if fused else "unfused", "full": bool(args.full),
                          **windows_fields(dts),
                          "timing": "median of `repeats` consecutive windows of `steps` steps each"},
               "roofline": dominant, "roofline_contraction": contraction, "roofline_solve": solve}
        if world == 1 and args.full and not args.no_cpu_baseline:
            from oracle import oracle as O
            import numpy as np
            ctx = O.IvSystemCtx(O.default_cfg(mfcc_f32=int(args.frontend == "f32")), sy, nthreads=1)
            n_s = min(B, SPD + 1)                                # a bounded sample: at most 51 utterances (seconds of CPU work)
            wavs = [(synthetic_audio(u, N_SAMPLES) * 32768).astype(np.int16) for u in range(n_s)]
            t0 = time.perf_counter()
            ctx.score_batch(wavs)
            t8 = time.perf_counter() - t0
            out["cpu_baseline"] = {"value": n_s / (t8 * B), "unit": "NES iterations/s", "cores": 1,
                                   "kind": "port", "sample": "%d of the %d utterances of one NES batch (3 s each) scored by "
                                   "the CPU oracle, 1 thread, %.1f s" % (n_s, B, t8)}
        emit(out)
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()
    for e in engs:
        e.close()


GMM_MODE = os.environ.get("FB_GMM_MODE", "fx2") or "fx2"
GMM_TRAFFIC_KEY = {"fx2": "k_gmm_fx2w<5, 6>", "bx3": "k_gmm_bx3<5, false>"}[GMM_MODE]
TRAFFIC_FILE = "r06_traffic.json"
# bf16 32x32x16 chain on random operands, this chip (tools/probes/bx_probe.hip, a round-1 PROBE, not a specification):
# the clock drops to ~1.6 GHz under a saturated matrix pipe (DVFS), which bounds any real kernel below the 2.5 PF peak
MFMA16_POWER_LIMITED_TFLOPS_PROBE = 1660.0


def kernel_source_hash():
    """sha256 over the HIP sources and headers the library is built from: what profiles/<TRAFFIC_FILE> was taken on
    (tools/profile/prof_r05.sh records it) must be what runs now, or the committed PMC traffic is not this build's."""
    import hashlib
    h = hashlib.sha256()
    root = os.path.join(ROOT, "fakebob_amd", "csrc")
    for f in sorted(os.listdir(root)):
        if f.endswith((".hip", ".h")):
            h.update(f.encode())
            with open(os.path.join(root, f), "rb") as r:
                h.update(r.read())
    return h.hexdigest()[:16]


def committed_traffic(key):
    """(hbm bytes per launch, provenance dict) from the committed rocprofv3 PMC passes, or (None, why): PMC counters
    cannot be collected in-process, so the bench line carries the profile's number ONLY when the kernel sources are
    byte-identical to the ones that were profiled -- a stale profile is reported as such, loudly, never as a number."""
    try:
        with open(os.path.join(ROOT, "profiles", TRAFFIC_FILE)) as r:
            tj = json.load(r)
        now = kernel_source_hash()
        if tj.get("kernel_source_sha16") != now:
            print("bench.py: profiles/%s was taken on kernel sources %s, this build is %s -- roofline.traffic is NOT "
                  "reported (re-run tools/profile/prof_r06.sh)" % (TRAFFIC_FILE, tj.get("kernel_source_sha16"), now),
                  file=sys.stderr)
            return None, {"traffic_stale": True, "traffic_profiled_on": tj.get("kernel_source_sha16"), "kernel_source_sha16": now}
        return tj["kernels"][key]["hbm_bytes_per_launch"], {
            "traffic_source": "profiles/%s (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE, separate passes, gfx950 x2 fetch "
                              "correction; taken on these exact kernel sources)" % TRAFFIC_FILE,
            "traffic_profiled_on": tj.get("kernel_source_sha16"), "traffic_profiled_commit": tj.get("commit")}
    except Exception as ex:  # noqa: BLE001
        return None, {"traffic_error": str(ex)[:120]}


def _gmm_roofline(flops_launch, gmm_ms_avg, solo_ms, solo_rows, variant="fx2w/3", tiles=None, M=S_SPK + 1):
    """Roofline of the dominant kernel.  `achieved` = ALGORITHMIC flops ((S+1)*C*4D per voiced frame,
    two length-D dot products per component per model as Kaldi evaluates them) / average launch duration;
    `peak` = the dense peak of the pipe the kernel issues its MFMAs on (f16 / bf16: 2.5 PF), so `frac` is a true
    fraction.  `executed_*`: the products the kernel really issues per (frame, component), K padded to 16*nk:
    k_gmm_fx2w -- the shared quadratic item and the base model with 3 partial products each, every other model as a
    delta item with the products of its component tile (tiles = (#P=1, #P=2, #P=3, #F6)); k_gmm_fx2 / k_gmm_bx3 -- quadratic
    item + one item per model, 3 / 6 partial products each."""
    per_s = 1.0 / (gmm_ms_avg * 1e-3) / 1e12 if gmm_ms_avg > 0 else 0.0
    achieved = flops_launch * per_s
    alg_per_fc = M * 4.0 * D_FEAT                                  # algorithmic flops per (frame, component)
    if GMM_MODE == "fx2":
        nk = (D_FEAT + 1 + 15) // 16
        pipe, peak = "f16 MFMA (v_mfma_f32_32x32x16_f16)", PEAK_F16_MFMA_TFLOPS
        if variant.startswith("fx2w/"):
            n1, n2, n3, n6 = (tuple(tiles) + (0,))[:4] if tiles and sum(tiles) else (0, 0, 1, 0)
            # (an F6 item issues its five f16 MFMAs and four scaled fp6 / fp4 MFMAs per half, each of the latter in the
            #  time of one f16 MFMA: counted as 9 / 5 products' worth of f16 issue slots)
            p_avg = (n1 + 2.0 * n2 + 3.0 * n3 + 1.8 * n6) / (n1 + n2 + n3 + n6)
            ex = flops_launch * (3 + 3 + (M - 1) * p_avg) * 2.0 * 16 * nk / alg_per_fc
            name = ("k_gmm_fx2w<5,%d> (diag-GMM log-likelihood + logsumexp; f32 operands as a two-term f16 split, "
                    "f32 accumulate on v_mfma_f32_32x32x16_f16: shared quadratic item and the base model with 3 partial "
                    "products, the other %d models as deltas from the base model's accumulator with 1 / 2 / 3 products "
                    "per component tile or one product + the corrections on v_mfma_scale_f32_32x32x64_f8f6f4 (F6) "
                    "(%d / %d / %d / %d tiles, components sorted by adaptation distance); accumulators in "
                    "log2 units relative to a per-frame reference: one v_exp_f32 + one v_add_f32 per value; one wave per "
                    "SIMD, 64 frames per wave, software-pipelined)" % (M, M - 1, n1, n2, n3, n6))
        else:
            ex = flops_launch * (1 + M) * 3 * 2.0 * 16 * nk / alg_per_fc
            name = "k_gmm_fx2<5,false> (two-term f16 split, 3 partial products per item, quadratic item shared)"
    else:
        nk = (D_FEAT + 3 + 15) // 16
        ex, pipe, peak = flops_launch * (1 + M) * 6 * 2.0 * 16 * nk / alg_per_fc, "bf16 MFMA (v_mfma_f32_32x32x16_bf16)", PEAK_F16_MFMA_TFLOPS
        name = ("k_gmm_bx3<5,false> (diag-GMM log-likelihood + logsumexp; f32 operands as an exact 3-way bf16 split, "
                "6 partial products on v_mfma_f32_32x32x16_bf16, f32 accumulate)")
    r = {"bound": "mfma", "achieved": achieved, "peak": peak, "unit": "TFLOP/s", "frac": achieved / peak,
         "traffic": None, "avg_launch_ms": gmm_ms_avg, "algorithmic_flops_per_launch": flops_launch,
         "kernel": name, "kernel_variant": variant, "peak_pipe": pipe,
         "executed_flops_per_launch": ex, "executed_tflops": ex * per_s, "executed_frac": ex * per_s / peak}
    r["executed_frac_of_power_limited_probe"] = ex * per_s / MFMA16_POWER_LIMITED_TFLOPS_PROBE
    r["power_limited_probe_tflops"] = MFMA16_POWER_LIMITED_TFLOPS_PROBE
    if solo_ms and solo_ms > 0:
        fl_solo = M * C_GAUSS * 4 * D_FEAT * solo_rows
        r["solo_launch_ms"] = solo_ms
        r["solo_achieved"] = fl_solo / (solo_ms * 1e-3) / 1e12
        r["solo_frac"] = r["solo_achieved"] / peak
        r["solo_executed_frac"] = r["solo_frac"] * ex / flops_launch
    return r


class AttackSet(object):
    """K attacks in flight on one GPU: one engine (= HIP stream + device state) each, a different utterance each,
    driven from K persistent host threads.  run(n, timed): n NES iterations of every attack -- the first call uploads
    the audio and resets the NES state, every later call CONTINUES the resident attack."""

    def __init__(self, engs, prms, auds):
        self.engs, self.prms, self.auds = engs, prms, auds
        self.K = len(engs)
        self.results = [None] * self.K
        self.windows = [None] * self.K
        self.started = [False] * self.K
        self.workers = Workers(self.K, self._run)

    def _run(self, k, n, timed):
        t_in = time.perf_counter()
        self.results[k] = self.engs[k].bench_nes(self.prms[k], self.auds[k], 0 if not self.started[k] else -1, n, time_gmm=timed)
        self.started[k] = True
        self.windows[k] = (t_in, time.perf_counter())

    def run(self, n, timed):
        self.workers.run(n, timed)

    def restart(self):
        """the engines' models or front-end changed: the next run() starts new attacks"""
        self.started = [False] * self.K

    def close(self):
        self.workers.close()


def quick_measure(torch, aset, steps, warm, single_fused=True, chain_fused=None, time_kernel=1):
    """A secondary measurement on rank 0 (no collectives): `warm` untimed, then `steps` timed NES iterations of every
    attack of the set between two device synchronisations, then the same step count with ONE attack in flight.
    Returns a dict; the headline number is NOT measured here (timed_region is)."""
    for e in aset.engs:
        e.set_fused_chain(chain_fused)
    aset.run(max(2, warm), False)
    solo_ms, solo_rows = aset.engs[0].bench_gmm_kernel(10) if time_kernel == 1 and getattr(aset.engs[0], "kind", "gmm") != "iv" else (None, None)
    dts = []
    for _ in range(3):   # the median of three windows (a single 40-step window was seen 40 % off now and then: a clock transient behind a model reload)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        aset.run(steps, time_kernel)
        torch.cuda.synchronize()
        dts.append(time.perf_counter() - t0)
    dt = median(dts)
    out = {"value": steps * aset.K / dt, "unit": "NES iterations/s", "steps": steps, "warmup": max(2, warm), "windows": 3,
           "attacks_in_flight": aset.K, "ms_per_step": 1e3 * dt / steps,
           "kernel_avg_launch_ms": sum(r[1] for r in aset.results) / aset.K / steps}
    if solo_ms:
        out["kernel_solo_launch_ms"] = solo_ms
    aset.engs[0].set_fused_chain(single_fused)
    d1s = []
    for _ in range(3):
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        r1 = aset.engs[0].bench_nes(aset.prms[0], aset.auds[0], -1, steps, time_gmm=time_kernel)
        torch.cuda.synchronize()
        d1s.append(time.perf_counter() - t1)
    d1 = median(d1s)
    out["single_attack"] = {"value": steps / d1, "ms_per_step": 1e3 * d1 / steps, "kernel_launch_ms": r1[1] / steps}
    out["voiced_rows_per_iter"] = int(r1[2])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--streams", type=int, default=3, help="attacks in flight per GPU (one engine/stream each)")
    ap.add_argument("--repeats", type=int, default=9,
                    help="consecutive timed windows of --steps steps each; the line reports their median (config.windows_ms: all)")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps (and, for the solo kernel launches, between the precondition and the warm-up) also "
                         "measure everything the headline figure does not need: the dominant kernel with the chip to itself, one "
                         "attack in flight, the secondary configurations, whole attacks with the early stop on, the CPU baseline.  "
                         "Without it the run sets up, warms up, times the steps and prints the line")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full: skip the CPU baseline")
    ap.add_argument("--no-single", action="store_true", help="--full: skip the extra one-attack-in-flight measurement")
    ap.add_argument("--no-secondary", action="store_true",
                    help="--full: skip the secondary measurements (forced three products, realistic enrolment, "
                         "reference-pipeline mode, GMM CSI, i-vector SV / OSI)")
    ap.add_argument("--arch", default="gmm", choices=["gmm", "iv"], help="gmm = headline (configs[1]); iv = configs[2]")
    ap.add_argument("--e2e-only", action="store_true",
                    help="only the whole-attack measurement (secondary.end_to_end) -- with --gpus N: one list of attacks for the "
                         "whole job, dealt or drawn across ranks (parallel.WorkQueue's cross-rank ticket)")
    ap.add_argument("--dist-backend", default="nccl", help="nccl (= RCCL over xGMI) | gloo (plumbing test)")
    ap.add_argument("--same-device", action="store_true",
                    help="plumbing test on a 1-GPU box: every rank uses cuda:0 (implies a non-RCCL backend)")
    ap.add_argument("--precondition", type=int, default=60,
                    help="untimed iterations per attack run once before the declared warm-up (module load, first-touch "
                         "allocations, clock ramp of a cold GPU); reported in config.precondition_steps")
    ap.add_argument("--chain", default="auto", choices=["auto", "fused", "unfused"],
                    help="launch chain of the attack loop (fb_set_fused_chain): auto = 4 launches per iteration with fewer "
                         "than 3 attacks in flight, 6 launches otherwise (finalisation and loss on their own: they interleave better)")
    ap.add_argument("--task", default=None, choices=["SV", "OSI", "CSI"],
                    help="--arch iv: the system (configs[2]: SV, the default; configs[4]: OSI).  --arch gmm: OSI (headline, "
                         "default) or CSI = configs[3]'s per-GPU work (GMM CSI untargeted, speaker models only)")
    ap.add_argument("--speakers", type=int, default=None, help="--arch iv: enrolled speakers (default 1 for SV, 10 otherwise)")
    ap.add_argument("--spd", type=int, default=SPD, help="--arch iv: samples_per_draw (configs[4]: 200)")
    ap.add_argument("--enrol", default="survey", choices=["survey", "realistic"],
                    help="synthetic speakers: SURVEY.md 8(d)'s 200-frame enrolment (headline) or 20 000 frames (models.ENROL_REALISTIC)")
    ap.add_argument("--faithful", action="store_true",
                    help="run the reference pipeline's two file round trips on the device (MFCCs through Kaldi's "
                         "CompressedMatrix, scores through 6-digit text: gmm_ubm_kaldiHelper.py:138-140, 236-248) -- "
                         "the drop-in modules' default; the headline line is measured without them")
    ap.add_argument("--frontend", default="f32", choices=["f32", "f64"],
                    help="MFCC arithmetic: f32 = Kaldi's own BaseFloat precision (fb_frontend_cfg.mfcc_f32, k_mfcc_f32; C0 from "
                         "the exact integer energy), f64 = float64 between Kaldi's float32 storage points (k_mfcc_r16)")
    ap.add_argument("--force-dist", action="store_true",
                    help="initialise the process group even with one rank (exercises RCCL on a 1-GPU box)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the timed path computed in its last step (adversarial audio, "
                         "scores, losses of every attack in flight) as DIR/<name>.npy (float64, at most 64 MB)")
    args = ap.parse_args()
    if args.steps < 1:
        raise SystemExit("--steps must be at least 1")
    if args.dump_outputs and args.e2e_only:
        raise SystemExit("--dump-outputs writes the outputs of the timed steps; --e2e-only has none")
    self_launch(args)

    import torch  # device sync + torch.distributed (RCCL); imported before the HIP library
    if args.arch == "iv":
        args.task = args.task or "SV"
        return bench_ivector(args, torch)
    gmm_task = args.task or "OSI"
    if gmm_task == "SV":
        raise SystemExit("--arch gmm takes --task OSI (headline) or CSI")
    from fakebob_amd import parallel
    rank, world, dev_index, dist = dist_setup(args, torch)
    from fakebob_amd.engine import Engine, nes_params
    from fakebob_amd.models import ENROL_REALISTIC, synthetic_audio, synthetic_gmm_system

    K = max(1, args.streams)
    fused = (K < 3) if args.chain == "auto" else (args.chain == "fused")
    ubm, spk = synthetic_gmm_system(S_SPK, C_GAUSS, D_FEAT, **(ENROL_REALISTIC if args.enrol == "realistic" else {}))
    kw_common = dict(samples_per_draw=SPD, epsilon=0.002, sigma=0.001, max_lr=0.001, min_lr=1e-6, momentum=0.9,
                     plateau_length=5, plateau_drop=2.0, adver_thresh=0.0, max_iter=1000)

    def system_of(task, ubm_, spk_):
        """(models, attack type, NES keywords, z-norm) of the task's synthetic system"""
        if task == "CSI":   # configs[3]: no UBM, z-normalised speaker log-likelihoods, untargeted
            return list(spk_), "untargeted", dict(kw_common, true=0), ([-150.0] * len(spk_), [5.0] * len(spk_))
        return [ubm_] + list(spk_), "targeted", dict(kw_common, target=0, threshold=0.2277), (None, None)

    models, attack_type, kw, znorm = system_of(gmm_task, ubm, spk)
    engs, auds, prms = [], [], []
    for k in range(K):
        e = Engine(dev_index)
        e.set_frontend(mfcc_f32=int(args.frontend == "f32"))
        if args.faithful:
            e.set_frontend(compress_feats=1, text_scores=1)
        e.load_gmm(models)
        e.set_system(gmm_task, *znorm)
        e.set_fused_chain(fused)
        engs.append(e)
        utt = rank * K + k                                  # a different utterance per attack
        auds.append(synthetic_audio(utt, N_SAMPLES))
        prms.append(nes_params(gmm_task, attack_type, seed=42, stream=utt, **kw))
    audio = auds[0]
    n_models = len(models)
    variant, tiles = engs[0].gmm_kernel_variant, engs[0].gmm_delta_tiles + (engs[0].gmm_delta_tiles_f6,)
    if not variant.startswith("fx2w/") and GMM_MODE == "fx2":
        print("bench.py: WARNING: this system is scored by the general kernel %s, not k_gmm_fx2w (more than %d models, "
              "several variance groups or partial tiles)" % (variant, 10), file=sys.stderr)

    if args.e2e_only:
        r = end_to_end(torch, engs, kw_common, dist=dist, dist_backend=args.dist_backend)
        if rank == 0:
            emit({"metric": "whole attacks with the early stop on (bench.end_to_end)", "n_gpus": world, "end_to_end": r,
                  "value": r["dynamic"]["nes_iterations_per_s"], "unit": "NES iterations/s", "data": "synthetic",
                  "config": {"workload": "24 attacks against the headline system, %d attacks in flight per rank, %d ranks%s"
                             % (K, world, " on ONE device (plumbing run)" if args.same_device else "")}})
        for e in engs:
            e.close()
        if dist is not None:
            dist.barrier()
            dist.destroy_process_group()
        return
    # outside everything: module load, first-touch allocations, the clock ramp of a cold GPU, and (--full) the same GMM
    # launch with the chip to itself
    aset = AttackSet(engs, prms, auds)
    aset.run(max(2, args.precondition), False)
    solo_ms, solo_rows = engs[0].bench_gmm_kernel(20) if args.full else (None, None)
    # ... and the same launch as one workgroup per compute unit (what a lone attack runs): with three or more attacks per GPU the
    # engine launches HALF as many workgroups, each scoring two component chunks one after the other -- slower alone, faster for
    # the job (fb_engine.hip, run_scoring)
    full_ms = None
    if args.full and "FB_GMM_SUB" not in os.environ and not fused:
        os.environ["FB_GMM_SUB"] = "1"
        try:
            full_ms, _ = engs[0].bench_gmm_kernel(20)
        finally:
            os.environ.pop("FB_GMM_SUB", None)
    acc = []
    dts = timed_region(args, torch, dist, aset.workers, K, after_window=lambda: acc.append((list(aset.results), list(aset.windows))))
    dt = median(dts)
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, engs, prms, N_SAMPLES, rank, world)
    results, windows = acc[dts.index(sorted(dts)[len(dts) // 2])]   # the per-attack view of a median window
    ms_dev = sum(sum(r[0] for r in rs) for rs, _ in acc) / K / len(acc)
    ms_gmm = sum(sum(r[1] for r in rs) for rs, _ in acc) / K / len(acc)   # per attack and window: sum over its timed launches
    rows = int(sum(r[2] for r in results) / K)
    total_steps = args.steps * K
    if dist is not None:
        # final counter reduction (mirrors success_cnt / total_cnt, attackMain.py:312,411): the only
        # data the ranks ever exchange
        total_steps, total_scored, _ = parallel.reduce_counters([args.steps * K, args.steps * K * (SPD + 1), rows], dist)
        assert total_steps == world * args.steps * K, (total_steps, world, args.steps, K)
        assert total_scored == total_steps * (SPD + 1)
    its = total_steps / dt
    single = None
    if rank == 0 and K > 1 and args.full and not args.no_single:
        # the same K steps with ONE attack in flight (a single launch chain): the latency view of the same path
        engs[0].set_fused_chain(True if args.chain == "auto" else fused)   # what a lone attack runs (auto: fused)
        d1s = []
        for _ in range(3):   # (median of three passes, like the secondary measurements)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            r1 = engs[0].bench_nes(prms[0], auds[0], -1, args.steps, time_gmm=True)
            torch.cuda.synchronize()
            d1s.append((time.perf_counter() - t1, r1[1]))
        d1, g1 = sorted(d1s)[1]
        single = {"value": args.steps / d1, "unit": "NES iterations/s", "ms_per_step": 1e3 * d1 / args.steps,
                  "gmm_launch_ms": g1 / args.steps, "passes_ms": [1e3 * x[0] for x in d1s],
                  "note": "one attack in flight (a single launch chain), same workload, same step count; the median of three passes"}
    out = None
    if rank == 0:
        gmm_ms_avg = ms_gmm / args.steps
        flops_launch = n_models * C_GAUSS * 4 * D_FEAT * rows  # (S+1)*C*4D*F_voiced
        wl = ("GMM-UBM OSI targeted, 5 speakers+UBM" if gmm_task == "OSI" else
              "GMM CSI untargeted (BASELINE.json configs[3]'s per-GPU work), 5 speaker models, no UBM")
        out = {
            "metric": "NES iterations/sec (and scored-utts/sec) at samples_per_draw=50, 3 s@16 kHz",
            "value": its, "unit": "NES iterations/s", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": 1e3 * dt / args.steps, "higher_is_better": True,
            "scaling": "weak", "vs_baseline": None,
            "dtype": {"fx2": "f32 (GMM: two-term f16 split on MFMA, f32 accumulate, f32-equivalent; %s MFCC; f64 NES)",
                      "bx3": "f32 (GMM: exact bf16x3 split on MFMA, f32 accumulate; %s MFCC; f64 NES)"}[GMM_MODE] % args.frontend,
            "data": "synthetic",
            "scored_utts_per_s": its * (SPD + 1),
            "vs_readme_nominal": its / README_GMM_ITS if gmm_task == "OSI" else None,
            "single_attack": single,
            "per_attack": [{"host_ms": 1e3 * (b - a), "device_ms": r[0], "gmm_ms": r[1]} for (a, b), r in zip(windows, results)],
            "config": {"workload": "%s, C=2048, D=72, spd=50, N=48000 (3 s @ 16 kHz), %d attacks in flight per GPU "
                                   "(1 step = 1 NES iteration of each)%s%s"
                                   % (wl, K, "; reference-pipeline round trips ON (compress_feats, text_scores)" if args.faithful else "",
                                      "; speakers enrolled on 20 000 frames (models.ENROL_REALISTIC)" if args.enrol == "realistic" else ""),
                       "faithful_pipeline": bool(args.faithful), "enrolment": args.enrol, "full": bool(args.full),
                       "frontend_precision": {"f32": "float32 MFCC (Kaldi's BaseFloat; C0 from the exact integer energy), float64 "
                                                     "deltas / CMVN sums", "f64": "float64 between Kaldi's float32 storage points"}[args.frontend],
                       "attacks_in_flight_per_gpu": K, "precondition_steps": max(2, args.precondition),
                       **windows_fields(dts),
                       "timing": "value / ms_per_step: the MEDIAN of `repeats` consecutive windows of exactly `steps` steps, each "
                                 "between (barrier + device synchronize) pairs and max over ranks; windows_ms lists them all",
                       "launch_chain": "4 launches per iteration (fused)" if fused else "6 launches per iteration (mfcc; vad + deltas + cmvn; gmm on half as many workgroups as compute units; finalize; loss; update + next batch)",
                       "voiced_rows_per_iter": rows, "utterances_per_iter": SPD + 1,
                       "gmm_kernel": variant,
                       "gmm_delta_p": {"tiles_p1": tiles[0], "tiles_p2": tiles[1], "tiles_p3": tiles[2],
                                       "tiles_f6": engs[0].gmm_delta_tiles_f6, "shift_rms": engs[0].gmm_shift_rms,
                                       "note": "component tiles (32 components) by the class of their delta items: 1 .. 3 f16 "
                                               "partial products, or F6 = one f16 product + the two corrections as "
                                               "block-scaled fp6 / fp4 products; chosen by fb_load_gmm from the models "
                                               "(DESIGN.md section 5)"},
                       "seeds": {"audio": 1234, "ubm": 2001, "speakers": 2100, "philox": 42}},
            "roofline": dict(_gmm_roofline(flops_launch, gmm_ms_avg, solo_ms, solo_rows, variant, tiles, n_models),
                             gmm_share_of_stream_time=ms_gmm / ms_dev if ms_dev > 0 else None,
                             note="avg_launch_ms: HIP events around every launch of the timed region on each attack's own "
                                  "stream; with several attacks in flight a launch shares the chip with other attacks' "
                                  "kernels (the rocprofv3 average of the same command agrees: profiles/); solo_*: the same "
                                  "launch with the chip to itself, measured before the warm-up (--full only)"),
        }
        if full_ms:
            fl_solo = n_models * C_GAUSS * 4 * D_FEAT * solo_rows
            out["roofline"]["whole_chip_grid"] = {
                "solo_launch_ms": full_ms, "solo_achieved": fl_solo / (full_ms * 1e-3) / 1e12,
                "solo_frac": fl_solo / (full_ms * 1e-3) / 1e12 / PEAK_F16_MFMA_TFLOPS,
                "note": "the same launch with one workgroup per compute unit: what a lone attack runs, and the kernel's own "
                        "fraction of the chip's peak.  The timed region launches half as many workgroups, each scoring two "
                        "component chunks one after the other (solo_launch_ms above; the same partial sums bit for bit): alone "
                        "that is slower, with three attacks in flight the other half of the chip carries the other attacks' "
                        "front-end kernels meanwhile and the job is faster (DESIGN.md section 6)"}
        tr, prov = committed_traffic(GMM_TRAFFIC_KEY if n_models == S_SPK + 1 else GMM_TRAFFIC_KEY.replace("6", str(n_models)))
        out["roofline"]["traffic"] = tr
        out["roofline"].update(prov)
    if rank == 0 and world == 1 and args.full and not args.no_secondary and not args.faithful and args.enrol == "survey" \
            and gmm_task == "OSI" and GMM_MODE == "fx2":
        # ---- secondary measurements of the same run (rank 0, single GPU): small step counts, same code paths.  They
        #      bracket the headline (three delta products forced in every tile = the cost for ANY speaker models) and put
        #      the other configurations of BASELINE.json under the driver's eyes.
        n2 = max(10, min(args.steps, 40))
        sec = {}

        def reload(models_, task_, znorm_, prm_kw, atk, env=None, frontend=None):
            for k_, v_ in (env or {}).items():
                os.environ[k_] = v_
            try:
                for k in range(K):
                    e = engs[k]
                    e.set_frontend(**(frontend or dict(compress_feats=0, text_scores=0)))
                    e.load_gmm(models_)
                    e.set_system(task_, *znorm_)
                    aset.prms[k] = nes_params(task_, atk, seed=42, stream=rank * K + k, **prm_kw)
            finally:
                for k_ in (env or {}):
                    os.environ.pop(k_, None)
            aset.restart()

        def gmm_case(name, note, n_mod):
            r = quick_measure(torch, aset, n2, 10, chain_fused=fused)
            r["gmm_kernel"], r["gmm_delta_tiles"] = engs[0].gmm_kernel_variant, list(engs[0].gmm_delta_tiles) + [engs[0].gmm_delta_tiles_f6]
            fl = n_mod * C_GAUSS * 4 * D_FEAT * r["voiced_rows_per_iter"]
            r["kernel_solo_frac"] = fl / (r["kernel_solo_launch_ms"] * 1e-3) / 1e12 / PEAK_F16_MFMA_TFLOPS
            r["note"] = note
            sec[name] = r
            return r

        try:
            reload(models, "OSI", (None, None), kw, "targeted", env={"FB_GMM_DELTA_P": "3"})
            wc = gmm_case("forced_three_products", "the headline workload with three partial products forced in every tile "
                          "(FB_GMM_DELTA_P=3): what k_gmm_fx2w costs for speaker models adapted arbitrarily far", n_models)
            out["roofline"]["worst_case"] = {
                "kernel_variant": wc["gmm_kernel"], "tiles_p1_p2_p3_f6": wc["gmm_delta_tiles"], "value": wc["value"],
                "single_attack": wc["single_attack"]["value"], "avg_launch_ms": wc["kernel_avg_launch_ms"],
                "solo_launch_ms": wc["kernel_solo_launch_ms"], "solo_frac": wc["kernel_solo_frac"], "steps": n2,
                "note": "same run, same workload, P = 3 in every component tile: what speaker models unrelated to model 0 cost "
                        "(the lower bracket of `value`; models adapted from model 0, however far, run the F6 class: "
                        "secondary.forced_f6)"}
            reload(models, "OSI", (None, None), kw, "targeted", env={"FB_GMM_DELTA_P": "6"})
            gmm_case("forced_f6", "the headline workload with the F6 class forced in every tile (FB_GMM_DELTA_P=6: one f16 "
                     "product + the two corrections as block-scaled fp6 / fp4 products, float32-equivalent scores): what "
                     "k_gmm_fx2w costs for speakers enrolled on any amount of data", n_models)
            ubm_r, spk_r = synthetic_gmm_system(S_SPK, C_GAUSS, D_FEAT, **ENROL_REALISTIC)
            reload([ubm_r] + spk_r, "OSI", (None, None), kw, "targeted")
            gmm_case("realistic_enrolment", "speakers enrolled on 20 000 frames (models.ENROL_REALISTIC: alpha ~ 0.2-0.4 where "
                     "the enrolment data fell), the class of every tile chosen by fb_load_gmm", n_models)
            reload([ubm_r] + spk_r, "OSI", (None, None), kw, "targeted", env={"FB_GMM_DELTA_BUDGET": "5e-5"})
            gmm_case("realistic_enrolment_budget_5e-5", "the same speakers with the delta-product rule's error budget relaxed "
                     "from 6e-6 (float32-equivalent scores, the default) to 5e-5 (inside north_star's 1e-4 against the "
                     "reference; FB_GMM_DELTA_BUDGET, tests/test_gpu_parity.py): what the tolerance itself would buy", n_models)
            reload(models, "OSI", (None, None), kw, "targeted", frontend=dict(compress_feats=1, text_scores=1))
            gmm_case("faithful", "the reference pipeline's two file round trips ON (CompressedMatrix MFCCs, 6-digit score "
                     "text): the drop-in modules' default", n_models)
            if args.frontend == "f32":
                reload(models, "OSI", (None, None), kw, "targeted", frontend=dict(compress_feats=0, text_scores=0, mfcc_f32=0))
                gmm_case("frontend_f64", "the headline workload with the float64-between-storage-points MFCC kernel "
                         "(k_mfcc_r16) instead of the float32 one", n_models)
                for e_ in engs:
                    e_.set_frontend(mfcc_f32=1)
            m_c, atk_c, kw_c, z_c = system_of("CSI", ubm, spk)
            reload(m_c, "CSI", z_c, kw_c, atk_c)
            gmm_case("gmm_csi", "BASELINE.json configs[3]'s per-GPU work: GMM CSI untargeted, 5 speaker models, no UBM "
                     "(`--arch gmm --task CSI` is the full line)", len(m_c))
            # ---- back on the headline system: attacks that STOP (early stop ON) dealt statically / drawn dynamically,
            #      and the headline kernel timed solo once more -- at the clocks everything above has left
            reload(models, "OSI", (None, None), kw, "targeted")
            sec["end_to_end"] = end_to_end(torch, engs, kw_common)
            sec["end_to_end_two_ranks"] = two_rank_end_to_end(K)
            aset.restart()
            aset.run(4, False)
            solo_end, _rows_end = engs[0].bench_gmm_kernel(20)
            out["roofline"]["solo_launch_ms_end"] = solo_end
            out["roofline"]["solo_drift"] = solo_end / solo_ms - 1.0 if solo_ms else None
        except Exception as ex:  # noqa: BLE001 -- the headline above is the contract; a secondary case must not lose it
            sec["error"] = repr(ex)[:300]
        out["secondary"] = sec
    aset.close()
    for e in engs:
        e.close()
    engs = []
    if rank == 0 and out is not None and "secondary" in out and "error" not in out["secondary"]:
        try:
            out["secondary"].update(secondary_ivector(torch, dev_index, K, int(args.frontend == "f32")))
        except Exception as ex:  # noqa: BLE001
            out["secondary"]["ivector_error"] = repr(ex)[:300]
    if rank == 0:
        if world == 1 and args.full and not args.no_cpu_baseline and gmm_task == "OSI":
            ckw = dict(kw)
            out["cpu_baseline"] = cpu_baseline(audio, models, ckw, args.faithful, int(args.frontend == "f32"))
            out["gpu_over_cpu_port"] = its / out["cpu_baseline"]["value"]
        emit(out)
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()


def end_to_end(torch, engs, kw_common, n_utts=24, max_iter=100, reps=3, dist=None, dist_backend="nccl"):
    """Whole attacks with the early stop ON (FAKEBOB.py:181-191), as attackMain.py:324-409 runs them: `n_utts` synthetic
    utterances against the headline system, each with the speaker it already scores highest for as the target and the
    system threshold calibrated (untimed pass) so that the attack stops at a seeded iteration between 8 and 60.  The K engines of the GPU take them from fakebob_amd.parallel.WorkQueue --
    dealt in advance (`static`: stream k takes every K-th, what rounds 1 - 4 did) or drawn when a stream is free
    (`dynamic`) --, alternating, `reps` times each: wall-clock attacks/s and NES iterations/s, the median run of each.
    (trace rows = iterations run: the stopping iteration included.)
    Upload of the audio, read-back of the adversarial audio and trace included (fb_attack).
    With `dist` (several ranks): ONE list of attacks for the whole job -- dealt rank by rank and stream by stream, or drawn
    from the job's ticket (parallel.WorkQueue: `store.add` across ranks) --, a barrier on both sides of each run, the wall
    time the maximum over ranks, the row counts all-reduced (every attack runs on exactly one rank)."""
    import threading
    import numpy as np
    from fakebob_amd import parallel
    from fakebob_amd.engine import nes_params
    from fakebob_amd.models import synthetic_audio
    K = len(engs)
    rng = np.random.default_rng(77)
    items, wanted = [], []
    for u in range(n_utts):
        a = synthetic_audio(200 + u, N_SAMPLES)
        raw, _ = engs[0].score_raw([(a * 32768.0).astype(np.int16)])
        sc = raw[0, 1:] - raw[0, 0]
        tgt = int(np.argmax(sc))
        # calibration (untimed): the attack with an unreachable threshold -- with the target already the best speaker the
        # loss is threshold - s_target, a constant shift that the antithetic estimate cancels -- gives the target score of
        # the clean iterate per iteration; the threshold of the timed attack sits between the record before a seeded
        # iteration n in [8, 60] and the score at n, so the early stop fires there (or an iteration or two beside it)
        kw = dict(kw_common, target=tgt, threshold=float(sc[tgt]) + 10.0, max_iter=72)
        _adv, _flag, _advf, tr = engs[0].attack(nes_params("OSI", "targeted", seed=42, stream=1000 + u, **kw), a)
        st = tr[:, 3 + tgt]
        rec = np.maximum.accumulate(st)
        want = int(rng.integers(8, 61))
        cand = [i for i in range(want, len(st)) if st[i] > rec[i - 1]]
        n_u = cand[0] if cand else int(np.argmax(st))
        thr = 0.5 * (float(rec[n_u - 1]) + float(st[n_u])) if n_u > 0 else float(st[0]) - 1e-3
        wanted.append(n_u)
        kw = dict(kw_common, target=tgt, threshold=thr, max_iter=max_iter)
        items.append((a, nes_params("OSI", "targeted", seed=42, stream=1000 + u, **kw)))
    rows, flags = [0] * n_utts, [0] * n_utts

    world = 1
    if dist is not None:
        world = dist.get_world_size()

    def sync():
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    def run(schedule):
        for i in range(n_utts):
            rows[i], flags[i] = 0, 0
        q = parallel.WorkQueue(n_utts, dist, schedule, streams=K)
        busy, err = [0.0] * K, []

        def worker(k):
            try:
                while True:
                    i = q.next(k)
                    if i is None:
                        break
                    _adv, flag, _advf, tr = engs[k].attack(items[i][1], items[i][0])
                    rows[i], flags[i] = int(tr.shape[0]), int(flag)
                busy[k] = time.perf_counter() - t0
            except BaseException as ex:  # noqa: BLE001
                err.append(ex)
        sync()
        t0 = time.perf_counter()
        ths = [threading.Thread(target=worker, args=(k,)) for k in range(K)]
        [t.start() for t in ths]
        [t.join() for t in ths]
        sync()
        dt = time.perf_counter() - t0
        if dist is not None:
            # (a failing rank is seen by every rank: the counters below would not add up)
            tdev = "cuda" if dist_backend == "nccl" else "cpu"
            t = torch.tensor([dt], dtype=torch.float64, device=tdev)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            dt = float(t.item())
            both = parallel.reduce_counters(list(rows) + list(flags) + [q.drawn, 1 if err else 0], dist)
            assert both[-1] == 0, "an attack stream failed on some rank"
            assert both[-2] == n_utts, ("attacks drawn over all ranks", both[-2], n_utts)
            for i in range(n_utts):
                rows[i], flags[i] = int(both[i]), int(both[n_utts + i])
        if err:
            raise err[0]
        assert all(r > 0 for r in rows), "every attack of the list ran exactly once"
        return dt, busy

    run("dynamic")                                          # untimed: first-touch allocations of the attack path
    res = {"static": [], "dynamic": []}
    for _ in range(reps):
        for sch in ("static", "dynamic"):
            res[sch].append(run(sch))
    out = {"attacks": n_utts, "attacks_in_flight": K, "ranks": world, "max_iter": max_iter, "early_stop": True,
           "iterations_per_attack": list(rows), "calibrated_stop_iterations": wanted,
           "successes": int(sum(1 for f in flags if f == 1)),
           "iterations_total": int(sum(rows)),
           "note": "whole attacks through fb_attack with the early stop ON; the same %d attacks (Philox stream = attack "
                   "index: identical trajectories) dealt statically over the streams or drawn from the ticket queue" % n_utts}
    for sch in ("static", "dynamic"):
        runs = sorted(res[sch], key=lambda r: r[0])
        dt, busy = runs[len(runs) // 2]
        out[sch] = {"wall_s": dt, "attacks_per_s": n_utts / dt, "nes_iterations_per_s": sum(rows) / dt,
                    "stream_busy_s": busy, "runs_wall_s": [r[0] for r in res[sch]]}
    out["dynamic_over_static"] = out["static"]["wall_s"] / out["dynamic"]["wall_s"]
    return out


def two_rank_end_to_end(K):
    """The same measurement as a TWO-rank job on this one device (`--gpus 2 --same-device --dist-backend gloo --e2e-only` in
    a child process): the self-launch under torch.distributed.run, the job's own key-value store, the cross-rank ticket
    (`store.add`) that hands attacks to whichever stream of whichever rank is free, the all-reduced counters.  Not a
    scaling number -- both ranks share the chip --: it puts the N > 1 attack distribution on the GPU box in every run."""
    import subprocess
    cmd = [sys.executable, os.path.abspath(__file__), "--gpus", "2", "--same-device", "--dist-backend", "gloo", "--e2e-only",
           "--streams", str(max(1, K // 2 + K % 2)), "--no-cpu-baseline"]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", OMP_NUM_THREADS="4")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    try:
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600, env=env, cwd=ROOT)
        lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
        if r.returncode != 0 or len(lines) != 1:
            return {"error": (r.stderr or r.stdout)[-300:]}
        d = json.loads(lines[0])["end_to_end"]
        return {"ranks": d["ranks"], "attacks": d["attacks"], "attacks_in_flight_per_rank": d["attacks_in_flight"],
                "iterations_total": d["iterations_total"], "successes": d["successes"],
                "static": {k_: d["static"][k_] for k_ in ("wall_s", "attacks_per_s", "nes_iterations_per_s")},
                "dynamic": {k_: d["dynamic"][k_] for k_ in ("wall_s", "attacks_per_s", "nes_iterations_per_s")},
                "dynamic_over_static": d["dynamic_over_static"],
                "note": "two ranks (gloo) on this one device: attacks dealt in advance or drawn from the job's cross-rank ticket"}
    except Exception as ex:  # noqa: BLE001
        return {"error": repr(ex)[:300]}


def secondary_ivector(torch, dev_index, K, mfcc_f32=1):
    """i-vector-PLDA SV spd=50 (configs[2]) and OSI, 10 speakers, spd=200 (configs[4]'s share of one GPU) with small step
    counts: the numbers `--arch iv` reports in full, under the default line."""
    from fakebob_amd.engine import Engine, nes_params
    from fakebob_amd.models import synthetic_audio, synthetic_ivector_system
    sec = {}
    for name, task, n_spk, spd, steps in (("ivector_sv", "SV", 1, SPD, 20), ("ivector_osi_b201", "OSI", 10, 200, 10)):
        sy = synthetic_ivector_system(C=C_GAUSS, D=D_FEAT, R=400, L=200, n_speakers=n_spk)
        sy = sy.with_enrolled(sy.enrolled, [-40.0] * n_spk, [10.0] * n_spk)
        kw = dict(samples_per_draw=spd, epsilon=0.002, sigma=0.001, max_iter=1000, threshold=1.0)
        if task != "SV":
            kw["target"] = 0
        engs = []
        for k in range(K):
            e = Engine(dev_index)
            e.set_frontend(mfcc_f32=mfcc_f32)
            e.load_ivector(sy, task)
            engs.append(e)
        aset = AttackSet(engs, [nes_params(task, "targeted", seed=42, stream=k, **kw) for k in range(K)],
                         [synthetic_audio(k, N_SAMPLES) for k in range(K)])
        try:
            r = quick_measure(torch, aset, steps, 4, chain_fused=(K < 3), time_kernel=2)
            r["kernel_timed"] = "the posterior solve launch (k_iv_solve_rw / k_iv_solve_ll + back-end + loss)"
            torch.cuda.synchronize()
            rc = engs[0].bench_nes(aset.prms[0], aset.auds[0], -1, steps, time_gmm=1)   # one attack: the contraction's launches
            torch.cuda.synchronize()
            con, sol = iv_rooflines(2 * (spd // 2) + 1, engs[0].debug_iv_active(), rc[1] / steps, r["single_attack"]["kernel_launch_ms"])
            r["roofline"] = {"solve": {k_: sol[k_] for k_ in ("bound", "achieved", "peak", "unit", "frac", "avg_launch_ms")},
                             "contraction": dict({k_: con[k_] for k_ in ("bound", "achieved", "peak", "unit", "frac", "avg_launch_ms",
                                                                         "executed_gbps", "active_components")},
                                                 mfma_f64_frac=con["mfma_f64"]["frac"]),
                             "note": "one attack in flight, HIP events around each launch (bench.iv_rooflines; --arch iv is the full line)"}
            r["note"] = "i-vector-PLDA %s, %d enrolled, spd=%d (%d utterances per NES batch), C=2048, R=400" % (task, n_spk, spd, 2 * (spd // 2) + 1)
            sec[name] = r
        finally:
            aset.close()
            for e in engs:
                e.close()
    return sec


if __name__ == "__main__":
    main()
