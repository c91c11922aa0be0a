#!/usr/bin/env python
"""Golden vectors from the reference's own FAKEBOB.py at the parameter values where the product's NES step switches
kernels, templates or launch paths (samples_per_draw, the speaker count, plateau_length, the utterance length), away
from the recipe's values that make_golden.py covers.  Same means as make_golden.py: the reference is imported, its
np.random.normal is replaced by a frozen legacy stream, the exactly reproducible SynthModel scores.  Run:

    python tests/golden/make_golden_nes_edges.py   ->  tests/golden/g11_nes_edges.npz, tests/golden/g11_meta.json

grad_<i> ...   get_grad cases, as G2 (final_loss, grad, adver_loss, score)
dadv_<i> ...   attack cases, as G3 (adv, flag, trace rows [distance, adver_loss, scores], the printed rates); adv is kept as
               its difference to the int16 cast of the clean audio (int8)
"""
import json
import os
import shutil
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_golden import REF_FB, patched_normal, run_attack  # noqa: E402  (imports the reference's FAKEBOB)
from synth_model import SynthModel, synth_audio  # noqa: E402

GRAD_SPD = [8, 14, 66, 80, 82, 126, 128, 130, 300, 302]


def get_grad_cases():
    """OSI targeted, 5 speakers.  N = 515: three blocks of 256 samples, the last of 3, N % 4 = 3.  spd 1030 at N = 259:
    a batch of more than 1024 utterances."""
    out, meta = {}, []
    for ci, (spd, N) in enumerate([(s, 515) for s in GRAD_SPD] + [(1030, 259)]):
        model = SynthModel("OSI", 5, N, seed=1300 + ci)
        audio = synth_audio(N, 1400 + ci)
        target, thr = ci % 5, 0.1
        fb = REF_FB.FakeBob("OSI", "targeted", model, adver_thresh=0.05, samples_per_draw=spd, sigma=0.001)
        fb.threshold, fb.target, fb.true = thr, target, None
        with patched_normal(1500 + ci):
            final_loss, grad, adver_loss, score = fb.get_grad(audio)
        meta.append(dict(task="OSI", attack="targeted", spd=spd, target=target, true=None, thr=thr, kappa=0.05,
                         n_spk=5, model_seed=1300 + ci, audio_seed=1400 + ci, noise_seed=1500 + ci, N=N))
        out["final_loss_%d" % ci] = np.float64(final_loss)
        out["grad_%d" % ci] = grad
        out["adver_loss_%d" % ci] = np.asarray(adver_loss, np.float64)
        out["score_%d" % ci] = np.asarray(score, np.float64)
    return out, meta


def attack_cases(tmp):
    out, meta = {}, []

    def add(name, task, at, n_spk, N, model_seed, audio_seed, noise_seed, fbkw, atkw):
        model = SynthModel(task, n_spk, N, seed=model_seed)
        a = synth_audio(N, audio_seed)
        adv, flag, trace, lrs, calls = run_attack(tmp, task, at, model, a, noise_seed, fbkw, atkw)
        i = len(meta)
        S = model.S
        T = np.zeros((len(trace), 2 + S))
        for r, row in enumerate(trace):
            assert len(row) == 4                       # [distance, adver_loss, score, used_time]
            T[r, 0] = row[0]
            T[r, 1] = np.asarray(row[1]).reshape(-1)[0]
            T[r, 2:] = np.asarray(row[2], np.float64).reshape(-1)
        # adv minus the int16 cast of the clean audio: within the epsilon ball, so it packs to half of adv's size
        q = (a * 32768.0).astype(np.int16)
        d = adv.reshape(-1).astype(np.int32) - q.astype(np.int32)
        assert np.abs(d).max() <= 127
        out["dadv_%d" % i] = d.astype(np.int8)
        out["trace_%d" % i] = T
        out["lrs_%d" % i] = np.asarray(lrs)
        meta.append(dict(name=name, task=task, attack=at, n_spk=n_spk, model_seed=model_seed, audio_seed=audio_seed,
                         noise_seed=noise_seed, fbkw=fbkw, atkw=atkw, flag=int(flag), n_rows=len(trace),
                         n_get_grad=calls, N=N, adv_shape=list(adv.shape), adv_dtype=str(adv.dtype),
                         last_time_is_zero=bool(trace[-1][3] == 0.0)))
        return meta[-1], np.asarray(lrs)

    base = dict(epsilon=0.002, max_lr=0.001, min_lr=1e-6, samples_per_draw=10, sigma=0.001, momentum=0.9,
                plateau_length=5, plateau_drop=2.0)
    # the window of recent losses: 1, exactly 8 (the last that stays in registers), 9 and 12 (kept in memory), with the
    # settings of make_golden.py's plateau_to_min_lr (a tiny epsilon ball: the loss stalls quickly)
    for pl, iters in ((1, 10), (8, 40), (9, 60), (12, 60)):
        m, lrs = add("plateau_%d" % pl, "OSI", "untargeted", 5, 1601, 601, 701, 1803,
                     dict(base, max_iter=iters, adver_thresh=50.0, epsilon=0.0002, plateau_length=pl, min_lr=2.4e-4),
                     dict(threshold=5.0))
        # the rate did drop -- except with a window of one, whose only loss is never larger than itself (FAKEBOB.py:197)
        assert m["n_rows"] == iters and (lrs.min() < lrs.max()) == (pl > 1), (pl, lrs)
    # speaker counts around the eight scores a thread keeps in registers, and the documented maximum; spd 130 puts
    # B * S on both sides of 2048
    for S in (7, 8, 9, 62):
        add("csi_targeted_S%d_spd130" % S, "CSI", "targeted", S, 1601, 1610 + S, 1710 + S, 1810 + S,
            dict(base, max_iter=4, adver_thresh=50.0, samples_per_draw=130), dict(target=S - 2))
        add("osi_untargeted_S%d_spd12" % S, "OSI", "untargeted", S, 1601, 1910 + S, 2010 + S, 2110 + S,
            dict(base, max_iter=4, adver_thresh=50.0, samples_per_draw=12), dict(threshold=0.3))
    # utterances shorter than, one short of and one past a 256-sample block
    for N in (3, 255, 257):
        add("osi_targeted_N%d" % N, "OSI", "targeted", 5, N, 2200 + N, 2500 + N, 2800 + N,
            dict(base, max_iter=4, adver_thresh=50.0, samples_per_draw=12), dict(threshold=0.1, target=1))
    return out, meta


def main():
    tmp = tempfile.mkdtemp(prefix="fb_golden_")
    try:
        out, gmeta = get_grad_cases()
        aout, ameta = attack_cases(tmp)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    out.update(aout)
    np.savez_compressed(os.path.join(HERE, "g11_nes_edges.npz"), **out)
    with open(os.path.join(HERE, "g11_meta.json"), "w") as w:
        json.dump(dict(numpy=np.__version__, get_grad=gmeta, attack=ameta), w, indent=1, sort_keys=True)
    for f in ("g11_nes_edges.npz", "g11_meta.json"):
        print(f, os.path.getsize(os.path.join(HERE, f)))


if __name__ == "__main__":
    main()
