#!/usr/bin/env python
"""Multi-GPU counterpart of the reference's driver (attackMain.py:274-475) -- SURVEY.md 8(f) row 1.

Same command-line flags, data layout (`data/test-set/<spk>/*.wav`, `data/illegal-set/...`), model
pickles (`model/<spk>.gmm|.iv` = [spk_id, utt_id, identity_location, z_mean, z_std]), benign-decision
filtering (CSI keeps correctly classified voices :129, OSI/SV keep rejected ones :201,:266), target
expansion (:141-162, :213-227), output naming (`<name>_<target>.wav` / `.cp`) and success-rate print
(`%d`, :411) as the reference.  What differs: every (audio, target) attack is independent, so the
list is sharded round-robin over the ranks of a `torch.distributed.run` launch (one process per
GPU) and, inside a rank, over `--streams` engines driven by host threads; the estimated threshold is
computed on rank 0 and broadcast, the success counters are all-reduced (fakebob_amd/parallel.py).

    python -m torch.distributed.run --nproc-per-node 8 -m fakebob_amd.attack_main -spk_id 1580 2830 61 ...

(The reference's own attackMain.py also runs unmodified on the engine: see fakebob_amd/dropin/.)
"""
import argparse
import functools
import os
import pickle
import threading

import numpy as np
from scipy.io.wavfile import read, write

from . import parallel
from .attack import FakeBob
from .codec import NAMES as CODEC_NAMES

bits_per_sample = 16
fs = 16000


def load_spk_models(model_dir, spk_id_list, architecture):
    ext = ".iv" if architecture == "iv" else ".gmm"
    out = []
    for spk_id in spk_id_list:
        with open(os.path.join(model_dir, spk_id + ext), "rb") as r:
            out.append(pickle.load(r))
    return out


def make_model(architecture, task, model_list, pre_model_dir, threshold, group_id, dither=None, input_transform=None,
               feature_compression=None, air_channel=None, codec=None):
    """attackMain.load_model (:38-85).  dither: the systems' keyword (Kaldi's --dither: a number, or "conf");
    input_transform: theirs too (the defended victim's input-transform chain, a spec such as "ms:7"); feature_compression:
    theirs as well (the feature-level defence, a spec such as "0.5" or "0.5:10"); air_channel: theirs too (the random room
    in front of the victim, a spec such as "t60:200-600,drr:6"); codec: theirs as well (the telephone line in front of the
    victim: "ulaw", "alaw" or "adpcm")."""
    from .systems import gmm_CSI, gmm_OSI, gmm_SV, iv_CSI, iv_OSI, iv_SV
    ubm = os.path.join(pre_model_dir, "final.dubm")
    if architecture == "iv":
        if task == "OSI":
            return iv_OSI(group_id, model_list, pre_model_dir=pre_model_dir, threshold=threshold, dither=dither,
                          input_transform=input_transform, feature_compression=feature_compression, air_channel=air_channel, codec=codec)
        if task == "CSI":
            return iv_CSI(group_id, model_list, pre_model_dir=pre_model_dir, dither=dither,
                          input_transform=input_transform, feature_compression=feature_compression, air_channel=air_channel, codec=codec)
        return iv_SV(group_id, model_list[0], pre_model_dir=pre_model_dir, threshold=threshold, dither=dither,
                          input_transform=input_transform, feature_compression=feature_compression, air_channel=air_channel, codec=codec)
    if task == "OSI":
        return gmm_OSI(group_id, model_list, ubm, pre_model_dir=pre_model_dir, threshold=threshold, dither=dither,
                          input_transform=input_transform, feature_compression=feature_compression, air_channel=air_channel, codec=codec)
    if task == "CSI":
        return gmm_CSI(group_id, model_list, pre_model_dir=pre_model_dir, dither=dither,
                          input_transform=input_transform, feature_compression=feature_compression, air_channel=air_channel, codec=codec)
    return gmm_SV(group_id, model_list[0], ubm, pre_model_dir=pre_model_dir, threshold=threshold, dither=dither,
                          input_transform=input_transform, feature_compression=feature_compression, air_channel=air_channel, codec=codec)


def collect_voices(data_dir):
    """[(spk_id, file_name, float audio in [-1,1))] in a deterministic (sorted) order."""
    out = []
    for spk_id in sorted(os.listdir(data_dir)):
        d = os.path.join(data_dir, spk_id)
        if not os.path.isdir(d):
            continue
        for name in sorted(os.listdir(d)):
            _, a = read(os.path.join(d, name))
            out.append((spk_id, name, a / (2 ** (bits_per_sample - 1))))
    return out


def build_attack_list(task, attack_type, model, test_dir, illegal_dir, out_audio_dir, out_cp_dir):
    """attackMain.loadData (:87-272) -> list of dicts {audio, true, target, wav_path, cp_path, name, spk}."""
    voices = collect_voices(test_dir if task == "CSI" else illegal_dir)
    if not voices:
        return []
    spk_ids = list(model.spk_ids) if hasattr(model, "spk_ids") else []
    decisions, _ = model.make_decisions([v[2] for v in voices], fs=fs, bits_per_sample=bits_per_sample)
    decisions = decisions if isinstance(decisions, list) else [decisions]
    items = []
    for (spk, name, audio), dec in zip(voices, decisions):
        stem = name.split(".")[0]
        base = dict(audio=audio, name=name, spk=spk, true=None, target=None,
                    wav_path=os.path.join(out_audio_dir, spk, name),
                    cp_path=os.path.join(out_cp_dir, spk, stem + ".cp"))
        if task == "CSI":
            true = spk_ids.index(spk)
            if int(dec) != true:          # skip those wrongly classified (:127-129)
                continue
            base["true"] = true
        elif int(dec) != -1:              # OSI / SV: keep voices the system rejects (:199-201, :264-266)
            continue
        if task != "SV" and attack_type == "targeted":
            for t in range(len(spk_ids)):
                if task == "CSI" and t == base["true"]:
                    continue
                it = dict(base, target=t)
                it["wav_path"] = os.path.join(out_audio_dir, spk, stem + "_" + str(t) + ".wav")
                it["cp_path"] = os.path.join(out_cp_dir, spk, stem + "_" + str(t) + ".cp")
                items.append(it)
        else:
            items.append(base)
    return items


def with_companions(items, idx, count):
    """--companions: items[idx]'s audio and the next `count` utterances of its speaker (companions.pick_companions), all
    cropped to the shortest of them -- printed, never silent -> (audio, list of companions; [] when the speaker has no
    other utterance)."""
    from .companions import crop_to_shortest, pick_companions
    picks = pick_companions(items, idx, count)
    wavs, n = crop_to_shortest([items[idx]["audio"]] + [items[i]["audio"] for i in picks])
    cut = [(items[i]["name"], items[i]["audio"].shape[0]) for i in [idx] + picks if items[i]["audio"].shape[0] != n]
    print("--- %s/%s: %d companions (%s), %d samples each%s ---" % (
        items[idx]["spk"], items[idx]["name"], len(picks), ", ".join(items[i]["name"] for i in picks) or "none", n,
        "".join("; %s cropped from %d" % c for c in cut)))
    return wavs[0], wavs[1:]


def _int_pair(text):
    """'A:B' -> (int A, int B): --hsj-evals"""
    parts = text.split(":")
    if len(parts) != 2:
        raise argparse.ArgumentTypeError("expected A:B, got %r" % text)
    try:
        return int(parts[0]), int(parts[1])
    except ValueError:
        raise argparse.ArgumentTypeError("expected two integers A:B, got %r" % text)


def _pair(text):
    """'A:B' -> (float A, float B): --pso-w, --pso-c"""
    parts = text.split(":")
    if len(parts) != 2:
        raise argparse.ArgumentTypeError("%r: two numbers joined by a colon" % (text,))
    try:
        return float(parts[0]), float(parts[1])
    except ValueError:
        raise argparse.ArgumentTypeError("%r: two numbers joined by a colon" % (text,))


def _quorum(text):
    """--query-eot's value: "majority" or 1 .. 32"""
    from .query_eot import quorum_code
    q = text if text == "majority" else int(text)
    if quorum_code(q) == 0:
        raise ValueError(text)
    return q


def print_votes(attack, name, flag, res):
    """--query-eot: the summary of an attack's logged votes (Kenansville's and HopSkipJump's results carry them)"""
    votes = getattr(res, "votes", None)
    if votes is None:
        return
    v = np.asarray(votes).reshape(-1)
    v = v[v >= 0]
    if v.size:
        print("%s %s: success %d, votes of %d rows: min %d, mean %.2f, max %d" % (attack, name, flag, v.size, v.min(), v.mean(), v.max()))


def _play_offset(text):
    """--play-offset's value: "max" or an integer 0 .. 2^31 - 2"""
    from .play_offset import check_offset
    t = str(text).strip().lower()
    if t == "max":
        return "max"
    try:
        return check_offset(int(t))
    except ValueError as ex:
        raise argparse.ArgumentTypeError("--play-offset: 'max' or an integer 0 .. 2^31 - 2 (%s)" % ex)


def set_play_offset(bob, option, n_samples):
    """--play-offset for the attack that comes next: through the attack object's own check where it has one (the PGD classes:
    an offset needs universal=True), else the attribute FakeBob.attack reads"""
    from .play_offset import parse_option
    S = parse_option(option, n_samples)
    if hasattr(bob, "_set_play_offset"):
        bob._set_play_offset(S)
    else:
        bob.play_offset = S


def print_offsets(name, res):
    """--play-offset: how many of the grid's offsets succeeded on every utterance (AttackResult.per_offset)"""
    per = getattr(res, "per_offset", None)
    if per:
        print("play offset %s: %s of %d offsets succeed (utterance 0 first)" % (name, [d["n_success"] for d in per], len(per[0]["offsets"])))


def main(argv=None, model_factory=None, bob_factory=None):
    """model_factory(architecture, task, model_list, pre_model_dir, threshold, group_id) / bob_factory(task,
    attack_type, model, **hyper_parameters): injection points for the driver-rule tests (a stub model / stub FakeBob
    as in tests/golden/driver_site.py); default: the GPU systems and fakebob_amd.attack.FakeBob."""
    ap = argparse.ArgumentParser()
    ap.add_argument("--speaker_id", "-spk_id", nargs="+", type=str, required=True)
    ap.add_argument("--architecture", "-archi", default="gmm", choices=["gmm", "iv"])
    ap.add_argument("--task", "-task", default="OSI", choices=["OSI", "CSI", "SV"])
    ap.add_argument("--attack_type", "-type", default="targeted", choices=["untargeted", "targeted"])
    ap.add_argument("--adver_thresh", "-adver", default=0., type=float)
    ap.add_argument("--epsilon", "-epsilon", default=0.002, type=float)
    ap.add_argument("--max_iter", "-max_iter", default=1000, type=int)
    ap.add_argument("--max_lr", "-max_lr", default=0.001, type=float)
    ap.add_argument("--min_lr", "-min_lr", default=1e-6, type=float)
    ap.add_argument("--samples_per_draw", "-samples", default=50, type=int)
    ap.add_argument("--sigma", "-sigma", default=0.001, type=float)
    ap.add_argument("--momentum", "-momentum", default=0.9, type=float)
    ap.add_argument("--plateau_length", "-plateau_length", default=5, type=int)
    ap.add_argument("--plateau_drop", "-plateau_drop", default=2.0, type=float)
    ap.add_argument("--n_jobs", "-nj", default=1, type=int)                     # accepted, unused
    ap.add_argument("--debug", "-debug", default="f", choices=["t", "f"])       # accepted, unused
    ap.add_argument("--threshold", "-thresh", default=0., type=float)
    ap.add_argument("--streams", default=3, type=int, help="attacks in flight per GPU")
    ap.add_argument("--schedule", default="dynamic", choices=["dynamic", "static"],
                    help="dynamic: free attack streams draw the next attack (ticket counter); static: round-robin deal")
    ap.add_argument("--seed", default=None, type=int, help="Philox key (default: from numpy's global RNG)")
    ap.add_argument("--dither", default=None,
                    help="Kaldi's --dither for the victim's front end: a number, or 'conf' for what pre-models/conf/mfcc.conf "
                         "configures (Kaldi's 1.0 when it is silent); default: off, or FB_DITHER")
    ap.add_argument("--dither-seed", dest="dither_seed", default=0, type=int,
                    help="dither key of the scoring calls outside an attack (inside one, --seed and the attack's stream key it)")
    ap.add_argument("--input-transform", dest="input_transform", default=None,
                    help="attack a defended victim: the input-transform chain in front of its recogniser, e.g. 'ms:7', "
                         "'qt:512', 'ds:2', 'lpf:4000' or several joined by commas (fakebob_amd/input_transform.py); "
                         "default: none, or FB_INPUT_TRANSFORM")
    ap.add_argument("--air-channel", dest="air_channel", default=None, metavar="SPEC",
                    help="attack over the air: a random room impulse response in front of the victim, drawn afresh for "
                         "every query, e.g. 't60:200-600,drr:6,taps:2048,delay:32' (t60 in ms, required; "
                         "fakebob_amd/air_channel.py); randomised, so combine with --eot-size; default: none, or FB_AIR_CHANNEL")
    ap.add_argument("--codec", dest="codec", default=None, choices=CODEC_NAMES + ("none",), metavar="NAME",
                    help="attack through a telephone line: the encode / decode round trip of a line codec directly behind the "
                         "input-transform chain, one of 'ulaw', 'alaw' (G.711), 'adpcm' (IMA ADPCM, 4 bit) "
                         "(fakebob_amd/codec.py); default: none, or FB_CODEC")
    ap.add_argument("--feco", dest="feco", default=None, metavar="RATIO[:ITERS]",
                    help="attack a victim defended by feature compression: k-means over every utterance's voiced frames, "
                         "RATIO * T cluster centres scored in their place after ITERS (default 10) Lloyd iterations, e.g. "
                         "'0.5' or '0.2:10'; randomised, so combine with --eot-size; default: none, or FB_FECO")
    ap.add_argument("--eot-size", dest="eot_size", default=None, type=int,
                    help="expectation over transformation against a randomised victim (a 'noise:' / 'at:' stage, --dither): "
                         "every NES sample is scored under this many independent draws and the losses are averaged "
                         "(1 .. 32); default: 1, or FB_EOT_SIZE")
    ap.add_argument("--query-eot", dest="query_eot", nargs="?", const="majority", default=None, type=_quorum, metavar="Q",
                    help="--attack pso | kenansville | hsj: take --eot-size and --companions -- every candidate is scored "
                         "utterances * eot-size times and counts as adversarial from Q adversarial replicas on (its votes; "
                         "no value: the majority; pso reads the mean loss).  Without this flag the three attacks refuse both")
    ap.add_argument("--companions", dest="companions", default=0, type=int, metavar="N",
                    help="universal perturbation: the next N utterances of the same speaker in the data directory ride along "
                         "with every attacked one (1 .. 31, times --eot-size at most 32); all are cropped to the shortest, "
                         "which is printed; default: 0")
    ap.add_argument("--play-offset", dest="play_offset", default=None, type=_play_offset, metavar="S|max",
                    help="--attack nes | pgd: the perturbation plays on a loop and cannot be timed to the victim's speech -- every "
                         "replica of every row (--eot-size, --companions) carries it rotated by an offset of its own, uniform in "
                         "0 .. S samples; 'max': the whole loop, N - 1 of the (cropped) utterance; --attack pgd needs --wb-universal; "
                         "the result's per_offset counts are printed; default: none")
    ap.add_argument("--attack", default="nes", choices=["nes", "pso", "kenansville", "hsj", "pgd", "cw2", "psy"],
                    help="the search: FAKEBOB's NES gradient estimate (default), SirenAttack's particle swarm "
                         "(fakebob_amd/pso.py; -epsilon, -max_iter, -adver and --seed apply, the other NES options do not), "
                         "Kenansville's decision-only spectral removal (fakebob_amd/kenansville.py; --kv-* and --seed apply), hsj: "
                         "HopSkipJump, the decision-only attack that reaches a decision from a starting audio that already has it "
                         "(fakebob_amd/hsj.py; --hsj-*, -max_iter and --seed apply; a targeted attack needs --hsj-init) or the "
                         "white-box gradient attack (fakebob_amd/pgd.py: the analytic gradient of a GMM-UBM system in FAKEBOB's "
                         "loop; -momentum 0 is PGD, -max_iter 1 the single step; -samples and -sigma do not apply; an undefended "
                         "victim unless --bpda is given); cw2: Carlini-Wagner's L2 attack on the same gradient "
                         "(fakebob_amd/cw2.py: tanh space, Adam, a binary search over the constant; it minimises the distortion; "
                         "-max_iter counts the iterations of one search step, -adver is CW's confidence, --cw2-* apply; --bpda "
                         "--eot-size and -archi iv --wb-ivector as for pgd); psy: cw2's loop with the psychoacoustic masking "
                         "distortion in its place (fakebob_amd/psy.py; --psy-window, --psy-l2-weight and --cw2-* apply)")
    ap.add_argument("--psy-window", dest="psy_window", default=2048, type=int, choices=[512, 1024, 2048],
                    help="--attack psy: CW2's loop with the psychoacoustic masking distortion in place of |delta|^2 "
                         "(fakebob_amd/psy.py; --cw2-* apply as for cw2); this is the STFT window of the masking model, hop = window/4")
    ap.add_argument("--psy-l2-weight", dest="psy_l2_weight", default=0.0, type=float,
                    help="--attack psy: this much of CW2's |delta|^2 is added to the masking distortion (default 0: masking alone)")
    ap.add_argument("--cw2-const", dest="cw2_const", default=1e-3, type=float, help="--attack cw2: the initial trade-off constant c")
    ap.add_argument("--cw2-steps", dest="cw2_steps", default=9, type=int, help="--attack cw2: binary search steps over c (1 .. 32)")
    ap.add_argument("--cw2-lr", dest="cw2_lr", default=1e-2, type=float, help="--attack cw2: Adam's learning rate in tanh space")
    ap.add_argument("--cw2-abort-every", dest="cw2_abort_every", default=1000, type=int,
                    help="--attack cw2: every this many iterations a search step ends unless its objective fell by 0.01 %%; 0: never")
    ap.add_argument("--bpda", action="store_true",
                    help="--attack pgd: the adaptive attack on a defended victim -- BPDA through --input-transform and --codec, "
                         "expectation over --eot-size draws of the random stages; --air-channel is refused unless --wb-air is "
                         "given, --feco and --dither unless --wb-frontend is given, --companions unless --wb-universal is given")
    ap.add_argument("--wb-air", dest="wb_air", action="store_true",
                    help="--attack pgd: differentiate through --air-channel as well (fakebob_amd/pgd.py: air=True; the forward's "
                         "drawn room responses transposed, with --bpda --eot-size r the expectation over r rooms per iteration); "
                         "on a GMM-UBM system with --bpda, on -archi iv with --wb-ivector")
    ap.add_argument("--wb-frontend", dest="wb_frontend", action="store_true",
                    help="--attack pgd: differentiate through --feco and --dither as well (fakebob_amd/pgd.py: frontend=True; the "
                         "forward's final k-means assignment and its dither draws held constant, with --bpda --eot-size r the "
                         "expectation over r draws per iteration); needs no other switch at --eot-size 1")
    ap.add_argument("--wb-universal", dest="wb_universal", action="store_true",
                    help="--attack pgd: take --companions N (fakebob_amd/pgd.py: universal=True; the gradient of the loss averaged "
                         "over the N + 1 utterances, with --bpda --eot-size r over r draws of each); needs no other switch on an "
                         "undefended GMM-UBM victim; on -archi iv with --wb-ivector, where it also allows --bpda --eot-size r")
    ap.add_argument("--wb-ivector", dest="wb_ivector", action="store_true",
                    help="--attack pgd -archi iv: differentiate the i-vector-PLDA victim (fakebob_amd/pgd.py: IvectorPGD; the "
                         "frames' component selection and pruned sets held constant); under --eot-size > 1 only with --wb-universal")
    ap.add_argument("--kv-window", dest="kv_window", default=100, type=int, help="--attack kenansville: samples per window (8 .. 128)")
    ap.add_argument("--kv-grid", dest="kv_grid", default=15, type=int, help="--attack kenansville: candidates per round (1 .. 64)")
    ap.add_argument("--kv-max-factor", dest="kv_max_factor", default=1.0, type=float,
                    help="--attack kenansville: the largest share of a window's spectral energy to remove, in (0, 1]")
    ap.add_argument("--hsj-init", dest="hsj_init", default=None, metavar="WAV",
                    help="--attack hsj: the starting audio, one the system already decides as wanted (the target speaker's own "
                         "voice); cropped or tiled to each attacked utterance; an untargeted attack without it starts from noise")
    ap.add_argument("--hsj-grid", dest="hsj_grid", default=15, type=int, help="--attack hsj: rows per search round and step batch (1 .. 64)")
    ap.add_argument("--hsj-evals", dest="hsj_evals", default=(32, 256), type=_int_pair, metavar="B0:BMAX",
                    help="--attack hsj: probes per iteration, min(BMAX, isqrt(B0^2 t)) at iteration t (1 <= B0 <= BMAX <= 1024)")
    ap.add_argument("--hsj-max-queries", dest="hsj_max_queries", default=0, type=int,
                    help="--attack hsj: no batch is scored that would take an attack's rows beyond this many (0: no cap)")
    ap.add_argument("--hsj-sigma-min", dest="hsj_sigma_min", default=2.0 ** -15, type=float,
                    help="--attack hsj: the floor of the probes' standard deviation (default: one int16 step)")
    ap.add_argument("--hsj-probe-scale", dest="hsj_probe_scale", default=0.05, type=float,
                    help="--attack hsj: the probes' standard deviation is this times |x - audio| / sqrt(N) above the floor")
    ap.add_argument("--particles", default=25, type=int, help="--attack pso: particles of the swarm (2 .. 64)")
    ap.add_argument("--pso-w", dest="pso_w", default=(0.9, 0.1), type=_pair, metavar="WI:WE",
                    help="--attack pso: inertia weight, falling linearly from WI to WE over max_iter iterations")
    ap.add_argument("--pso-c", dest="pso_c", default=(1.4961, 1.4961), type=_pair, metavar="C1:C2",
                    help="--attack pso: the pulls towards a particle's own best and the swarm's best")
    ap.add_argument("--pso-vmax", dest="pso_vmax", default=None, type=float,
                    help="--attack pso: largest step of a sample per iteration (default: epsilon)")
    ap.add_argument("--model_dir", default="./model")
    ap.add_argument("--pre_model_dir", default="pre-models")
    ap.add_argument("--test_dir", default="./data/test-set")
    ap.add_argument("--illegal_dir", default="./data/illegal-set")
    ap.add_argument("--out_dir", default=".")
    ap.add_argument("--dist-backend", default=None)
    args = ap.parse_args(argv)
    query_attack = args.attack in ("pso", "kenansville", "hsj")
    if args.query_eot is not None and not query_attack:
        ap.error("--query-eot belongs to --attack pso, kenansville and hsj (--attack %s)" % args.attack)
    if args.attack == "pso" and args.query_eot is None:      # refused here, before any model is built
        if args.eot_size is not None and args.eot_size > 1:
            ap.error("--attack pso does not run under expectation over transformation (--eot-size %d)" % args.eot_size)
        if args.companions > 0:
            ap.error("--attack pso does not take companion utterances (--companions %d)" % args.companions)
    if args.attack == "kenansville" and args.query_eot is None:      # likewise
        if args.eot_size is not None and args.eot_size > 1:
            ap.error("--attack kenansville does not run under expectation over transformation (--eot-size %d)" % args.eot_size)
        if args.companions > 0:
            ap.error("--attack kenansville does not take companion utterances (--companions %d)" % args.companions)
    if args.attack == "hsj":      # likewise
        if args.query_eot is None and args.eot_size is not None and args.eot_size > 1:
            ap.error("--attack hsj does not run under expectation over transformation (--eot-size %d)" % args.eot_size)
        if args.query_eot is None and args.companions > 0:
            ap.error("--attack hsj does not take companion utterances (--companions %d)" % args.companions)
        if args.hsj_init is None and (args.attack_type == "targeted" or args.task == "SV"):
            ap.error("--attack hsj: a targeted attack needs --hsj-init, an audio the system already decides as the target")

    if args.play_offset is not None and args.play_offset != 0:      # likewise: what the library refuses by name is refused here
        if args.attack in ("pso", "kenansville", "hsj", "cw2", "psy"):
            ap.error("--attack %s does not run under a play offset in this version (--play-offset %s)" % (args.attack, args.play_offset))
        if args.attack == "pgd" and not args.wb_universal:
            ap.error("--attack pgd takes --play-offset %s only with --wb-universal (the offset rides on the universal path)" % args.play_offset)
    if args.bpda and args.attack not in ("pgd", "cw2", "psy"):
        ap.error("--bpda belongs to --attack pgd (--attack %s)" % args.attack)
    if args.wb_ivector and args.attack not in ("pgd", "cw2", "psy"):
        ap.error("--wb-ivector belongs to --attack pgd (--attack %s)" % args.attack)
    if args.wb_air and args.attack != "pgd":
        ap.error("--wb-air belongs to --attack pgd (--attack %s)" % args.attack)
    if args.wb_frontend and args.attack != "pgd":
        ap.error("--wb-frontend belongs to --attack pgd (--attack %s)" % args.attack)
    if args.wb_universal and args.attack != "pgd":
        ap.error("--wb-universal belongs to --attack pgd (--attack %s)" % args.attack)
    if args.attack == "pgd":      # likewise: the gradient is that of a GMM-UBM victim, undefended unless --bpda is given
        if args.architecture == "iv" and args.wb_ivector and args.eot_size is not None and args.eot_size > 1 and not args.wb_universal:
            ap.error("--attack pgd --wb-ivector does not run under expectation over transformation (--eot-size %d: an i-vector "
                     "system keeps one row's state)" % args.eot_size)
        if args.architecture != "gmm" and not args.wb_ivector:
            ap.error("--attack pgd differentiates GMM-UBM systems only (--architecture %s)" % args.architecture)
        if args.wb_air and not args.bpda and not args.wb_ivector and args.air_channel is None:
            ap.error("--attack pgd --wb-air belongs to the adaptive attack: give --bpda (GMM-UBM) or --wb-ivector (-archi iv)")
        if not args.bpda and args.eot_size is not None and args.eot_size > 1:
            ap.error("--attack pgd does not run under expectation over transformation (--eot-size %d)" % args.eot_size)
        if args.companions > 0 and not args.wb_universal:
            ap.error("--attack pgd does not take companion utterances (--companions %d)" % args.companions)
        for flag, val in (("--input-transform", args.input_transform), ("--air-channel", args.air_channel),
                          ("--codec", None if args.codec == "none" else args.codec), ("--feco", args.feco), ("--dither", args.dither)):
            if flag == "--air-channel" and val is not None and args.wb_air and (args.wb_ivector if args.architecture == "iv" else args.bpda):
                continue
            if flag in ("--feco", "--dither") and args.wb_frontend:
                continue
            if val is not None and not (args.bpda and flag in ("--input-transform", "--codec")):
                ap.error("--attack pgd attacks an undefended victim: %s %s is not differentiated in this version" % (flag, val))
    if args.attack in ("cw2", "psy"):      # likewise; what fb_attack_cw2 refuses whatever the switches say is refused here by name
        if args.architecture != "gmm" and not args.wb_ivector:
            ap.error("--attack %s differentiates an i-vector system only with --wb-ivector (--architecture %s)" % (args.attack, args.architecture))
        if args.eot_size is not None and args.eot_size > 1 and (not args.bpda or args.architecture != "gmm"):
            ap.error("--attack %s runs under expectation over transformation only with --bpda on a GMM-UBM system "
                     "(--eot-size %d)" % (args.attack, args.eot_size))
        if args.companions > 0:
            ap.error("--attack %s does not take companion utterances in this version (--companions %d)" % (args.attack, args.companions))
        for flag, val in (("--air-channel", args.air_channel), ("--feco", args.feco), ("--dither", args.dither)):
            if val is not None:
                ap.error("--attack %s does not differentiate %s %s in this version" % (args.attack, flag, val))
        for flag, val in (("--input-transform", args.input_transform), ("--codec", None if args.codec == "none" else args.codec)):
            if val is not None and not args.bpda:
                ap.error("--attack %s attacks an undefended victim unless --bpda is given: %s %s" % (args.attack, flag, val))
        from .cw2 import check_cw2_params
        try:
            check_cw2_params(args.cw2_const, args.cw2_steps, args.max_iter, args.cw2_lr, max(args.cw2_abort_every, 1),
                             args.eot_size if args.eot_size is not None else 1, args.bpda)
            if args.cw2_abort_every < 0:
                raise ValueError("CW2: --cw2-abort-every must be >= 0")
            if args.attack == "psy" and not (args.psy_l2_weight >= 0.0 and args.psy_l2_weight < float("inf")):
                raise ValueError("--psy-l2-weight must be finite and >= 0")
        except ValueError as ex:
            ap.error(str(ex))

    task, attack_type, spk_id_list = args.task, args.attack_type, args.speaker_id
    if task == "SV":                      # SV only supports one enrolled speaker (:449-451)
        attack_type, spk_id_list = "targeted", spk_id_list[0:1]
    ident = args.architecture + "-" + task + "-" + attack_type
    out_audio = os.path.join(args.out_dir, "adversarial-audio", ident)
    out_cp = os.path.join(args.out_dir, "checkpoint", ident)
    if task == "SV":
        out_audio, out_cp = os.path.join(out_audio, spk_id_list[0]), os.path.join(out_cp, spk_id_list[0])

    dist = parallel.init_process_group(args.dist_backend)
    rank, _local, world = parallel.dist_env()
    K = max(1, args.streams)
    if model_factory is None:
        model_list = load_spk_models(args.model_dir, spk_id_list, args.architecture)
        kw = {k: v for k, v in (("dither", args.dither), ("input_transform", args.input_transform),
                                       ("feature_compression", args.feco), ("air_channel", args.air_channel),
                                       ("codec", args.codec)) if v is not None}
        model_factory = functools.partial(make_model, **kw) if kw else make_model
    else:
        model_list = spk_id_list
    models = [model_factory(args.architecture, task, model_list, args.pre_model_dir, args.threshold,
                            os.path.join(args.out_dir, ident + ("-%d" % k))) for k in range(K)]
    for m in models:  # (a stub model of the driver-rule tests has no engine)
        if hasattr(m, "engine") and hasattr(m.engine, "set_dither_seed"):
            m.engine.set_dither_seed(args.dither_seed)
        # (under --query-eot the three query attacks set the size themselves, for the length of an attack: the threshold sweep
        #  runs without)
        if args.eot_size is not None and not (query_attack and args.query_eot is not None) and hasattr(m, "engine") and hasattr(m.engine, "set_eot"):
            m.engine.set_eot(args.eot_size)
    if args.play_offset and any(not hasattr(m, "engine") for m in models):   # (as FakeBob refuses eot_size there)
        ap.error("--play-offset applies to the engine's own systems, not to a foreign model")
    if K >= 3:  # several engines share the GPU: the separate launches interleave better (fb_set_fused_chain)
        for m in models:
            if hasattr(m, "engine"):
                m.engine.set_fused_chain(False)
    # one Philox key for the whole job: drawn on rank 0 when --seed is omitted and broadcast, so that a multi-rank
    # run is reproducible and its results do not depend on the sharding
    seed = args.seed if args.seed is not None else (int(np.random.randint(0, 2 ** 31 - 1)) if rank == 0 else 0)
    seed = parallel.broadcast_int(seed, dist)
    hp = dict(adver_thresh=args.adver_thresh, epsilon=args.epsilon, max_iter=args.max_iter, max_lr=args.max_lr,
              min_lr=args.min_lr, samples_per_draw=args.samples_per_draw, sigma=args.sigma,
              momentum=args.momentum, plateau_length=args.plateau_length, plateau_drop=args.plateau_drop)
    if args.attack == "pso":
        hp = dict(adver_thresh=args.adver_thresh, epsilon=args.epsilon, max_iter=args.max_iter, n_particles=args.particles,
                  w_init=args.pso_w[0], w_end=args.pso_w[1], c1=args.pso_c[0], c2=args.pso_c[1], v_max=args.pso_vmax)
    if args.attack == "kenansville":
        hp = dict(window=args.kv_window, grid=args.kv_grid, max_factor=args.kv_max_factor)
    hsj_init = None
    if args.attack == "hsj":
        hp = dict(grid=args.hsj_grid, num_evals_init=args.hsj_evals[0], num_evals_max=args.hsj_evals[1],
                  max_queries=args.hsj_max_queries, sigma_min=args.hsj_sigma_min, probe_scale=args.hsj_probe_scale,
                  max_iter=args.max_iter)
        if args.hsj_init is not None:
            hsj_init = np.asarray(read(args.hsj_init)[1], np.float64).reshape(-1) / (2 ** (bits_per_sample - 1))
    if query_attack and args.query_eot is not None:   # (absent otherwise: a bob_factory sees the keywords it always saw)
        hp.update(eot_size=args.eot_size, quorum=args.query_eot)
    if args.attack == "pgd":
        hp = dict(adver_thresh=args.adver_thresh, epsilon=args.epsilon, max_iter=args.max_iter, max_lr=args.max_lr,
                  min_lr=args.min_lr, momentum=args.momentum, plateau_length=args.plateau_length, plateau_drop=args.plateau_drop)
        if args.bpda:  # (absent otherwise: a bob_factory of the driver-rule tests sees the keywords it always saw)
            hp.update(bpda=True, eot_size=args.eot_size if args.eot_size is not None else 1)
        if args.wb_ivector and not args.wb_universal:  # IvectorPGD has no eot_size without universal=True
            hp.pop("eot_size", None)
        if args.wb_air:
            hp.update(air=True)
        if args.wb_frontend:
            hp.update(frontend=True)
            if not args.bpda and not args.wb_ivector:  # (AdaptivePGD's default is bpda=True)
                hp.update(bpda=False)
        if args.wb_universal:
            hp.update(universal=True)
            if not args.bpda and not args.wb_ivector:
                hp.update(bpda=False)
    if args.attack in ("cw2", "psy"):
        hp = dict(confidence=args.adver_thresh, initial_const=args.cw2_const, binary_search_steps=args.cw2_steps,
                  max_iter=args.max_iter, lr=args.cw2_lr, stop_early=args.cw2_abort_every > 0,
                  stop_early_iter=max(args.cw2_abort_every, 1))
        if args.bpda:
            hp.update(bpda=True, eot_size=args.eot_size if args.eot_size is not None else 1)
        if args.wb_ivector:
            hp.update(ivector=True)
    if bob_factory is None and args.attack == "psy":
        from .psy import Imperceptible
        bobs = [Imperceptible(task, attack_type, m, window=args.psy_window, l2_weight=args.psy_l2_weight, seed=seed, verbose=False, **hp)
                for m in models]
    elif bob_factory is None and args.attack == "cw2":
        from .cw2 import CW2
        bobs = [CW2(task, attack_type, m, seed=seed, verbose=False, **hp) for m in models]
    elif bob_factory is None and args.attack == "pgd" and args.wb_ivector:
        from .pgd import IvectorPGD
        bobs = [IvectorPGD(task, attack_type, m, seed=seed, verbose=False, **hp) for m in models]
    elif bob_factory is None and args.attack == "pgd":
        from .pgd import PGD, AdaptivePGD
        bobs = [(AdaptivePGD if (args.bpda or args.wb_frontend or args.wb_universal) else PGD)(task, attack_type, m, seed=seed, verbose=False, **hp) for m in models]
    elif bob_factory is None and args.attack == "kenansville":
        from .kenansville import Kenansville
        bobs = [Kenansville(task, attack_type, m, seed=seed, verbose=False, **hp) for m in models]
    elif bob_factory is None and args.attack == "hsj":
        from .hsj import HopSkipJump
        bobs = [HopSkipJump(task, attack_type, m, seed=seed, verbose=False, **hp) for m in models]
    elif bob_factory is None and args.attack == "pso":
        from .pso import ParticleSwarm
        bobs = [ParticleSwarm(task, attack_type, m, seed=seed, verbose=False, **hp) for m in models]
    elif bob_factory is None:
        bobs = [FakeBob(task, attack_type, m, seed=seed, verbose=False, **hp) for m in models]
    else:
        bobs = [bob_factory(task, attack_type, m, **hp) for m in models]

    items = build_attack_list(task, attack_type, models[0], args.test_dir, args.illegal_dir, out_audio, out_cp)
    total = len(items)
    if rank == 0:
        print("------ load data done, total num: %d ------" % total)
    for it in items:
        os.makedirs(os.path.dirname(it["wav_path"]), exist_ok=True)
        os.makedirs(os.path.dirname(it["cp_path"]), exist_ok=True)

    threshold = 0.
    if task != "CSI" and total > 0:       # estimate the threshold on one random voice (:355-357, :393-394)
        thr = None
        if rank == 0:
            pick = items[int(np.random.choice(total, 1)[0])]["audio"]
            thr, _, _ = bobs[0].estimate_threshold(pick, fs=fs, bits_per_sample=bits_per_sample)
        threshold = parallel.broadcast_threshold(thr, dist)

    # every attack stream of every rank draws the next global attack index when it is free (attack cost ranges from one
    # iteration -- early stop, FAKEBOB.py:181-191 -- to max_iter); --schedule static: round-robin over ranks and streams
    queue = parallel.WorkQueue(total, dist, args.schedule, streams=K)
    results = {}
    lock = threading.Lock()
    errors = []

    def worker(k):
        try:
            run_stream(k)
        except BaseException as ex:  # noqa: BLE001  (re-raised below: a dead stream must not look like a short list)
            errors.append(ex)

    def run_stream(k):
        bob = bobs[k]
        while True:
            idx = queue.next(k)
            if idx is None:
                return
            it = items[idx]
            bob._stream = idx + 1         # Philox stream = global attack index: results do not depend on the sharding
            audio_c, comp = with_companions(items, idx, args.companions) if args.companions > 0 else (it["audio"], None)
            if args.play_offset:          # ('max': N - 1 of THIS utterance, cropped as --companions crops; fixed otherwise)
                set_play_offset(bob, args.play_offset, len(audio_c))
            # the reference passes true= only for CSI untargeted (:346) and target= only for targeted attacks (:332,:367)
            true = it["true"] if (task == "CSI" and attack_type == "untargeted") else None
            extra = dict(init=hsj_init) if args.attack == "hsj" else {}
            if args.companions > 0:
                audio = audio_c
                if hasattr(bob, "attack_universal"):   # (the PGD classes: PGD.attack keeps FakeBob.attack's plain signature)
                    res = bob.attack_universal(audio, it["cp_path"], comp, threshold=threshold, true=true, target=it["target"],
                                               fs=fs, bits_per_sample=bits_per_sample)
                    adv, flag = res
                else:
                    res = bob.attack(audio, it["cp_path"], threshold=threshold, true=true, target=it["target"], fs=fs,
                                     bits_per_sample=bits_per_sample, companions=comp, **extra)
                    adv, flag = res
                    print_votes(args.attack, it["name"], flag, res)
                print_offsets(it["name"], res)
                write(it["wav_path"], fs, adv)
                with lock:
                    results[idx] = flag
                continue
            res = bob.attack(it["audio"], it["cp_path"], threshold=threshold, true=true,
                             target=it["target"], fs=fs, bits_per_sample=bits_per_sample, **extra)
            adv, flag = res
            print_votes(args.attack, it["name"], flag, res)
            print_offsets(it["name"], res)
            if args.attack == "psy" and hasattr(res, "best_dist"):
                print("psy %s: success %d, dist %.6g, over %d, l2 %.6g, snr %.2f dB, c %.3g" %
                      (it["name"], flag, res.best_dist, res.n_over, res.best_l2, res.snr_db, res.const))
            if args.attack == "cw2" and hasattr(res, "best_l2"):   # the figure this attack is run for
                print("cw2 %s: success %d, l2 %.6g, snr %.2f dB, c %.3g" % (it["name"], flag, res.best_l2, res.snr_db, res.const))
            write(it["wav_path"], fs, adv)
            with lock:
                results[idx] = flag

    ths = [threading.Thread(target=worker, args=(k,)) for k in range(K)]
    [t.start() for t in ths]
    [t.join() for t in ths]
    if parallel.agree_on_failure(bool(errors), dist):   # every rank learns of it BEFORE the result reduction
        if errors:
            raise errors[0]
        raise RuntimeError("an attack stream of another rank failed: the job's results are incomplete")
    st = [m.engine.stats() if hasattr(m, "engine") else dict(nes_iters=0, scored_utts=0) for m in models]
    succ = sum(1 for f in results.values() if f == 1)
    g = parallel.reduce_counters([succ, len(results), sum(s["nes_iters"] for s in st), sum(s["scored_utts"] for s in st)], dist)
    if g[1] != total:
        raise RuntimeError("the work queue handed out %d of %d attacks" % (g[1], total))
    if rank == 0:
        if g[1] > 0:
            print('------ attack successful rate %d ------' % (g[0] * 100 / g[1]))
        print("----- generate adversarial voices done: %d attacks, %d NES iterations, %d utterances scored -----"
              % (g[1], g[2], g[3]))
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()
    return g, results, threshold


if __name__ == "__main__":
    main()
