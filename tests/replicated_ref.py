"""What the device must have computed for EVERY row of a replicated NES batch (fb_set_eot, fb_set_companions, dither and
feature compression inside fb_get_grad / fb_attack), put together on the host from paths that know nothing of replication.
Written from the contract text of include/fakebob_hip.h ("Row order", "Averaging", the dither, noise and FeCo RNG contracts):

    replica rho = u * eot + j of NES row b   ->   row b * K * eot + rho of the batch the front end scores
    noise stages  draw with (utterance row b, replica rho)            -- the row of the UN-replicated batch
    FeCo          draws with (utterance row b, replica rho)           -- likewise
    dither        draws with utterance index b * K * eot + rho        -- the REPLICATED row
    loss[b]     = (l[b][0] + ... + l[b][K eot - 1]) / (K eot)         float64, rho ascending; scores[b][s] likewise

The pieces: the NES rows q[B][N] are the engine's own batch builder seen through fb_get_grad_ext's callback (pinned by
tests/test_gpu_plugin_api.py); composition and chain are tests/companions_ref.compose; a replica's raw scores come from an
ordinary scoring call (or, for dither and FeCo, from the front end's debug hooks, tests/feco_ref and per-frame
log-likelihoods averaged in float64); a replica's loss is the CPU oracle's loss_fn; the means are
companions_ref.mean_over_replicas.  Nothing here reads the engine's replicated buffers."""
import numpy as np

from fakebob_amd import companions as CP
from fakebob_amd.engine import nes_params
from tests import companions_ref as R
from tests.feco_ref import feco

SCORE_BATCH = 64        # rows per scoring call of the reference: far from any replicated batch's shape


def flat_row(b, u, j, K, r):
    """The row of replica (utterance u, draw j) of NES row b in the batch the front end scores"""
    assert 0 <= u < K and 0 <= j < r
    return b * K * r + u * r + j


def replica_word(u, j, r):
    """rho, the `replica` of the noise and FeCo contracts"""
    return u * r + j


def nes_rows(bare, p, audio, it=0):
    """q[B][N] int16: the rows the engine's batch builder makes for (seed, stream, it) of p around `audio`, taken from the
    callback of fb_get_grad_ext on an engine that has no system, chain, companions or EOT (`bare`)."""
    audio = np.ascontiguousarray(audio, np.float64).reshape(-1)
    seen = []

    def score(a):                       # (N, B) float64 -> (B, 1)
        seen.append(np.array(a, np.float64))
        return np.zeros((a.shape[1], 1))
    cap = nes_params("SV", "targeted", samples_per_draw=p.samples_per_draw, sigma=p.sigma, seed=p.seed, stream=p.stream,
                     bits_per_sample=p.bits_per_sample or 16)
    bare.get_grad_ext(cap, 1, score, audio, it=it)
    assert len(seen) == 1
    batch = seen[0]
    B = 2 * (p.samples_per_draw // 2) + 1
    assert batch.shape == (audio.size, B)
    q = np.stack([CP.cast_i16(batch[:, b], p.bits_per_sample or 16) for b in range(B)])
    assert np.array_equal(q[0], CP.cast_i16(audio, p.bits_per_sample or 16))      # column 0: the unperturbed audio
    return q


def composed_rows(q, a0, comp, chain, r, normals):
    """[B][K][r][N] int16 (companions_ref.compose); comp None: K = 1"""
    comp = np.zeros((0, q.shape[1]), np.int16) if comp is None else np.asarray(comp)
    return R.compose(q, a0, comp, _tuples(chain), r, normals)


def _tuples(chain):
    return [(st[0], st[1], st[2]) for st in (chain or [])]


def device_normals(bare, p, it, n):
    """normals(b, rho, s) of the noise contract at (seed, stream, it) of p, from the generator's own hook"""
    return lambda b, rho, s: bare.debug_tf_noise(p.seed, p.stream, it, b, rho, s, 0, n)


def replica_losses(oracle, lossdef, sc):
    """FakeBob.loss_fn (the CPU oracle's, pinned to the reference's goldens) of score rows sc[..., S] -> [...]"""
    sc = np.asarray(sc, np.float64)
    flat = sc.reshape(-1, sc.shape[-1])
    out = oracle.loss(lossdef["task"], lossdef["attack"], flat, threshold=lossdef.get("threshold", 0.0),
                      adver_thresh=lossdef.get("adver_thresh", 0.0), target=lossdef.get("target"), true=lossdef.get("true"))
    return out.reshape(sc.shape[:-1])


def averages(rep_l, rep_sc):
    """rep_l [B][R], rep_sc [B][R][S] -> loss[B], scores[B][S]: the contract's mean over the replicas, rho ascending"""
    rep_l, rep_sc = np.asarray(rep_l, np.float64), np.asarray(rep_sc, np.float64)
    return R.mean_over_replicas(rep_l), R.mean_over_replicas(np.swapaxes(rep_sc, 1, 2))


def _score_rows(scorer, rows):
    """raw[rows][M], tv[rows] of int16 rows by ordinary scoring calls of at most SCORE_BATCH utterances"""
    raw, tv = [], []
    for i in range(0, len(rows), SCORE_BATCH):
        a, t = scorer.score_raw([np.ascontiguousarray(w) for w in rows[i:i + SCORE_BATCH]])
        raw.append(a)
        tv.append(t)
    return np.concatenate(raw), np.concatenate(tv)


def _frames_mean(scorer, feats):
    return scorer.debug_gmm_frames(feats).astype(np.float64).mean(axis=1)


def raw_scores(scorer, rows, mode, p, it, K, r, feco_cfg=None, keys=None):
    """Per-replica raw scores of the composed rows [B][K][r][N] -> raw[B * K * r][M], tv[B * K * r], in flat-row order.
    mode "score": scoring calls on `scorer` (no chain, companions or EOT: the rows ARE what the MFCC reads).
    mode "dither": fb_debug_feats_dither at the row's point of the dither contract (utterance index = the replicated row)
    -> per-frame log-likelihoods -> float64 mean.  mode "feco": fb_debug_feats -> tests/feco_ref with keys(b, rho, T) ->
    per-frame log-likelihoods of the centres -> float64 mean."""
    B = rows.shape[0]
    assert rows.shape[1:3] == (K, r)
    BR = B * K * r
    if mode == "score":
        flat = np.empty((BR, rows.shape[-1]), np.int16)
        for b in range(B):
            for u in range(K):
                for j in range(r):
                    flat[flat_row(b, u, j, K, r)] = rows[b, u, j]
        return _score_rows(scorer, list(flat))
    raw, tv = [None] * BR, np.zeros(BR, np.int32)
    for b in range(B):
        for u in range(K):
            for j in range(r):
                row = flat_row(b, u, j, K, r)
                w = rows[b, u, j]
                if mode == "dither":
                    feats, _T = scorer.debug_feats_dither(w, p.seed, p.stream, it, row)
                else:
                    assert mode == "feco"
                    feats, _T = scorer.debug_feats(w)
                tv[row] = feats.shape[0]
                if feats.shape[0] == 0:
                    raise ValueError("row %d (b %d, u %d, j %d) has no voiced frames: choose other inputs" % (row, b, u, j))
                if mode == "feco":
                    ratio, iters = feco_cfg
                    feats, _labels = feco(feats, keys(b, replica_word(u, j, r), feats.shape[0]), ratio, iters)
                raw[row] = _frames_mean(scorer, feats)
    return np.stack(raw), tv


def reference(oracle, bare, scorer, p, audio, lossdef, comp=None, chain=None, r=1, mode="score", feco_cfg=None, it=0):
    """-> dict(q, rows [B][K][r][N], rep_sc [B][R][S], rep_l [B][R], loss [B], scores [B][S], tv [B * R]) for the NES batch
    of (p, audio, it) on a system whose `scorer` engine holds the models (and, for mode "dither", the dither)."""
    n = np.asarray(audio).size
    q = nes_rows(bare, p, audio, it)
    a0 = q[0]
    K = 1 if comp is None else np.asarray(comp).shape[0] + 1
    rows = composed_rows(q, a0, comp, chain, r, device_normals(bare, p, it, n))
    B, R_ = q.shape[0], K * r
    keys = (lambda b, rho, T: bare.debug_feco_keys(p.seed, p.stream, it, b, rho, T)) if mode == "feco" else None
    raw, tv = raw_scores(scorer, rows, mode, p, it, K, r, feco_cfg, keys)
    if not np.all(tv > 0):
        raise ValueError("rows without voiced frames: %s" % np.flatnonzero(tv <= 0)[:8])
    sc = scorer.system_scores(raw)
    rep_sc = sc.reshape(B, R_, sc.shape[1])
    rep_l = replica_losses(oracle, lossdef, rep_sc)
    loss, scores = averages(rep_l, rep_sc)
    return dict(q=q, rows=rows, rep_sc=rep_sc, rep_l=rep_l, loss=loss, scores=scores, tv=tv, K=K, r=r)


def swap_replicas(ref, b1, b2):
    """The reference with the replicas of rows b1 and b2 exchanged -> (loss, scores): what a batch whose row index slipped
    between those two rows would average to"""
    rep_l, rep_sc = ref["rep_l"].copy(), ref["rep_sc"].copy()
    rep_l[[b1, b2]] = rep_l[[b2, b1]]
    rep_sc[[b1, b2]] = rep_sc[[b2, b1]]
    return averages(rep_l, rep_sc)


# ---- the choice of inputs, checked without a device
def host_nes_rows(oracle, spd, sigma, seed, stream, audio, it=0):
    """q[B][N] from the CPU oracle's batch builder at the same (seed, stream, it): the batch its get_grad hands its scorer"""
    audio = np.ascontiguousarray(audio, np.float64).reshape(-1)
    seen = []

    def score(a):
        seen.append(np.array(a, np.float64))
        return np.zeros((a.shape[1], 1))
    po = oracle.nes_params("SV", "targeted", 1, samples_per_draw=spd, sigma=sigma)
    fn = oracle.py_score_fn(score, 1)
    oracle.get_grad(po, fn, None, audio, seed=seed, it=it, stream=stream)
    return np.stack([CP.cast_i16(seen[0][:, b]) for b in range(seen[0].shape[1])])


def host_voiced_counts(oracle, cfg, q, comp, chain, r, normals):
    """tv of every composed row [B * K * r] from the oracle's front end (no dither: the VAD's count of the undithered row)"""
    rows = composed_rows(q, q[0], comp, chain, r, normals)
    flat = rows.reshape(-1, rows.shape[-1])
    return np.array([oracle.frontend(cfg, w)[0].shape[0] for w in flat], np.int32)


# ---- the cases of tests/test_gpu_replicated_batches.py (here, so that the choice of inputs is checked on the CPU too)
SEED, STREAM, IT = 11, 6, 0
THR, ADV_THR = 0.1, 0.05
# name -> system, task, samples_per_draw, K, eot, chain spec, samples, mode, rows the front end scores
CASES = {
    "calibration": dict(system="gmm", task="OSI", spd=50, K=1, eot=1, chain=None, n=4000, mode="score", rows=51),
    "recipe-eot": dict(system="gmm", task="OSI", spd=50, K=1, eot=4, chain="at:20", n=4000, mode="score", rows=204),
    "full-replicas": dict(system="gmm", task="OSI", spd=50, K=8, eot=4, chain="noise:20", n=4000, mode="score", rows=1632),
    "below-256": dict(system="gmm", task="SV", spd=50, K=1, eot=5, chain="at:20", n=4000, mode="score", rows=255),
    "above-256": dict(system="gmm", task="SV", spd=52, K=1, eot=5, chain="at:20", n=4000, mode="score", rows=265),
    "large-B": dict(system="gmm8", task="CSI", spd=256, K=1, eot=2, chain="noise:20", n=4000, mode="score", rows=514),
    "ivector": dict(system="ivector", task="SV", spd=50, K=2, eot=2, chain="at:20", n=4000, mode="score", rows=204),
    "long": dict(system="gmm", task="OSI", spd=6, K=2, eot=2, chain="ms:7,qt:512", n=48400, mode="score", rows=28),
    "feco": dict(system="gmm", task="OSI", spd=6, K=2, eot=2, chain=None, n=4000, mode="feco", rows=28),
    "dither": dict(system="gmm", task="OSI", spd=6, K=2, eot=2, chain=None, n=4000, mode="dither", rows=28),
}
FECO_CFG = (0.5, 10)
DITHER = 1.0


def case_lossdef(case):
    d = dict(task=case["task"], attack="targeted", threshold=THR, adver_thresh=ADV_THR)
    if case["task"] == "OSI":
        d["target"] = 1
    elif case["task"] == "CSI":
        d["target"] = 2
    return d


def case_params(case):
    d = case_lossdef(case)
    return nes_params(d["task"], d["attack"], samples_per_draw=case["spd"], threshold=d["threshold"],
                      adver_thresh=d["adver_thresh"], target=d.get("target"), seed=SEED, stream=STREAM)


def case_audio(case):
    """(the attacked audio, the companions (K - 1, n) int16 or None): utterance 9 and utterances 20 and up"""
    from fakebob_amd.models import synthetic_audio
    n, K = case["n"], case["K"]
    comp = np.stack([CP.cast_i16(synthetic_audio(20 + u, n)) for u in range(K - 1)]) if K > 1 else None
    return synthetic_audio(9, n), comp
