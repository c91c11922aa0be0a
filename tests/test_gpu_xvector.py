"""x-vector (TDNN) systems on the device (include/fakebob_hip.h, "x-vector"): the chain on handed-in rows against the CPU
restatements of tests/xvector_ref.py, the two contract properties (a run repeats, an embedding does not depend on its batch) to
the bit, scoring, the NES loss against per-row scoring calls to the bit, whole attacks, and the refusals.

Shapes: the stock five contexts with hidden 64, pool 96, R 64, L 32, S 3 on the default front end with delta_order = 0
(5 * D is no multiple of 16); hidden 96 (three column tiles: the fourth wave of a workgroup idles); one layer; hidden 76 and
pool 100 (partial column tiles, and inputs whose width is no multiple of 8: the element-wise gather).  A batch of
lengths {1, 2, 15, 31, 32, 33, 70} is 184 rows: two row tiles of 128, with utterance boundaries inside both.

Accuracy: err = max |x - ref64| / max |ref64| per stage, for the device (err_dev) and for the float32 restatement (err_32);
err_dev <= 4 * err_32, the factor for another summation order at equal precision.  Both figures are printed."""
import ctypes as C
import pickle

import numpy as np
import pytest
import torch

from fakebob_amd import _native as N
from fakebob_amd import companions as CP
from fakebob_amd import input_transform as T
from fakebob_amd.attack import FakeBob
from fakebob_amd.engine import Engine, cw2_params, nes_params, psy_params
from fakebob_amd.hsj import HopSkipJump
from fakebob_amd.kenansville import Kenansville
from fakebob_amd.models import STOCK_XV_CONTEXTS, synthetic_audio, synthetic_xvector_system
from fakebob_amd.pso import ParticleSwarm
from fakebob_amd.systems import xv_CSI, xv_OSI, xv_SV
from tests import replicated_ref as RR
from tests import xvector_ref as ref

pytestmark = pytest.mark.gpu
LENGTHS = [33, 1, 70, 2, 32, 15, 31]
BACKEND_TOL = 1e-7     # the i-vector back end against the oracle at equal i-vectors (tests/test_gpu_ivector.py)
Z_MEAN, Z_STD = [-30.0, -50.0, -20.0], [5.0, 8.0, 4.0]
SHAPES = {"stock": dict(hidden=64), "hidden96": dict(hidden=96), "one-layer": dict(contexts=(STOCK_XV_CONTEXTS[0],)),
          "partial-tiles": dict(hidden=76, pool=100)}


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    e.set_frontend(delta_order=0)
    yield e
    e.close()


def _system(D, hidden=64, contexts=STOCK_XV_CONTEXTS, n_speakers=3, seed=11, pool=96):
    sy = synthetic_xvector_system(D, hidden=hidden, pool=pool, R=64, L=32, n_speakers=n_speakers, seed=seed, contexts=contexts)
    return sy.with_enrolled(sy.enrolled, Z_MEAN[:n_speakers], Z_STD[:n_speakers])


def _ranged(sy):
    """layer 1's bn_scale * 4096, layer 2's weights * 2^-12: values far outside f16's range between them"""
    layers = [dict(ly) for ly in sy.layers]
    layers[1]["bn_scale"] = layers[1]["bn_scale"] * np.float32(4096.0)
    layers[2]["W"] = layers[2]["W"] * np.float32(2.0 ** -12)
    return type(sy)(sy.D, layers, sy.seg_W, sy.seg_bias, sy.mean_vec, sy.lda, sy.plda_mean, sy.plda_transform, sy.plda_psi,
                    sy.enrolled, sy.z_mean, sy.z_std)


def _rows(D, lengths=LENGTHS, seed=3):
    rng = np.random.default_rng(seed)
    return [(3.0 * rng.normal(size=(t, D))).astype(np.float32) for t in lengths]


_REFS = {}


def _refs(name, sy, mats):
    """the two restatements of every utterance, once per system: lists of (layer outputs, statistics, embedding)"""
    if name not in _REFS:
        _REFS[name] = ([ref.stages(sy, m) for m in mats], [ref.stages(sy, m, torch.float32) for m in mats])
    return _REFS[name]


def _stage(per_utt, s, n_layers):
    """stage s of every utterance, concatenated: s < n_layers a layer's rows, then the statistics, then the embeddings"""
    if s < n_layers:
        return np.concatenate([u[0][s] for u in per_utt], axis=0)
    return np.stack([u[1] if s == n_layers else u[2] for u in per_utt])


def _check_accuracy(eng, name, sy):
    mats = _rows(sy.D)
    r64, r32 = _refs(name, sy, mats)
    eng.load_xvector(sy, "OSI")
    nl = len(sy.layers)
    worst = 0.0
    for s in range(nl + 2):
        dev = eng.debug_xv_embed(mats, s)
        dev = np.concatenate(dev, axis=0).astype(np.float64) if s < nl else dev
        want, f32 = _stage(r64, s, nl), _stage(r32, s, nl)
        assert dev.shape == want.shape and np.all(np.isfinite(dev))
        scale = np.abs(want).max()
        err_dev, err_32 = np.abs(dev - want).max() / scale, np.abs(f32 - want).max() / scale
        print("%s stage %d (%s): err_dev %.3g err_32 %.3g ratio %.2f" %
              (name, s, "layer" if s < nl else ("statistics", "embedding")[s - nl], err_dev, err_32, err_dev / err_32))
        assert err_32 > 0.0
        assert err_dev <= 4.0 * err_32, (name, s, err_dev, err_32)
        worst = max(worst, err_dev / err_32)
    return worst


# ------------------------------------------------------------------------------------------------ 1, 2: accuracy, range
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_accuracy_of_every_stage(eng, name):
    _check_accuracy(eng, name, _system(eng.feat_dim, **SHAPES[name]))


def test_accuracy_with_values_outside_f16s_range(eng):
    sy = _ranged(_system(eng.feat_dim))
    outs, _, _ = ref.stages(sy, _rows(sy.D)[2])
    assert np.abs(outs[1]).max() > 65504.0 and np.abs(sy.layers[2]["W"]).max() < 2.0 ** -10     # the case is what it says
    _check_accuracy(eng, "ranged", sy)


# ------------------------------------------------------------------------------------------------ 3: batch independence
@pytest.mark.parametrize("name", ["stock", "hidden96", "partial-tiles"])
def test_an_embedding_does_not_depend_on_its_batch(eng, name):
    sy = _system(eng.feat_dim, **SHAPES[name])
    eng.load_xvector(sy, "OSI")
    mats = _rows(sy.D)
    nl = len(sy.layers)
    full = eng.debug_xv_embed(mats, nl + 1)
    stats = eng.debug_xv_embed(mats, nl)
    assert np.array_equal(full, eng.debug_xv_embed(mats, nl + 1))           # a run repeats
    assert np.array_equal(stats, eng.debug_xv_embed(mats, nl))
    other = _rows(sy.D, [5, 40, 129, 7], seed=9)
    for i, m in enumerate(mats):
        alone = eng.debug_xv_embed([m], nl + 1)[0]
        first = eng.debug_xv_embed([m] + other, nl + 1)[0]
        last = eng.debug_xv_embed(other + [m], nl + 1)[-1]
        between = eng.debug_xv_embed(other[:2] + [m] + other[2:], nl + 1)[2]
        for what, got in (("alone", alone), ("first", first), ("last", last), ("between", between)):
            assert np.array_equal(got, full[i]), (name, i, m.shape[0], what, np.abs(got - full[i]).max())
        assert np.array_equal(eng.debug_xv_embed(other + [m], nl)[-1], stats[i])
    # every layer's rows too: utterance 2 (70 rows) behind 129 others starts in the middle of a row tile
    for s in range(nl):
        a = eng.debug_xv_embed([mats[2]], s)[0]
        b = eng.debug_xv_embed([other[2], mats[2]], s)[1]
        assert np.array_equal(a, b), (name, s)
    assert len({full[i].tobytes() for i in range(len(mats))}) == len(mats)  # (the utterances differ)


# ------------------------------------------------------------------------------------------------ 4: scores, decisions
def _wav(utt, n):
    return CP.cast_i16(synthetic_audio(utt, n), 16)


def test_scores_are_the_back_end_of_the_devices_embeddings(eng):
    sy = _system(eng.feat_dim)
    eng.load_xvector(sy, "OSI")
    wavs = [_wav(0, 16000), _wav(1, 5000), _wav(2, 9000), _wav(3, 2000)]
    llr, tv = eng.score_raw(wavs)
    assert np.all(tv > 0)
    emb = eng.last_ivectors(len(wavs), sy.R)
    want = ref.plda_llr(sy, emb)
    print("LLR against the numpy back end: %.3g" % np.abs(llr - want).max())
    assert np.abs(llr - want).max() <= BACKEND_TOL
    assert np.allclose(eng.system_scores(llr), (llr - sy.z_mean) / sy.z_std, rtol=0, atol=1e-12)
    # the scoring path runs the chain of the hook on the front end's own rows
    feats = [eng.debug_feats(w)[0] for w in wavs]
    assert [f.shape[0] for f in feats] == list(tv)
    assert np.array_equal(eng.debug_xv_embed(feats, len(sy.layers) + 1), emb)
    # ... and that embedding is the contract's function of those rows
    e64 = np.stack([ref.stages(sy, f)[2] for f in feats])
    e32 = np.stack([ref.stages(sy, f, torch.float32)[2] for f in feats])
    err_dev, err_32 = np.abs(emb - e64).max() / np.abs(e64).max(), np.abs(e32 - e64).max() / np.abs(e64).max()
    print("embeddings of scored audio: err_dev %.3g err_32 %.3g" % (err_dev, err_32))
    assert err_dev <= 4.0 * err_32
    llr2, _ = eng.score_raw(wavs[::-1])
    assert np.array_equal(llr2[::-1], llr)


def test_make_decisions_of_the_three_classes(eng, tmp_path):
    sy = _system(eng.feat_dim)
    d = str(tmp_path)
    ml = [["spk%d" % i, "utt%d" % i, sy.enrolled[i].copy(), Z_MEAN[i], Z_STD[i]] for i in range(3)]
    wavs = [_wav(u, 6000) for u in range(4)]
    csi = xv_CSI(d + "/csi", ml, pre_model_dir=d, engine=eng, system=sy)
    dec, sc = csi.make_decisions(wavs)
    assert sc.shape == (4, 3) and dec == [int(np.argmax(s)) for s in sc]
    thr = float(np.sort(sc.max(axis=1))[1:3].mean())                        # two voices below, two above
    osi = xv_OSI(d + "/osi", ml, pre_model_dir=d, threshold=thr, engine=eng, system=sy)
    dec_o, sc_o = osi.make_decisions(wavs)
    assert np.array_equal(sc_o, sc)
    assert dec_o == [(-1 if s.max() < thr else int(np.argmax(s))) for s in sc] and sorted(set(dec_o))[0] == -1 and max(dec_o) >= 0
    one, sc1 = osi.make_decisions(wavs[0])
    assert one == dec_o[0] and np.array_equal(sc1, sc[0])
    sv = xv_SV(d + "/sv", ml[1], pre_model_dir=d, threshold=float(np.median(sc[:, 1])), engine=eng, system=sy)
    dec_s, sc_s = sv.make_decisions(wavs)
    assert np.array_equal(sc_s, sc[:, 1]) and dec_s == [1 if s >= sv.threshold else -1 for s in sc[:, 1]]
    assert sorted(set(dec_s)) == [-1, 1]
    with pytest.raises(TypeError):
        xv_SV(d + "/sv", ml[1], pre_model_dir=d, engine=eng, system=sy, feature_compression="0.5")


# ------------------------------------------------------------------------------------------------ 5: NES, to the bit
def _captured_rows(bare, p, audio, noise):
    seen = []

    def score(a):
        seen.append(np.array(a, np.float64))
        return np.zeros((a.shape[1], 1))
    cap = nes_params("SV", "targeted", samples_per_draw=p.samples_per_draw, sigma=p.sigma, seed=p.seed, stream=p.stream)
    bare.get_grad_ext(cap, 1, score, audio, it=0, noise_pos=noise)
    return np.stack([CP.cast_i16(seen[0][:, b], 16) for b in range(seen[0].shape[1])])


@pytest.mark.parametrize("n,eot", [(1000, 1), (2000, 1), (1500, 2)])
def test_nes_loss_is_the_loss_of_per_row_scoring_calls(oracle, n, eot):
    """fb_get_grad with handed-in noise: score0, the adversarial loss and the mean loss of the perturbed rows equal -- bit for
    bit -- the loss function applied in numpy to ordinary scoring calls of the composed int16 rows, scored one by one (an
    embedding does not depend on its batch).  eot = 2: behind a noise stage, against the mean over the two replicas."""
    bare, scorer, d = Engine(0), Engine(0), Engine(0)
    try:
        for e in (scorer, d):
            e.set_frontend(delta_order=0)
            e.load_xvector(_system(e.feat_dim), "OSI")
        audio = synthetic_audio(9, n)
        lossdef = dict(task="OSI", attack="targeted", threshold=0.1, adver_thresh=0.05, target=1)
        p = nes_params("OSI", "targeted", samples_per_draw=4, threshold=0.1, adver_thresh=0.05, target=1, seed=11, stream=6)
        noise = np.random.default_rng(n).normal(size=(n, 2))
        q = _captured_rows(bare, p, audio, noise)
        assert q.shape == (5, n)
        chain = T.parse("noise:20") if eot > 1 else []
        rows = RR.composed_rows(q, q[0], None, chain, eot, RR.device_normals(bare, p, 0, n))    # [5][1][eot][n]
        raw = np.stack([scorer.score_raw([np.ascontiguousarray(rows[b, 0, j])])[0][0] for b in range(5) for j in range(eot)])
        sc = scorer.system_scores(raw).reshape(5, eot, -1)
        loss, scores = RR.averages(RR.replica_losses(oracle, lossdef, sc), sc)
        if eot > 1:
            d.set_input_transform(chain)
            d.set_eot(eot)
        fl, _g, al, sc0 = d.get_grad(p, audio, it=0, noise_pos=noise, want_grad=False)
        assert np.ptp(loss) > 0.0
        assert np.array_equal(np.asarray(sc0)[:3], scores[0]), (sc0, scores[0])
        assert al == loss[0], (al, loss[0])
        assert fl == oracle.np_sum(loss[1:]) / 4.0, (fl, loss)
    finally:
        for e in (bare, scorer, d):
            e.close()


# ------------------------------------------------------------------------------------------------ 6: whole attacks
N_ATT = 4000


def _sv_setting(tmp_path, **kw):
    """an xv_SV system on an engine of its own and (the attacked voice, an accepted voice, the threshold between them)"""
    e = Engine(0)
    e.set_frontend(delta_order=0)
    sy = _system(e.feat_dim, n_speakers=1)
    d = str(tmp_path)
    model = xv_SV(d + "/sv", ["spk0", "utt0", sy.enrolled[0].copy(), -40.0, 10.0], pre_model_dir=d, threshold=0.0, engine=e, system=sy, **kw)
    voices = [synthetic_audio(u, N_ATT) for u in range(4)]
    sc = np.array([model.score(CP.cast_i16(v, 16)) for v in voices])
    lo, hi = int(np.argmin(sc)), int(np.argmax(sc))
    assert sc[hi] - sc[lo] > 1e-3
    model.threshold = float(sc[lo] + 0.05 * (sc[hi] - sc[lo]))
    return model, voices[lo], voices[hi], model.threshold


def _agrees(model, adv, flag):
    """a success flag is the system's own decision on the returned audio (flag -1: the last iterate was never scored)"""
    assert flag in (1, -1)
    if flag == 1:
        dec, _sc = model.make_decisions(np.asarray(adv).reshape(-1))
        assert dec == 1, (dec, flag)


@pytest.mark.parametrize("defended", [False, True])
def test_fakebob_lowers_the_loss_and_the_flag_is_the_decision(tmp_path, defended):
    kw = dict(input_transform="qt:512", codec="ulaw") if defended else {}
    model, audio, _init, thr = _sv_setting(tmp_path, **kw)
    try:
        fb = FakeBob("SV", "targeted", model, max_iter=12 if defended else 30, samples_per_draw=10, epsilon=0.004, max_lr=0.002, seed=3, verbose=False)
        ck = str(tmp_path / "trace.pkl")
        adv, flag = fb.attack(audio, ck, threshold=thr)
        with open(ck, "rb") as f:
            trace = pickle.load(f)
        losses = [float(np.asarray(r[1]).reshape(-1)[0]) for r in trace]
        print("x-vector SV%s: adversarial loss %s, flag %d" % (" behind qt:512 + mu-law" if defended else "", ["%.4g" % v for v in losses], flag))
        assert losses[0] > 0.0 and np.all(np.isfinite(losses))
        if not defended:
            assert min(losses[1:]) < losses[0]
            assert flag == 1 or losses[-1] >= 0.0
        _agrees(model, adv, flag)
    finally:
        model.engine.close()


def test_hopskipjump_particle_swarm_and_kenansville_dispatch(tmp_path):
    model, audio, init, thr = _sv_setting(tmp_path)
    try:
        hsj = HopSkipJump("SV", "targeted", model, grid=7, max_rounds=1, num_evals_init=8, num_evals_max=8, max_iter=1, seed=3, verbose=False)
        adv, flag = hsj.attack(audio, None, threshold=thr, init=init)
        assert flag == 1 and np.asarray(adv).size == N_ATT          # the start is accepted: the walk returns an accepted row
        _agrees(model, adv, flag)
        pso = ParticleSwarm("SV", "targeted", model, max_iter=1, n_particles=5, seed=3, verbose=False)
        adv, flag = pso.attack(audio, None, threshold=thr)
        _agrees(model, adv, flag)
        # Kenansville removes spectral content until an accepted voice is rejected: a success is a rejected row
        kv = Kenansville("SV", "untargeted", model, window=100, grid=5, max_rounds=2, seed=3, verbose=False)
        adv, flag = kv.attack(init, None, threshold=thr, true=1)
        assert flag in (1, -1) and np.asarray(adv).size == N_ATT
        if flag == 1:
            assert model.make_decisions(np.asarray(adv).reshape(-1))[0] == -1
    finally:
        model.engine.close()


# ------------------------------------------------------------------------------------------------ 7: refusals, limits
def _refused(call, text, code=N.FB_E_STATE):
    with pytest.raises(N.NativeError) as ei:
        call()
    assert ei.value.code == code and text in str(ei.value), str(ei.value)


def test_refusals_by_name_and_limits_keep_the_loaded_system(eng):
    D = eng.feat_dim
    sy = _system(D)
    eng.load_xvector(sy, "OSI")
    wavs = [_wav(0, 6000), _wav(1, 3000)]
    before, _ = eng.score_raw(wavs)
    audio = synthetic_audio(0, 2000)
    p = nes_params("OSI", "targeted", target=1, max_iter=2)
    for on in (False, True):
        eng.set_wb_ivector(on)
        eng.set_wb_bpda(on)
        _refused(lambda: eng.get_grad_wb(p, audio), "x-vector system is loaded")
        _refused(lambda: eng.get_grad_wb_iter(p, audio, 1), "x-vector system is loaded")
        _refused(lambda: eng.attack_wb(p, audio), "x-vector system is loaded")
        _refused(lambda: eng.attack_cw2(p, cw2_params(search_steps=1), audio), "x-vector system is loaded")
        _refused(lambda: eng.attack_psy(p, cw2_params(search_steps=1), psy_params(np.ones((1, 1025)), 1.0), audio[:2048]), "not in this version")
    _refused(lambda: eng.set_feature_compression(0.5, 10), "not in this version")
    eng.set_feature_compression(None)
    w = wavs[0]
    occ, F, tv = np.empty(1), np.empty((1, D)), C.c_int()
    _refused(lambda: N.check(eng._L.fb_gmm_acc_stats(eng._h, N.ptr(w), C.c_int64(w.size), N.ptr(occ), N.ptr(F), C.byref(tv))),
             "not in this version")
    bad = [(synthetic_xvector_system(D + 1, 64, 96, 64, 32, 3), "front-end feature dim"),
           (synthetic_xvector_system(D, 64, 96, 48, 16, 3), "R=48 must be a multiple of 32"),
           (synthetic_xvector_system(D, 64, 96, 64, 32, 61), "at most 60 enrolled speakers"),
           (synthetic_xvector_system(D, 64, 96, 64, 32, 3, contexts=((-3, -2, -1, 0, 1, 2), (0,))), "n_ctx=6")]
    for s, text in bad:
        _refused(lambda: eng.load_xvector(s, "OSI"), text, N.FB_E_ARG)
        after, _ = eng.score_raw(wavs)
        assert np.array_equal(after, before), text
    _refused(lambda: eng.score_raw([wavs[0], np.zeros(4000, np.int16)]), "no voiced frames", N.FB_E_NO_VOICED)
    after, _ = eng.score_raw(wavs)
    assert np.array_equal(after, before)
