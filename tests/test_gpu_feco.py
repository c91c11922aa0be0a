"""Feature compression on the device (fb_set_feature_compression; the stage contract of include/fakebob_hip.h): the kernel
against the numpy restatement (tests/feco_ref.py) bit for bit, then the plumbing -- at ratio 1 the compressed rows are the
input, so every scoring and attack path must give the undefended bits --, scoring through a real compression against the
restatement, reproducibility of attacks on the randomised victim, the refusals and the enrolment statistics.

Bit-exact checks use np.array_equal.  The one tolerance is the project's full-size parity bound between a score and the
float64 mean of fb_debug_gmm_frames: 1e-4."""
import ctypes

import numpy as np
import pytest

from fakebob_amd import _native
from fakebob_amd._native import FB_E_ARG, NativeError
from fakebob_amd.engine import Engine, nes_params
from fakebob_amd.models import synthetic_audio, synthetic_ivector_system
from tests.feco_ref import feco, feco_batch, feco_k, feco_keys

pytestmark = pytest.mark.gpu
D = 72
N = 16000
SPD = 10
# unequal rows in one batch: the empty one in the middle, around a wave's 64 frames, more frames than one block of 64 per
# wave group, an NES row (300: LDS path up to ratio 0.5), and 700, which no LDS holds (the general path)
LENGTHS = [1, 2, 3, 63, 0, 64, 65, 257, 300, 700]
SEED, STREAM, EPOCH = 0xC0FFEE1234567, 5, 9


@pytest.fixture(scope="module")
def eng():
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def mats():
    rng = np.random.RandomState(11)
    return [(3.0 * rng.standard_normal((T, D))).astype(np.float32) for T in LENGTHS]


@pytest.fixture(scope="module")
def philox(oracle):
    return oracle.philox


def _check(got, want):
    assert len(got) == len(want)
    for b, (gr, wr) in enumerate(zip(got, want)):
        for j, (g, w) in enumerate(zip(gr, wr)):
            assert g.dtype == np.float32 and g.shape == w.shape, (b, j, g.shape, w.shape)
            assert np.array_equal(g.view(np.uint32), w.view(np.uint32)), (b, j, int(np.flatnonzero((g != w).any(axis=1))[0]))


# ------------------------------------------------------------------------------------- 1. the kernel, bit for bit
def test_keys_equal_the_contracts_words(eng, philox):
    for utt, rep, T in ((0, 0, 300), (7, 2, 65), (3, 31, 1)):
        got = eng.debug_feco_keys(SEED, STREAM, EPOCH, utt, rep, T)
        assert got.dtype == np.uint32 and np.array_equal(got, feco_keys(philox, SEED, STREAM, EPOCH, utt, rep, T))


@pytest.mark.parametrize("iters", [1, 10])
@pytest.mark.parametrize("ratio", [0.001, 0.2, 0.5, 1.0])
def test_kernel_equals_the_restatement(eng, mats, philox, ratio, iters):
    eng.set_feature_compression(ratio, iters)
    try:
        got = eng.debug_feature_compress(mats, 1, SEED, STREAM, EPOCH)       # one batch of unequal rows
        _check(got, feco_batch(philox, mats, 1, SEED, STREAM, EPOCH, ratio, iters))
        assert [g[0].shape[0] for g in got] == [feco_k(T, ratio) for T in LENGTHS]
        if ratio == 1.0:
            assert all(np.array_equal(g[0], m) for g, m in zip(got, mats))
        one = eng.debug_feature_compress([mats[8]], 1, SEED, STREAM, EPOCH)  # ... and alone: utterance row 0, other keys
        _check(one, feco_batch(philox, [mats[8]], 1, SEED, STREAM, EPOCH, ratio, iters))
    finally:
        eng.set_feature_compression(None)


@pytest.mark.parametrize("ratio", [0.2, 0.5])
def test_kernel_with_replicas(eng, mats, philox, ratio):
    sub = [mats[i] for i in (3, 4, 6, 8, 9)]                                # 63, 0, 65, 300, 700
    eng.set_feature_compression(ratio, 10)
    try:
        got = eng.debug_feature_compress(sub, 3, SEED, STREAM, EPOCH)
        _check(got, feco_batch(philox, sub, 3, SEED, STREAM, EPOCH, ratio, 10))
        r300 = got[3]
        assert not np.array_equal(r300[0], r300[1]) and not np.array_equal(r300[1], r300[2])   # a draw per replica
    finally:
        eng.set_feature_compression(None)


@pytest.mark.parametrize("ratio", [0.25, 1.0])
def test_kernel_on_repeated_rows(eng, philox, ratio):
    """ties (equal rows give equal distances: the lower centre wins) and centres that stay empty and keep their value"""
    rng = np.random.RandomState(12)
    base = (3.0 * rng.standard_normal((9, D))).astype(np.float32)
    X = base[rng.randint(0, 9, 130)]                      # 130 frames, 9 distinct rows: most chosen centres are duplicates
    Y = np.concatenate([X[:40], (3.0 * rng.standard_normal((40, D))).astype(np.float32)])
    eng.set_feature_compression(ratio, 10)
    try:
        got = eng.debug_feature_compress([X, Y], 2, SEED, STREAM, EPOCH)
        _check(got, feco_batch(philox, [X, Y], 2, SEED, STREAM, EPOCH, ratio, 10))
    finally:
        eng.set_feature_compression(None)
    keys = feco_keys(philox, SEED, STREAM, EPOCH, 0, 0, 130)
    _c, labels = feco(X, keys, ratio, 10)
    assert len(set(labels.tolist())) < feco_k(130, ratio)           # the case does hold an empty cluster


# ------------------------------------------------------------------------------------- 2. the plumbing, bit for bit
def _cast(x):
    return (np.asarray(x, np.float64) * 32768.0).astype(np.int64).astype(np.int16)


def _gmm(system, task="OSI"):
    ubm, spk = system
    e = Engine(0)
    if task == "SV":
        e.load_gmm([ubm, spk[0]])
    else:
        e.load_gmm([ubm] + spk)
    e.set_system(task)
    return e


def _iv(task="SV"):
    sy = synthetic_ivector_system(C=96, D=72, R=48, L=24, n_speakers=1, seed=11)
    sy = sy.with_enrolled(sy.enrolled, [-40.0], [10.0])
    e = Engine(0)
    e.load_ivector(sy, task)
    return e


def _same(a, b):
    return a[1] == b[1] and np.array_equal(a[0], b[0]) and np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])


@pytest.mark.parametrize("victim", ["gmm f64", "gmm f32", "ivector"])
def test_ratio_one_scores_as_undefended(small_system, victim):
    wavs = [_cast(synthetic_audio(u, n)) for u, n in ((1, 16000), (2, 48000), (3, 9000))]
    e = _iv() if victim == "ivector" else _gmm(small_system)
    try:
        if victim == "gmm f32":
            e.set_frontend(mfcc_f32=1)
        want, tv = e.score_raw(wavs)
        e.set_feature_compression(1.0, 10)
        got, tv2 = e.score_raw(wavs)
        assert np.array_equal(got, want) and np.array_equal(tv, tv2)     # tv stays the VAD's count
        e.set_feature_compression(None)
        assert np.array_equal(e.score_raw(wavs)[0], want)
    finally:
        e.close()


@pytest.mark.parametrize("victim", ["gmm OSI", "ivector SV"])
@pytest.mark.parametrize("fused", [True, False])
def test_ratio_one_attack_is_the_undefended_attack(small_system, monkeypatch, victim, fused):
    monkeypatch.delenv("FB_NO_FUSE", raising=False)
    e = _iv() if victim.startswith("ivector") else _gmm(small_system)
    try:
        e.set_fused_chain(fused)
        kw = dict(target=1) if victim == "gmm OSI" else {}
        task = victim.split()[1]
        p = nes_params(task, "targeted", samples_per_draw=SPD, max_iter=30, epsilon=0.002, threshold=1e3, seed=5, stream=1, **kw)
        audio = synthetic_audio(9, N)
        base = e.attack(p, audio)
        assert base[3].shape[0] == 30 and np.all(np.isfinite(base[3]))
        e.set_feature_compression(1.0, 3)
        assert _same(base, e.attack(p, audio))
        e.set_feature_compression(None)
        assert _same(base, e.attack(p, audio))
    finally:
        e.close()


def test_ratio_one_eot_attack_equals_the_plain_attack(small_system, monkeypatch):
    """a deterministic victim (ms:3, ratio 1): both replicas are the same rows, the mean of two equal values is exact"""
    monkeypatch.delenv("FB_NO_FUSE", raising=False)
    e = _gmm(small_system)
    try:
        e.set_input_transform("ms:3")
        e.set_feature_compression(1.0, 10)
        e.set_fused_chain(False)
        p = nes_params("OSI", "targeted", samples_per_draw=6, max_iter=6, target=1, epsilon=0.002, threshold=1e3, seed=5, stream=1)
        audio = synthetic_audio(9, N)
        base = e.attack(p, audio)
        e.set_fused_chain(None)
        e.set_eot(2)
        assert _same(base, e.attack(p, audio))
    finally:
        e.close()


# ------------------------------------------------------------------------------------- 3. a real compression
def test_scoring_through_a_compression(small_system, philox):
    ratio, iters, seed = 0.5, 10, 77
    w = _cast(synthetic_audio(4, N))
    e = _gmm(small_system)
    try:
        plain, _ = e.score_raw([w])
        feats, _T = e.debug_feats(w)                                   # the front end's hook: never compressed
        e.set_feature_compression(ratio, iters)
        assert np.array_equal(e.debug_feats(w)[0], feats)
        e.set_dither_seed(seed)
        got, tv = e.score_raw([w])                                     # scoring-call serial 0 of that seed
        assert tv[0] == feats.shape[0]
        keys = feco_keys(philox, seed, 0xFFFFFFFF, 0, 0, 0, feats.shape[0])
        C, _l = feco(feats, keys, ratio, iters)
        assert C.shape[0] == feco_k(feats.shape[0], ratio)
        e.set_feature_compression(None)
        want = e.debug_gmm_frames(C).mean(axis=1)
    finally:
        e.close()
    print("score through compression: max |diff| %.3g" % np.abs(got[0] - want).max())
    assert np.abs(got[0] - want).max() <= 1e-4
    assert np.abs(got[0] - plain[0]).min() > 1e-2                      # and it is another score than the undefended one


# ------------------------------------------------------------------------------------- 4. reproducibility
def _attack_once(system, r, stream=2, batch=None, warm=False, monkeypatch=None):
    if batch is not None:
        monkeypatch.setenv("FB_ATTACK_BATCH", str(batch))
    e = _gmm(system)
    try:
        e.set_feature_compression(0.5, 10)
        e.set_eot(r)
        kw = dict(samples_per_draw=6, max_iter=5, target=1, epsilon=0.002, threshold=1e3, seed=5)
        if warm:
            e.attack(nes_params("OSI", "targeted", stream=9, **kw), synthetic_audio(3, N))
        return e.attack(nes_params("OSI", "targeted", stream=stream, **kw), synthetic_audio(9, N))
    finally:
        e.close()
        if batch is not None:
            monkeypatch.delenv("FB_ATTACK_BATCH")


def test_an_attack_on_the_compressing_victim_depends_on_seed_and_stream_only(small_system, monkeypatch):
    monkeypatch.delenv("FB_ATTACK_BATCH", raising=False)
    a = _attack_once(small_system, 3)
    assert a[3].shape[0] == 5 and np.all(np.isfinite(a[3]))
    assert _same(a, _attack_once(small_system, 3))                                            # a fresh engine
    assert _same(a, _attack_once(small_system, 3, batch=1, monkeypatch=monkeypatch))
    assert _same(a, _attack_once(small_system, 3, batch=4, monkeypatch=monkeypatch))
    assert _same(a, _attack_once(small_system, 3, warm=True))                                 # after another attack
    assert not np.array_equal(a[3], _attack_once(small_system, 3, stream=3)[3])               # another stream differs
    assert not np.array_equal(a[3], _attack_once(small_system, 1)[3])                         # and r matters here


def test_scoring_calls_advance_the_serial(small_system):
    w = [_cast(synthetic_audio(4, N))]
    e = _gmm(small_system)
    try:
        e.set_feature_compression(0.5, 10)
        e.set_dither_seed(3)
        a, b = e.score_raw(w)[0], e.score_raw(w)[0]
        assert not np.array_equal(a, b)                                # a fresh initialisation per call
        e.set_dither_seed(3)
        assert np.array_equal(e.score_raw(w)[0], a) and np.array_equal(e.score_raw(w)[0], b)
    finally:
        e.close()


# ------------------------------------------------------------------------------------- 5. refusals, enrolment
def test_refusals(eng, mats, philox):
    eng.set_feature_compression(0.5, 2)
    try:
        for ratio, iters in ((0.0, 5), (-0.5, 10), (1.5, 10), (float("nan"), 10), (0.5, 0), (0.5, 65), (0.0, -1), (1.0000001, 1)):
            rc = eng._L.fb_set_feature_compression(eng._h, ctypes.c_double(ratio), ctypes.c_int(iters))
            assert rc == FB_E_ARG, (ratio, iters)
            with pytest.raises(NativeError):
                _native.check(rc)
        got = eng.debug_feature_compress([mats[6]], 1, SEED, STREAM, EPOCH)       # the previous setting was kept
        _check(got, feco_batch(philox, [mats[6]], 1, SEED, STREAM, EPOCH, 0.5, 2))
    finally:
        eng.set_feature_compression(None)
    with pytest.raises(NativeError):                                   # off: the hook has nothing to run
        eng.debug_feature_compress([mats[6]], 1, SEED, STREAM, EPOCH)


def test_not_applied_at_enrolment(small_system):
    ubm, _spk = small_system
    w = _cast(synthetic_audio(6, N))
    e = Engine(0)
    try:
        e.load_gmm([ubm])
        occ, F, tv = e.gmm_acc_stats(w)
        e.set_feature_compression(0.2, 10)
        occ2, F2, tv2 = e.gmm_acc_stats(w)
        assert tv == tv2 and np.array_equal(occ, occ2) and np.array_equal(F, F2)
    finally:
        e.close()
